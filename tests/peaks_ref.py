"""The rule of `pyatac peaks` (natac_enriched_regions, include/natac.h) restated in NumPy: bincount, cumsum, clipped differences,
flatnonzero.  Written from the rule's text, not from the kernels; the device must agree with it exactly, in every array."""
import numpy as np
from scipy.special import gammaincinv

K_TABLE = 65536


def critical_rates(mlog10p, n_table=K_TABLE):
    """Lam[k]: the largest rate at which a Poisson count reaches k with probability at most 10^-mlog10p (Lam[0] = 0)"""
    lam = np.zeros(n_table, np.float64)
    lam[1:] = gammaincinv(np.arange(1, n_table, dtype=np.float64), 10.0 ** -float(mlog10p))
    return lam


def tables(h, S, L, mlog10p, n_table=K_TABLE):
    """(Lam, thr_small int32, thr_large int32)"""
    lam = critical_rates(mlog10p, n_table)
    top = 2 ** 31 - 1           # no count reaches it (fewer than 2^30 records a call), so the clip changes no verdict
    return (lam, np.minimum(np.floor(lam * (2 * S + 1) / (2 * h + 1)), top).astype(np.int32),
            np.minimum(np.floor(lam * (2 * L + 1) / (2 * h + 1)), top).astype(np.int32))


def min_pileup(lam, lam_g):
    """max(1, the smallest k with Lam[k] >= lam_g); None when no k of the table has"""
    k = int(np.searchsorted(lam, lam_g, "left"))
    return None if k >= len(lam) else max(1, k)


def insertions(pos, tlen, n):
    """the kept insertions of one chromosome of length n (either end is dropped on its own outside [0, n))"""
    pos, tlen = np.asarray(pos, np.int64), np.asarray(tlen, np.int64)
    x = np.concatenate([pos + 4, pos + tlen - 5])
    return x[(x >= 0) & (x < n)]


def window_counts(cum, n, w):
    """C_w(x) for every base, cum = the insertions in [0, j)"""
    x = np.arange(n, dtype=np.int64)
    return cum[np.minimum(x + w + 1, n)] - cum[np.maximum(x - w, 0)]


def enriched_regions(pos, tlen, n, h, S, L, max_gap, min_length, min_pile, thr_small, thr_large, counts=False):
    """(start, end, summit int64; pileup, n_small, n_large int32) of the kept regions, ascending; counts: also (regions before the
    length rule, significant bases)"""
    cum = np.concatenate([[0], np.cumsum(np.bincount(insertions(pos, tlen, n), minlength=n))]).astype(np.int64)
    p, s, g = (window_counts(cum, n, w) for w in (h, S, L))
    k = np.minimum(p, len(thr_small) - 1)
    sig = np.flatnonzero((p >= min_pile) & (s <= np.asarray(thr_small, np.int64)[k]) & (g <= np.asarray(thr_large, np.int64)[k]))
    out = [[] for _ in range(6)]
    found = 0
    if len(sig):
        cut = np.flatnonzero(np.diff(sig) - 1 > max_gap)          # more than max_gap non-significant bases in between
        first = sig[np.concatenate([[0], cut + 1])]
        last = sig[np.concatenate([cut, [len(sig) - 1]])]
        found = len(first)
        for a, b in zip(first.tolist(), last.tolist()):
            if b + 1 - a < min_length:
                continue
            top = a + np.flatnonzero(p[a:b + 1] == p[a:b + 1].max())
            c = int(top[0] + top[-1]) // 2
            for o, v in zip(out, (a, b + 1, c, p[c], s[c], g[c])):
                o.append(int(v))
    res = tuple(np.asarray(o, t) for o, t in zip(out, (np.int64,) * 3 + (np.int32,) * 3))
    return res + (found, len(sig)) if counts else res


def hotspot_chromosome(seed, n=60000, n_uniform=3000, hotspots=5, per_hotspot=400, spread=60, flush=True):
    """sorted (pos, tlen) of a chromosome with planted hotspots; flush: the first and the last one lie against the chromosome's ends"""
    rng = np.random.RandomState(seed)
    centres = rng.randint(n // 10, n - n // 10, hotspots)
    if flush and hotspots >= 2:
        centres[0], centres[-1] = 40, n - 40
    pos = [rng.randint(-50, n - 20, n_uniform)]
    for c in centres:
        pos.append(c + rng.randint(-spread, spread + 1, per_hotspot) - 60)
    pos = np.sort(np.concatenate(pos)).astype(np.int64)
    tlen = rng.randint(30, 220, len(pos)).astype(np.int64)
    return pos, tlen


def spike_chromosome(seed, n=20000, n_uniform=1000, spikes=6, per_spike=30):
    """sorted (pos, tlen) with point hotspots (every l of a spike at one base, some two and three bases further on): what the small
    geometry (h = 2, S = 5, L = 20) finds improbable"""
    rng = np.random.RandomState(seed)
    pos = [rng.randint(-20, n - 10, n_uniform)]
    for c in rng.randint(100, n - 100, spikes):
        pos.append(np.full(per_spike, c - 4) + rng.choice([0, 0, 0, 0, 2, 3], per_spike))
    pos = np.sort(np.concatenate(pos)).astype(np.int64)
    return pos, rng.randint(30, 220, len(pos)).astype(np.int64)
