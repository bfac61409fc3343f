"""Per-cell TSS counts, the aggregate TSS profile and per-cell fragments in peaks (natac_cell_site_qc, `pyatac cellqc`) restated in NumPy
from the rule of include/natac.h, not from the kernel.

A record is l = pos + 4, ilen = tlen - 8, r = l + ilen - 1; every record counts, both insertions l and r on their own.  For an insertion x
and a site (c, minus): d = x - c, or c - x on minus; with |d| <= flank the pair adds to profile[d + flank], to tss_center[cell] if
|d| <= center and to tss_flank[cell] if |d| > flank - edge.  A record with l or r in some interval [start, end) adds 1 to in_peaks[cell].

cellqc_brute   every insertion against every site, every record against every interval: a dense comparison, for small shapes
cellqc_ref     searchsorted / bincount, for the larger shapes and the benchmark; assumes, like the device, ascending centres and disjoint
               ascending intervals."""
import numpy as np


def _i64(x):
    return np.asarray(x, dtype=np.int64)


def _ends(pos, tlen):
    l = _i64(pos) + 4
    return l, l + (_i64(tlen) - 8) - 1


def cellqc_brute(pos, tlen, cell, n_cells, site_center, site_minus, flank, center, edge, peak_start, peak_end):
    """-> (tss_center, tss_flank, in_peaks int64[n_cells], profile int64[2 * flank + 1])"""
    l, r = _ends(pos, tlen)
    cell = np.asarray(cell, np.int64)
    sc = _i64([] if site_center is None else site_center)
    sm = np.zeros(len(sc), bool) if site_minus is None else np.asarray(site_minus).astype(bool)
    tss_center, tss_flank, in_peaks = (np.zeros(n_cells, np.int64) for _ in range(3))
    profile = np.zeros(2 * flank + 1, np.int64)
    for x in (l, r):
        d = x[:, None] - sc[None, :]
        d = np.where(sm[None, :], -d, d)
        reach = np.abs(d) <= flank
        np.add.at(profile, d[reach] + flank, 1)
        np.add.at(tss_center, cell, (reach & (np.abs(d) <= center)).sum(axis=1))
        np.add.at(tss_flank, cell, (reach & (np.abs(d) > flank - edge)).sum(axis=1))
    ps, pe = _i64([] if peak_start is None else peak_start), _i64([] if peak_end is None else peak_end)
    inside = np.zeros(len(l), bool)
    for x in (l, r):
        inside |= ((x[:, None] >= ps[None, :]) & (x[:, None] < pe[None, :])).any(axis=1)
    np.add.at(in_peaks, cell, inside.astype(np.int64))
    return tss_center, tss_flank, in_peaks, profile


def cellqc_ref(pos, tlen, cell, n_cells, site_center, site_minus, flank, center, edge, peak_start, peak_end):
    """the same four arrays without the dense comparison"""
    l, r = _ends(pos, tlen)
    cell = np.asarray(cell, np.int64)
    sc = _i64([] if site_center is None else site_center)
    sm = np.zeros(len(sc), bool) if site_minus is None else np.asarray(site_minus).astype(bool)
    tss_center, tss_flank, in_peaks = (np.zeros(n_cells, np.int64) for _ in range(3))
    profile = np.zeros(2 * flank + 1, np.int64)
    if len(sc) and len(l):
        for x in (l, r):
            def within(w):
                return np.searchsorted(sc, x + w, "right") - np.searchsorted(sc, x - w, "left")
            lo = np.searchsorted(sc, x - flank, "left")
            n = within(flank)
            tss_center += np.bincount(cell, weights=within(center), minlength=n_cells).astype(np.int64)
            tss_flank += np.bincount(cell, weights=n - within(flank - edge), minlength=n_cells).astype(np.int64)
            # the pairs: insertion i with sites lo[i] .. lo[i] + n[i]
            which = np.repeat(np.arange(len(x)), n)
            j = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n) + np.repeat(lo, n)
            d = x[which] - sc[j]
            d = np.where(sm[j], -d, d)
            profile += np.bincount(d + flank, minlength=2 * flank + 1)
    ps, pe = _i64([] if peak_start is None else peak_start), _i64([] if peak_end is None else peak_end)
    if len(ps) and len(l):
        inside = np.zeros(len(l), bool)
        for x in (l, r):
            k = np.searchsorted(ps, x, "right") - 1
            inside |= (k >= 0) & (x < pe[np.maximum(k, 0)])
        in_peaks += np.bincount(cell[inside], minlength=n_cells)
    return tss_center, tss_flank, in_peaks, profile


def assert_same(got, want):
    assert len(got) >= 4
    for name, a, b in zip(("tss_center", "tss_flank", "in_peaks", "profile"), got, want):
        assert a.dtype == np.int64 and a.shape == b.shape and np.array_equal(a, b), name


def mixed_case(seed, n_cells, flank, center, edge):
    """the mixed seeded case: 2,000 records with pos in [-30, 5000) and tlen in [0, 400) (so ilen is negative, 0 and 1 too), 300 sites with
    repeats and both strands, 40 disjoint intervals with length 1 and touching ones; insertions at exactly d = +-flank, +-center,
    +-(flank - edge) and one beyond each, around one site of either strand"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(-30, 5000, 2000).astype(np.int64)
    tlen = rng.integers(0, 400, 2000).astype(np.int64)
    tlen[:6] = [7, 8, 9, 0, 3, 8]                        # ilen -1, 0, 1, -8, -5, 0
    sc = rng.integers(-40, 5200, 300).astype(np.int64)
    sc[100:130] = sc[:30]                                # repeats
    sc[130:140] = sc[0]
    sm = rng.integers(0, 2, 300).astype(np.uint8)
    sc[298], sm[298], sc[299], sm[299] = 2500, 0, 9000 + flank, 1        # the sites the exact distances are built around
    k = 100
    for c, sign in ((2500, 1), (9000 + flank, -1)):
        for w in (flank, center, flank - edge):
            for d in (w, -w, w + 1, -w - 1):
                pos[k], tlen[k] = c + sign * d - 4, 9    # l == r == c + sign * d
                pos[k + 1], tlen[k + 1] = c + sign * d - 4 - 150, 159        # r == c + sign * d, l 150 before
                k += 2
    o = np.argsort(pos, kind="stable")
    pos, tlen = pos[o], tlen[o]
    cell = rng.integers(0, n_cells, 2000).astype(np.int32)
    o = np.argsort(sc, kind="stable")
    sc, sm = sc[o], sm[o]
    cuts = np.sort(rng.choice(np.arange(-20, 5100), 80, replace=False)).astype(np.int64)
    ps, pe = cuts[0::2].copy(), cuts[1::2].copy()
    ps[5] = pe[4]                                        # touching
    ps[9] = pe[8]
    pe[20] = ps[20] + 1                                  # length 1
    pe[21] = ps[21] + 1
    return pos, tlen, cell, sc, sm, ps, pe
