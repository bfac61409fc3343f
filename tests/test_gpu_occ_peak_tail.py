"""GPU: the occupancy peak tail (natac_run_occ_peaks -> natac_occ_peak_dist, the restatement of OccChunk.callPeaks' filter and
getNucDist, nucleoatac/Occupancy.py:225-240) on designed inputs, against a plain numpy restatement, BIT FOR BIT.

No stage runs: natac_batch_set_track writes OCC, OCC_LOWER, OCC_UPPER and OCC_COV, so every value the filter compares and every fragment
a window counts is placed by hand -- `lower` exactly on min_occ and one ulp above it, NaN and both infinities; coverage +0, -0, the
smallest denormal, -1, NaN; fragment centres on p - flank - 1, p - flank, p + flank, p + flank + 1 with sizes 0, 1, U - 1, U, U + 1 and
2000; a window of more than 256 fragments, many fragments of one centre, a kept peak whose window holds no size below U (0 / 0: the row
is NaN from there on, as numpy's), a chunk without peaks, one without fragments and one whose OCC track is flat (peaks where the
reference's jitter stream puts them).  With flank 150 and sep 60 the windows of the first and last peaks leave the chunk and count
fragments centred before 0 and at L and beyond (the packed margin).

nuc_dist can be held to bit equality: per size and kept peak both sides do one correctly rounded fp64 division and one addition, in
peak order, and the library is built without FMA contraction."""
import numpy as np
import pytest

from helpers import call_peaks_stable
from nucleoatac_amd import _lib as L
from nucleoatac_amd.packing import pack_chunks

pytestmark = pytest.mark.gpu

# (upper, flank, sep, min_occ): every upper in {2, 64, 200, 256} and every flank in {0, 1, 45, 60, 150}
TABLE = [(2, 0, 120, 0.1), (2, 60, 60, 0.3), (2, 150, 60, 0.1), (64, 0, 60, 0.1), (64, 1, 120, 0.3), (64, 45, 120, 0.0),
         (64, 150, 60, 0.1), (200, 1, 60, 0.1), (200, 45, 120, 0.1), (200, 60, 120, 0.3), (200, 150, 60, 0.0), (256, 0, 120, 0.1),
         (256, 45, 60, 0.1), (256, 60, 120, 0.1), (256, 150, 60, 0.3)]
LENS = [1500, 400, 977, 1203, 1411, 640, 555, 812]
DESIGNED, NAN_CHUNK, NO_PEAK, FLAT, NO_FRAGS = (0, 1, 2, 3, 4), 1, 5, 6, 7
GAP = 20000                       # genomic distance between chunk starts: no chunk sees another one's fragments
MARGIN = 2200                     # >= flank + upper, and wide enough for a 2000-base fragment centred next to a chunk


def _restate(occ, lower, cov, l, n, min_occ, sep, flank, U):
    """Occupancy.py:225-240 in numpy: (peaks, keep, nuc_dist) of one chunk.  call_peaks is the oracle's with reduce_peaks' argsort made
    stable (helpers.call_peaks_stable): the flat chunk's peaks are all of one height, where numpy's default sort may visit them in any
    order; wherever heights differ it is the oracle's call_peaks unchanged."""
    peaks = np.asarray(call_peaks_stable(occ.copy(), min_signal=min_occ, sep=sep, boundary=sep // 2, order=1), np.int64)
    with np.errstate(invalid="ignore"):
        keep = (lower[peaks] > min_occ) & (cov[peaks] > 0)
    cen = l + (n - 1) // 2
    nd = np.zeros(U)
    for p in peaks[keep]:                                  # ascending
        sel = (cen >= p - flank) & (cen <= p + flank) & (n >= 0) & (n < U)
        h = np.bincount(n[sel], minlength=U).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            nd += h / float(h.sum())
    return peaks, keep, nd


def _peak_positions(Lc, sep, dense=True):
    """designed peaks: the first on the boundary sep // 2, the last on L - boundary - 1, some exactly `sep` apart (none is reduced)"""
    bnd = sep // 2
    out, p, i = [], bnd, 0
    while p <= Lc - bnd - 1 - sep:
        out.append(p)
        p += sep + (i % 3 if dense else 3 * sep)
        i += 1
    return out + [Lc - bnd - 1]


def _tracks(rng, lens, sep, min_occ, dense=True):
    """OCC with a designed peak set over a base below min_occ, and the values the filter meets at the peaks: a chunk's first and last
    peak are kept (kept lower x kept coverage), of every three peaks between them one is kept and the others walk through kept lower x
    dropped coverage, dropped lower x kept coverage and dropped x dropped"""
    up1 = np.nextafter(min_occ, 1)
    kk = [(up1, 3.0), (np.inf, 5e-324), (up1, 5e-324), (np.inf, 3.0)]
    rest = [(lo, cv) for lo in (up1, np.inf) for cv in (0.0, -0.0, -1.0, np.nan)] + \
           [(lo, cv) for lo in (min_occ, np.nan, -np.inf) for cv in (5e-324, 3.0)] + [(np.nan, np.nan), (min_occ, 0.0)]
    occ, lower, upper, cov, peaks = [], [], [], [], []
    i = 0
    for k, Lc in enumerate(lens):
        o = np.full(Lc, min_occ - 0.05)
        lo = rng.random(Lc)
        cv = np.floor(rng.random(Lc) * 4)
        pk = []
        if k in DESIGNED or k == NO_FRAGS:
            pk = _peak_positions(Lc, sep, dense)
            o[pk] = min_occ + 0.2 + 0.4 * rng.random(len(pk))
            for j, p in enumerate(pk):
                if k == NO_FRAGS or (k == NAN_CHUNK and j == len(pk) - 1):
                    lo[p], cv[p] = np.inf, 3.0                    # kept, whatever the window holds
                elif j in (0, len(pk) - 1):
                    lo[p], cv[p] = kk[(k + j) % 4]                # the peaks next to the chunk's ends are kept
                else:
                    lo[p], cv[p] = kk[(i // 3) % 4] if i % 3 == 0 else rest[(i - i // 3 - 1) % len(rest)]
                    i += 1
            if k == 0:
                o[pk[1]] = min_occ                                # a peak exactly at min_signal is a peak (>=)
            if k == 2:
                o[pk[0] + 5:pk[0] + 25] = np.nan                  # call_peaks fills a NaN stretch with the chunk's minimum
        elif k == NO_PEAK:
            o = min_occ + np.linspace(0.0, 0.5, Lc)               # monotone: no local maximum
        elif k == FLAT:
            o[:] = min_occ + 0.7
            lo = min_occ + 0.01 + rng.random(Lc)
            cv[:] = 2.0
        occ.append(o); lower.append(lo); upper.append(rng.random(Lc) + 1.0); cov.append(cv); peaks.append(pk)
    return [np.concatenate(x) for x in (occ, lower, upper, cov)], peaks


def _fragments(rng, lens, peaks, flank, U):
    """absolute (l, n) sorted by l: around every designed peak the window's inclusive ends and the first centre outside on either side,
    each with the sizes around U; a crowd of 300 in the second peak's window of chunk 0 and 100 of one centre on the fifth (both kept); random
    ones everywhere.  The last peak of NAN_CHUNK keeps only sizes >= U in its window."""
    cs, ns = [], []
    for k, Lc in enumerate(lens):
        if k == NO_FRAGS:
            continue
        nr = 400 if k == FLAT else 120
        c = [rng.integers(-flank - 40, Lc + flank + 40, size=nr)]
        n = [np.where(rng.random(nr) < 0.5, rng.integers(0, U, size=nr), rng.integers(0, U + 30, size=nr))]
        for j, p in enumerate(peaks[k]):
            for cen in (p - flank - 1, p - flank, p + flank, p + flank + 1):
                c.append(np.full(6, cen)); n.append(np.array([0, 1, U - 1, U, U + 1, 2000]))
            if k == 0 and j == 1:
                c.append(rng.integers(p - flank, p + flank + 1, size=300)); n.append(rng.integers(0, U + 5, size=300))
            if k == 0 and j == 4:
                c.append(np.full(100, p)); n.append(rng.integers(0, U + 5, size=100))
        c, n = np.concatenate(c), np.concatenate(n)
        if k == NAN_CHUNK:
            p = peaks[k][-1]
            drop = (c >= p - flank) & (c <= p + flank) & (n < U)
            c, n = c[~drop], n[~drop]
        cs.append(c + k * GAP); ns.append(n)
    c, n = np.concatenate(cs).astype(np.int64), np.concatenate(ns).astype(np.int64)
    l = c - (n - 1) // 2                                   # centre = l + (n - 1) // 2 with floor division: size 0 sits at l - 1
    o = np.argsort(l, kind="stable")
    return l[o], n[o]


def _pack(lens, l, n):
    return pack_chunks([("c", k * GAP, k * GAP + Lc) for k, Lc in enumerate(lens)], {"c": l}, {"c": n}, margin=MARGIN)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check(b, pk, tracks, min_occ, sep, flank, U):
    """one natac_run_occ_peaks against the restatement; returns the restatement's (peaks, keep, nuc_dist) per chunk"""
    cc, cp, occ, lo, up, rd, keep, nd = b.run_occ_peaks(min_occ=min_occ, sep=sep)
    assert nd.shape == (pk.n_chunks, U)
    t = [b.split(x) for x in tracks]
    out = []
    for k in range(pk.n_chunks):
        l, n = pk.chunk_frags(k)
        peaks, kp, ref_nd = _restate(t[0][k], t[1][k], t[3][k], l.astype(np.int64), n.astype(np.int64), min_occ, sep, flank, U)
        m = cc == k
        assert np.array_equal(cp[m], peaks), ("peaks", k)
        for got, tr, name in ((occ, t[0][k], "occ"), (lo, t[1][k], "lower"), (up, t[2][k], "upper"), (rd, t[3][k], "reads")):
            assert np.array_equal(_bits(got[m]), _bits(tr[peaks])), (name, k)       # the very bits: -0.0, NaN, the denormal
        assert np.array_equal(keep[m].astype(bool), kp), ("keep", k)
        assert np.array_equal(nd[k], ref_nd, equal_nan=True), ("nuc_dist", k, int(np.sum(nd[k] != ref_nd)))
        out.append((peaks, kp, ref_nd))
    assert np.array_equal(cc, np.sort(cc))
    return out


def _set_tracks(b, tracks):
    for t, v in zip((L.T_OCC, L.T_OCC_LOWER, L.T_OCC_UPPER, L.T_OCC_COV), tracks):
        b.set_track(t, v)


def _model(U):
    p = np.arange(1, U + 1, dtype=np.float64)
    return p / p.sum(), p[::-1] / p.sum()


@pytest.mark.parametrize("U,flank,sep,min_occ", TABLE)
def test_occ_peak_tail_designed(U, flank, sep, min_occ):
    from nucleoatac_amd.device import Context
    rng = np.random.default_rng([U, flank, sep])
    tracks, peaks = _tracks(rng, LENS, sep, min_occ)
    l, n = _fragments(rng, LENS, peaks, flank, U)
    pk = _pack(LENS, l, n)
    assert MARGIN >= flank + U
    with Context(0) as c:
        c.set_occ_model(*_model(U), step=5, flank=flank)
        b = c.upload(pk)
        _set_tracks(b, tracks)                         # natac_run_occ never runs
        ref = _check(b, pk, tracks, min_occ, sep, flank, U)
        b.free()
    # the design is what it claims to be
    off = np.concatenate(([0], np.cumsum(LENS)))
    up1 = np.nextafter(min_occ, 1)
    met = set()
    for k in DESIGNED:
        assert np.array_equal(ref[k][0], peaks[k])     # every designed peak is found, none is reduced
        met |= {(repr(float(a)), repr(float(c_))) for a, c_ in zip(tracks[1][off[k] + ref[k][0]], tracks[3][off[k] + ref[k][0]])}
    for lo in (up1, np.inf):
        for cv in (0.0, -0.0, -1.0, np.nan):
            assert (repr(float(lo)), repr(float(cv))) in met
    for lo in (min_occ, np.nan, -np.inf):
        for cv in (5e-324, 3.0):
            assert (repr(float(lo)), repr(float(cv))) in met
    assert all(ref[k][1].sum() >= 2 for k in DESIGNED)
    assert len(ref[NO_PEAK][0]) == 0 and not ref[NO_PEAK][2].any()
    assert len(ref[FLAT][0]) >= 3 and ref[FLAT][1].all()
    assert flank < 45 or np.isfinite(ref[FLAT][2]).all()       # (a window of one or three bases may well be empty)
    assert ref[NO_FRAGS][1].all() and np.isnan(ref[NO_FRAGS][2]).all()
    assert np.isnan(ref[NAN_CHUNK][2]).all()           # the empty window of its last kept peak
    for k in (0, 2, 3, 4):
        assert np.isfinite(ref[k][2]).all() and ref[k][2].sum() > 1.5
    if flank == 150:                                   # windows that leave the chunk on both sides and hold fragments there
        for k in (0, 2, 3, 4):
            lk, nk = pk.chunk_frags(k)
            cen = lk.astype(np.int64) + (nk.astype(np.int64) - 1) // 2
            kept = ref[k][0][ref[k][1]]
            first, last = kept[0], kept[-1]
            assert first < flank and last >= LENS[k] - flank
            assert ((cen < 0) & (cen >= first - flank) & (nk < U)).any() and ((cen >= LENS[k]) & (cen <= last + flank) & (nk < U)).any()


def test_occ_peak_tail_state_between_calls():
    """one batch, searched again after OCC is rewritten: 5 designed peaks per long chunk, then more than n + n / 4 + 16 (the peak value
    arrays grow), then fewer; then natac_set_occ_model with another `upper` on the batch that never ran natac_run_occ: nuc_dist is
    re-allocated and its width follows.  Every result equals the restatement."""
    from nucleoatac_amd.device import Context
    U, flank, min_occ = 64, 45, 0.1
    rng = np.random.default_rng(77)
    sparse, peaks_sparse = _tracks(rng, LENS, 120, min_occ, dense=False)
    dense, peaks_dense = _tracks(rng, LENS, 60, min_occ)
    l, n = _fragments(rng, LENS, peaks_dense, flank, U)
    pk = _pack(LENS, l, n)
    with Context(0) as c:
        c.set_occ_model(*_model(U), step=5, flank=flank)
        b = c.upload(pk)
        _set_tracks(b, sparse)
        n1 = sum(len(r[0]) for r in _check(b, pk, sparse, min_occ, 120, flank, U))
        _set_tracks(b, dense)
        n2 = sum(len(r[0]) for r in _check(b, pk, dense, min_occ, 60, flank, U))
        assert n2 > n1 + n1 // 4 + 16
        b.set_track(L.T_OCC, sparse[0])
        mixed = [sparse[0]] + dense[1:]
        n3 = sum(len(r[0]) for r in _check(b, pk, mixed, min_occ, 120, flank, U))
        assert n3 < n2
        for U2 in (200, 2):
            c.set_occ_model(*_model(U2), step=5, flank=flank)
            _check(b, pk, mixed, min_occ, 120, flank, U2)
        b.free()
