"""Per-cell TSS counts, the aggregate TSS profile and per-cell fragments in peaks on the GPU (natac_cell_site_qc, csrc/natac_cellqc.hpp;
`pyatac cellqc`, nucleoatac_amd/pyatac/get_cellqc.py) against the NumPy restatements of tests/cellqc_ref.py.  Exact integers throughout:
equality, no tolerance.

The reach ladder gives one insertion exactly h sites in reach for every h at which the kernel changes its way (the lane / wave bound and
the tile size are read from include/natac.h), with record counts around the wave and the tile.  The two larger slice sizes -- the records
one sweep of the grid covers and the sites one launch takes, both read from the header too -- are passed together in one case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cellqc_ref as R
from conftest import ROOT
from helpers import bgzf_bytes

pytestmark = pytest.mark.gpu

_HDR = open(os.path.join(ROOT, "include", "natac.h")).read()
MAX_FLANK = int(re.search(r"#define NATAC_CELLQC_MAX_FLANK (\d+)", _HDR).group(1))
BLOCK = int(re.search(r"#define NATAC_CELLQC_BLOCK (\d+)", _HDR).group(1))
LANE_MAX = int(re.search(r"#define NATAC_CELLQC_LANE_MAX (\d+)", _HDR).group(1))
MAX_CELLS = int(re.search(r"#define NATAC_SPLIT_MAX_BARCODES (\d+)", _HDR).group(1))
MAX_BLOCKS = int(re.search(r"#define NATAC_CELLQC_MAX_BLOCKS (\d+)", _HDR).group(1))
SITE_CHUNK = int(re.search(r"#define NATAC_CELLQC_SITE_CHUNK (\d+)", _HDR).group(1))
REACH = sorted({0, 1, LANE_MAX, LANE_MAX + 1, 63, 64, 65, 4097})
RECORDS = sorted({1, 63, 64, 65, 257, BLOCK + 1})
FCE = [(1, 0, 1), (50, 10, 5), (1000, 500, 100), (MAX_FLANK, 0, 1)]


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i64(x):
    return np.ascontiguousarray(x, dtype=np.int64)


def test_constants_are_what_the_kernel_needs():
    # 2 * MAX_FLANK + 1 32-bit counters for each of the eight workgroups of a CU fit its 160 KiB of LDS; the defaults and 2,000 are allowed
    assert 2000 <= MAX_FLANK and (2 * MAX_FLANK + 1) * 4 * 8 <= 160 * 1024 and BLOCK % 64 == 0 and 1 <= LANE_MAX < 64
    # a step of a workgroup over the sites of one launch cannot wrap a 32-bit counter
    assert 2 * BLOCK * SITE_CHUNK < 1 << 32 and MAX_BLOCKS >= 1


def test_empty_inputs_each_way():
    pos, tlen, cell = _i64([10, 20]), _i64([100, 100]), np.array([0, 3], np.int32)
    sc, sm, ps, pe = _i64([60, 70]), np.array([0, 1], np.uint8), _i64([0]), _i64([500])
    for kw in (dict(pos=pos[:0], tlen=tlen[:0], cell=cell[:0], site_center=sc, site_minus=sm, peak_start=ps, peak_end=pe),     # no records
               dict(pos=pos, tlen=tlen, cell=cell),                                                                           # neither
               dict(pos=pos, tlen=tlen, cell=cell, site_center=sc[:0], site_minus=sm[:0], peak_start=ps[:0], peak_end=pe[:0])):
        out = _ctx().cell_site_qc(kw.pop("pos"), kw.pop("tlen"), kw.pop("cell"), 4, flank=50, center=10, edge=5, with_kernel_ms=True, **kw)
        assert [a.shape for a in out[:4]] == [(4,), (4,), (4,), (101,)] and all(a.dtype == np.int64 and not a.any() for a in out[:4])
        assert out[4] == 0
    # sites alone and peaks alone skip the other part
    out = _ctx().cell_site_qc(pos, tlen, cell, 4, sc, sm, 50, 10, 5, with_kernel_ms=True)
    R.assert_same(out, R.cellqc_brute(pos, tlen, cell, 4, sc, sm, 50, 10, 5, None, None))
    assert out[4] > 0 and out[3].sum() == 6 and not out[2].any()            # l = 14, 24 and r = 105, 115: 1 + 2 + 2 + 1 pairs
    out = _ctx().cell_site_qc(pos, tlen, cell, 4, None, None, 50, 10, 5, ps, pe)
    R.assert_same(out, R.cellqc_brute(pos, tlen, cell, 4, None, None, 50, 10, 5, ps, pe))
    assert out[2].tolist() == [1, 0, 0, 1] and not out[3].any() and not out[0].any()
    # records, sites and peaks, and nothing in reach
    out = _ctx().cell_site_qc(pos, tlen, cell, 4, sc + 100_000, sm, 50, 10, 5, ps + 100_000, pe + 100_000)
    assert not any(a.any() for a in out)


@pytest.mark.parametrize("fce", FCE)
@pytest.mark.parametrize("n_cells", [7, 1])
def test_mixed_seeded_case(fce, n_cells):
    flank, center, edge = fce
    pos, tlen, cell, sc, sm, ps, pe = R.mixed_case(23, n_cells, flank, center, edge)
    ilen = tlen - 8
    assert pos.min() < 0 and (ilen < 0).any() and (ilen == 0).any() and (ilen == 1).any() and np.all(np.diff(pos) >= 0)
    assert len(pos) == 2000 and len(sc) == 300 and len(ps) == 40 and sm.min() == 0 and sm.max() == 1 and np.any(np.diff(sc) == 0)
    assert np.any(pe - ps == 1) and np.any(ps[1:] == pe[:-1]) and np.all(ps[1:] >= pe[:-1])
    want = R.cellqc_brute(pos, tlen, cell, n_cells, sc, sm, flank, center, edge, ps, pe)
    R.assert_same(R.cellqc_ref(pos, tlen, cell, n_cells, sc, sm, flank, center, edge, ps, pe), want)
    # the exact distances are in the case: both ends of the profile are hit, and the classes change at their bounds
    assert want[3][0] > 0 and want[3][-1] > 0 and want[0].sum() > 0 and want[1].sum() > 0 and want[2].sum() > 100
    R.assert_same(_ctx().cell_site_qc(pos, tlen, cell, n_cells, sc, sm, flank, center, edge, ps, pe), want)
    # without strands every site is plus
    R.assert_same(_ctx().cell_site_qc(pos, tlen, cell, n_cells, sc, None, flank, center, edge, ps, pe),
                  R.cellqc_brute(pos, tlen, cell, n_cells, sc, None, flank, center, edge, ps, pe))


def _ladder_case(n_rec, flank=1000):
    """clusters 100,000 bases apart: cluster k has REACH[k] sites within flank of its base and two just outside; n_rec records have their
    left insertion at the base and their right one 30,000 further on, where no site is in reach"""
    rng = np.random.default_rng(n_rec)
    pos, sc = [], []
    for k, h in enumerate(REACH):
        base = 100_000 * (k + 1)
        inside = rng.integers(base - flank, base + flank + 1, h)
        if h >= 2:
            inside[:2] = [base - flank, base + flank]
        if h >= 64:
            inside[10:40] = base + 7                     # a run of one column inside a wave step
        sc += inside.tolist() + [base - flank - 1, base + flank + 1]
        pos += [base - 4] * n_rec
    sc = np.sort(_i64(sc))
    sm = rng.integers(0, 2, len(sc)).astype(np.uint8)
    pos = _i64(pos)
    tlen = np.full(len(pos), 30_000 + 9, np.int64)       # r = l + 30,000
    cell = rng.integers(0, 5, len(pos)).astype(np.int32)
    return pos, tlen, cell, sc, sm


@pytest.mark.parametrize("n_rec", RECORDS)
def test_reach_ladder(n_rec):
    flank, center, edge = 1000, 500, 100
    pos, tlen, cell, sc, sm = _ladder_case(n_rec)
    l = pos[::n_rec] + 4
    reach = np.searchsorted(sc, l + flank, "right") - np.searchsorted(sc, l - flank, "left")
    far = np.searchsorted(sc, l + 30_000 + flank, "right") - np.searchsorted(sc, l + 30_000 - flank, "left")
    assert reach.tolist() == REACH and not far.any()
    want = R.cellqc_ref(pos, tlen, cell, 5, sc, sm, flank, center, edge, None, None)
    assert want[3].sum() == n_rec * sum(REACH)
    if n_rec == 1:
        R.assert_same(R.cellqc_brute(pos, tlen, cell, 5, sc, sm, flank, center, edge, None, None), want)
    R.assert_same(_ctx().cell_site_qc(pos, tlen, cell, 5, sc, sm, flank, center, edge), want)
    # every cluster alone, with its own records only
    if n_rec in (1, 65):
        for k in range(len(REACH)):
            p, t, c = (a[k * n_rec:(k + 1) * n_rec] for a in (pos, tlen, cell))
            R.assert_same(_ctx().cell_site_qc(p, t, c, 5, sc, sm, flank, center, edge),
                          R.cellqc_ref(p, t, c, 5, sc, sm, flank, center, edge, None, None))


def test_minus_strand_reverses_the_profile_only():
    pos, tlen, cell, sc, sm, ps, pe = R.mixed_case(5, 7, 50, 10, 5)
    plus = _ctx().cell_site_qc(pos, tlen, cell, 7, sc, np.zeros(len(sc), np.uint8), 50, 10, 5, ps, pe)
    minus = _ctx().cell_site_qc(pos, tlen, cell, 7, sc, np.ones(len(sc), np.uint8), 50, 10, 5, ps, pe)
    assert np.array_equal(minus[3], plus[3][::-1]) and not np.array_equal(plus[3], plus[3][::-1])
    for a, b in zip(plus[:3], minus[:3]):
        assert np.array_equal(a, b)
    R.assert_same(plus, R.cellqc_brute(pos, tlen, cell, 7, sc, None, 50, 10, 5, ps, pe))


class _Store(object):
    """what get_cellqc.cell_qc reads of a tagged FragmentStore"""

    def __init__(self, parts):
        self.references = list(parts)
        self.pos = {c: p[0] for c, p in parts.items()}
        self.tlen = {c: p[1] for c, p in parts.items()}
        self.cell = {c: p[2] for c, p in parts.items()}


def test_splits_sum_to_the_single_call():
    from nucleoatac_amd.pyatac.get_cellqc import cell_qc
    flank, center, edge = 50, 10, 5
    pos, tlen, cell, sc, sm, ps, pe = R.mixed_case(8, 7, flank, center, edge)
    sc, sm = sc[140:152], sm[140:152]                    # a short list of sites
    whole = _ctx().cell_site_qc(pos, tlen, cell, 7, sc, sm, flank, center, edge, ps, pe)
    R.assert_same(whole, R.cellqc_brute(pos, tlen, cell, 7, sc, sm, flank, center, edge, ps, pe))
    assert whole[3].sum() > 50
    for cut in range(len(sc) + 1):                       # the sites at every point; the peaks go with the first part
        a = _ctx().cell_site_qc(pos, tlen, cell, 7, sc[:cut], sm[:cut], flank, center, edge, ps, pe)
        b = _ctx().cell_site_qc(pos, tlen, cell, 7, sc[cut:], sm[cut:], flank, center, edge)
        R.assert_same([x + y for x, y in zip(a, b)], whole)
    total = [np.zeros_like(a) for a in whole]            # the records in contiguous parts
    for lo, hi in ((0, 1), (1, 700), (700, 700), (700, 2000)):
        part = _ctx().cell_site_qc(pos[lo:hi], tlen[lo:hi], cell[lo:hi], 7, sc, sm, flank, center, edge, ps, pe)
        total = [x + y for x, y in zip(total, part)]
    R.assert_same(total, whole)
    # two chromosomes with tables of their own, a third without sites or peaks, a fourth without records: the sum in store order
    pos2, tlen2, cell2, sc2, sm2, ps2, pe2 = R.mixed_case(9, 7, flank, center, edge)
    store = _Store({"chrA": (pos, tlen, cell), "chrB": (pos2, tlen2, cell2), "chrC": (pos, tlen, cell), "chrD": (pos[:0], tlen[:0], cell[:0])})
    timing = {}
    got = cell_qc(store, 7, {"chrA": (sc, sm), "chrB": (sc2, sm2), "chrD": (sc, sm), "chrNowhere": (sc, sm)},
                  {"chrA": (ps, pe), "chrB": (ps2, pe2), "chrC": (ps[:0], pe[:0])}, flank, center, edge, timing=timing)
    other = R.cellqc_brute(pos2, tlen2, cell2, 7, sc2, sm2, flank, center, edge, ps2, pe2)
    R.assert_same(got, [x + y for x, y in zip(whole, other)])
    assert timing["kernel_ms"] > 0 and timing["device_s"] > 0


def test_cell_index_range():
    rng = np.random.default_rng(2)
    pos = np.sort(rng.integers(0, 3000, 500)).astype(np.int64)
    tlen = rng.integers(8, 300, 500).astype(np.int64)
    two = rng.integers(0, 2, 500).astype(np.int32)
    sc = np.sort(rng.integers(0, 3000, 40)).astype(np.int64)
    ps, pe = _i64([100, 900, 2000]), _i64([400, 901, 2600])
    want = R.cellqc_brute(pos, tlen, two, 2, sc, None, 50, 10, 5, ps, pe)
    got = _ctx().cell_site_qc(pos, tlen, two * (MAX_CELLS - 1), MAX_CELLS, sc, None, 50, 10, 5, ps, pe)
    for a, b in zip(got[:3], want[:3]):
        assert a.shape == (MAX_CELLS,) and a[[0, -1]].tolist() == b.tolist() and a.sum() == b.sum() and b.min() > 0
    assert np.array_equal(got[3], want[3])


def test_counts_past_2_to_the_32():
    n, c = 46_400, 1_000_000
    pos, tlen, cell = np.full(n, c - 4, np.int64), np.full(n, 9, np.int64), np.zeros(n, np.int32)        # ilen == 1: l == r == c
    tc, tf, ip, prof, ms = _ctx().cell_site_qc(pos, tlen, cell, 1, np.full(n, c, np.int64), None, 1000, 500, 100, with_kernel_ms=True)
    assert 92_800 * 46_400 == 4_305_920_000 > 1 << 32
    assert tc.tolist() == [4_305_920_000] and prof[1000] == 4_305_920_000 and prof.sum() == 4_305_920_000
    assert tf.tolist() == [0] and ip.tolist() == [0] and ms > 0


def test_one_over_the_grid_sweep_and_the_site_chunk():
    """more records than one sweep of the grid covers, so workgroups take a second step with their counters carried over, and more sites
    than one launch takes, so the host launches twice: the first launch has SITE_CHUNK sites, which makes it flush after every step
    (floor((2^32 - 1) / (2 * BLOCK * SITE_CHUNK)) == 1), and the peaks must count in it alone.  Most sites lie far below every record;
    3,000 lie among the records, with repeats and both strands, 1,000 of them in the first launch and 2,000 in the second."""
    assert ((1 << 32) - 1) // (2 * BLOCK * SITE_CHUNK) == 1
    rng = np.random.default_rng(41)
    n_rec, n_cells = MAX_BLOCKS * BLOCK + 20 * BLOCK + 44, 9         # twenty workgroups and one take a second step, the last a partial one
    pos = np.sort(rng.integers(0, 1_000_000, n_rec)).astype(np.int64)
    tlen = rng.integers(8, 700, n_rec).astype(np.int64)
    cell = rng.integers(0, n_cells, n_rec).astype(np.int32)
    far = -10_000_000_000 + 3 * np.arange(SITE_CHUNK - 1000, dtype=np.int64)
    near = np.sort(rng.integers(0, 1_000_000, 3000)).astype(np.int64)
    near[990:1010] = near[990]                           # one centre on both sides of the launch border
    near = np.sort(near)
    sc = np.concatenate([far, near])
    sm = rng.integers(0, 2, len(sc)).astype(np.uint8)
    assert len(sc) == SITE_CHUNK + 2000 and np.all(np.diff(sc) >= 0) and sc[SITE_CHUNK - 1] == sc[SITE_CHUNK]
    cuts = np.sort(rng.choice(1_000_000, 4000, replace=False)).astype(np.int64)
    ps, pe = cuts[0::2], cuts[1::2]
    flank, center, edge = 1000, 500, 100
    want = R.cellqc_ref(pos, tlen, cell, n_cells, sc, sm, flank, center, edge, ps, pe)
    first = R.cellqc_ref(pos, tlen, cell, n_cells, sc[:SITE_CHUNK], sm[:SITE_CHUNK], flank, center, edge, ps, pe)
    second = R.cellqc_ref(pos, tlen, cell, n_cells, sc[SITE_CHUNK:], sm[SITE_CHUNK:], flank, center, edge, None, None)
    R.assert_same([a + b for a, b in zip(first, second)], want)
    assert first[3].sum() > 500_000 and second[3].sum() > 1_000_000 and want[2].sum() > 100_000 and want[3].min() > 0
    # the records of the second step alone see sites of both launches
    tail = R.cellqc_ref(pos[MAX_BLOCKS * BLOCK:], tlen[MAX_BLOCKS * BLOCK:], cell[MAX_BLOCKS * BLOCK:], n_cells, sc, sm, flank, center, edge, ps, pe)
    assert tail[3].sum() > 100 and tail[2].sum() > 10
    got = _ctx().cell_site_qc(pos, tlen, cell, n_cells, sc, sm, flank, center, edge, ps, pe, with_kernel_ms=True)
    R.assert_same(got, want)
    assert got[4] > 0
    # the same records against the sites of the second launch alone, and against one site fewer than a launch takes
    R.assert_same(_ctx().cell_site_qc(pos, tlen, cell, n_cells, sc[SITE_CHUNK:], sm[SITE_CHUNK:], flank, center, edge), second)
    R.assert_same(_ctx().cell_site_qc(pos, tlen, cell, n_cells, sc[1:SITE_CHUNK], sm[1:SITE_CHUNK], flank, center, edge, ps, pe), first)


def _raw(pos, tlen, cell, n_cells, sc, sm, fce, ps, pe, nf=None, ns=None, n_peaks=None, outs="own"):
    """natac_cell_site_qc called directly with sentinel-filled outputs -> (return code, message, outputs)"""
    from nucleoatac_amd import _lib as L
    lib = L.load()
    out = [np.full(max(n_cells, 1) if k < 3 else 2 * MAX_FLANK + 1, -7, np.int64) for k in range(4)] if outs == "own" else outs
    ms = C.c_double(-7.0)
    rc = lib.natac_cell_site_qc(_ctx()._h, len(pos) if nf is None else nf, _vp(pos), _vp(tlen), _vp(cell), n_cells,
                                len(sc) if ns is None else ns, _vp(sc), _vp(sm), fce[0], fce[1], fce[2],
                                len(ps) if n_peaks is None else n_peaks, _vp(ps), _vp(pe), _vp(out[0]), _vp(out[1]), _vp(out[2]), _vp(out[3]), C.byref(ms))
    return rc, lib.natac_last_error().decode(), out + [ms.value]


def test_operand_checks_leave_the_outputs_untouched():
    fce = (50, 10, 5)
    pos, tlen, cell, sc, sm, ps, pe = R.mixed_case(4, 7, *fce)
    rc, _, out = _raw(pos, tlen, cell, 7, sc, sm, fce, ps, pe)
    want = R.cellqc_brute(pos, tlen, cell, 7, sc, sm, *fce, ps, pe)
    assert rc == 0 and out[4] > 0 and all(np.array_equal(a[:len(b)], b) for a, b in zip(out, want)) and np.all(out[3][101:] == -7) and np.all(out[0][7:] == -7)

    def refused(what, **kw):
        a = dict(pos=pos, tlen=tlen, cell=cell, n_cells=7, sc=sc, sm=sm, fce=fce, ps=ps, pe=pe)
        a.update(kw)
        rc, msg, out = _raw(**a)
        assert rc == -1 and what in msg, (kw.keys(), msg)                              # NATAC_E_ARG
        assert all(np.all(o == -7) for o in out[:4]) and out[4] == -7.0, kw.keys()         # kernel_ms is an output too

    bad = pos.copy()
    bad[1234] = bad[1233] - 1
    refused("pos must be non-decreasing (record 1234)", pos=bad)
    for k, v in ((1999, 7), (3, -1)):
        bad = cell.copy()
        bad[k] = v
        refused("record %d: cell %d outside [0, 7)" % (k, v), cell=bad)
    bad = sc.copy()
    bad[200] = bad[199] - 1
    refused("site centres must be ascending (site 200)", sc=bad)
    bad = ps.copy()
    bad[17] = pe[16] - 1
    refused("peaks must be disjoint and ascending (peak 17", ps=bad)
    bad = pe.copy()
    bad[30] = ps[30] - 1
    refused("peak 30: end", pe=bad)
    for f, what in (((0, 0, 1), "flank must be in [1, %d] (got 0)" % MAX_FLANK), ((MAX_FLANK + 1, 0, 1), "flank must be in"),
                    ((50, -1, 5), "center"), ((50, 10, 0), "edge"), ((50, 46, 5), "center + edge <= flank"), ((50, 10, 41), "center + edge <= flank")):
        refused(what, fce=f)
    refused("n_cells must be in [1, %d] (got 0)" % MAX_CELLS, n_cells=0)
    refused("n_cells must be in", n_cells=MAX_CELLS + 1)
    for kw in (dict(nf=-1), dict(ns=-1), dict(n_peaks=-1)):
        refused("negative size", **kw)
    for kw in (dict(pos=None, nf=5), dict(tlen=None), dict(cell=None), dict(sc=None, ns=3), dict(ps=None, n_peaks=2), dict(pe=None, n_peaks=2)):
        refused("null argument", **kw)
    keep = [np.full(7, -7, np.int64) for _ in range(3)] + [None]
    rc, msg, _ = _raw(pos, tlen, cell, 7, sc, sm, fce, ps, pe, outs=keep)
    assert rc == -1 and "null argument" in msg and all(np.all(o == -7) for o in keep[:3])
    # the bounds themselves pass: center + edge == flank, and the widest profile
    assert _raw(pos, tlen, cell, 7, sc, sm, (50, 45, 5), ps, pe)[0] == 0 and _raw(pos, tlen, cell, 7, sc, sm, (MAX_FLANK, 0, MAX_FLANK), ps, pe)[0] == 0
    with pytest.raises(ValueError):
        _ctx().cell_site_qc(pos, tlen, cell[:5], 7, sc, sm, *fce)
    with pytest.raises(ValueError):
        _ctx().cell_site_qc(pos, tlen, cell, 7, sc, sm[:5], *fce)
    for n in (0, -1, MAX_CELLS + 1, (1 << 32) + 7):       # before the binding narrows it to an int32
        with pytest.raises(ValueError, match="n_cells must be in"):
            _ctx().cell_site_qc(pos, tlen, cell, n, sc, sm, *fce)


# ---- pyatac cellqc ------------------------------------------------------------------------------------------------------------------------
def _crafted():
    """three chromosomes (chr3 has peaks and no sites; chrNoSites in the BEDs only), 12 listed cells of which the first six keep to the
    sites and peaks, and lines of a barcode that is not listed"""
    rng = np.random.default_rng(77)
    barcodes = [("%s-1" % "".join(rng.choice(list("ACGT"), 16))).encode() for _ in range(12)]
    tss = {"chr1": [(5000, 5001, "+"), (20_000, 20_011, "-"), (20_004, 20_006, "+"), (41_000, 41_002, "-")], "chr2": [(9000, 9001, "-")],
           "chrNoSites": [(100, 101, "+")]}
    peaks = {"chr1": [(4800, 5300), (5200, 5600), (19_000, 21_000), (19_500, 19_600), (30_000, 30_000)], "chr2": [(8500, 9500), (9500, 9700)],
             "chr3": [(100, 4000)], "chrNoSites": [(0, 500)]}
    lines = []
    for chrom, size in (("chr1", 50_000), ("chr2", 20_000), ("chr3", 8000)):
        recs = []
        for k, b in enumerate(barcodes + [b"NOTLISTED-1"]):
            n = 150 if k != 7 else 0                     # cell 7 has no line on chr1 and chr2 only
            start = rng.integers(0, size - 700, n)
            if k < 6 and chrom in tss:                   # around the sites
                at = np.array([s for s, _, _ in tss[chrom]])[rng.integers(0, len(tss[chrom]), n)]
                start = np.where(rng.random(n) < 0.7, at + rng.integers(-120, 60, n), start)
            recs += [(int(s), int(s + w), b) for s, w in zip(np.maximum(start, 0), rng.integers(1, 500, n))]
        if chrom == "chr3":
            recs = [r for r in recs if r[2] != barcodes[11]] + [(50, 90, barcodes[7])]
        recs.sort(key=lambda r: r[0])
        lines += [b"%s\t%d\t%d\t%s\t1\n" % (chrom.encode(), s, e, b) for s, e, b in recs]
    tss_text = "".join("%s\t%d\t%d\tg\t0\t%s\n" % (c, s, e, strand) for c, rows in tss.items() for s, e, strand in rows)
    peak_text = "".join("%s\t%d\t%d\n" % (c, s, e) for c, rows in peaks.items() for s, e in rows)
    return b"".join(lines), barcodes, tss_text.encode(), peak_text.encode()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from nucleoatac_amd.pyatac import get_cellqc as G
    from nucleoatac_amd.pyatac.chunk import read_bed_columns
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    d = tmp_path_factory.mktemp("cellqc_cli")
    text, barcodes, tss_text, peak_text = _crafted()
    frag, tss, peaks, table = str(d / "sample.fragments.tsv.gz"), str(d / "tss.bed"), str(d / "peaks.bed"), str(d / "cells.txt")
    open(frag, "wb").write(bgzf_bytes(text, blk=900))
    open(tss, "wb").write(tss_text)
    open(peaks, "wb").write(peak_text)
    open(table, "wb").write(b"barcode\tcluster\n" + b"".join(b"%s\tc%d\n" % (b, k % 3) for k, b in enumerate(barcodes)))
    store, bc_count, n_un = FragmentStore.cells_fragments_python(frag, barcodes)
    names, chrom, start, end, _ = read_bed_columns(peaks)
    merged = G.peaks_by_chrom(names, chrom, start, end)
    want = {}
    for strand_col in (6, None):                         # the restatement, chromosome by chromosome
        names, chrom, start, end, minus = read_bed_columns(tss, strand_col=strand_col)
        sites = G.sites_by_chrom(names, chrom, start, end, minus)
        n_sites = len(start)
        total = [np.zeros(12, np.int64) for _ in range(3)] + [np.zeros(2 * 200 + 1, np.int64)]
        for c in store.references:
            sc, sm = sites.get(c, (None, None))
            ps, pe = merged.get(c, (None, None))
            part = R.cellqc_brute(store.pos[c], store.tlen[c], store.cell[c], 12, sc, sm, 200, 50, 40, ps, pe)
            total = [a + b for a, b in zip(total, part)]
        want[strand_col] = total
    return dict(d=d, frag=frag, tss=tss, peaks=peaks, table=table, barcodes=barcodes, want=want, bc_count=bc_count, n_un=n_un, store=store,
                n_sites=n_sites, n_peaks=sum(len(p[0]) for p in merged.values()))


def test_command_end_to_end(files, tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac import get_cellqc as G
    from nucleoatac_amd.pyatac.cli import main
    monkeypatch.chdir(tmp_path)
    tc, tf, ip, prof = files["want"][6]
    assert files["store"].references == ["chr1", "chr2", "chr3"] and files["n_un"] == 450 and files["n_sites"] == 6 and files["n_peaks"] == 6
    geometry = ["--flank", "200", "--center", "50", "--edge", "40"]
    base = ["cellqc", "--fragments", files["frag"], "--cells", files["table"], "--header"] + geometry
    assert main(base + ["--tss", files["tss"], "--strand", "6", "--peaks", files["peaks"], "--min_tss_enrichment", "2.0", "--min_frip", "0.3"]) == 0
    assert capsys.readouterr().out.startswith("---------")
    ok, texts = G.finish(files["barcodes"], files["bc_count"], tc, tf, ip, prof, 200, 50, 40, 2.0, 0.3, files["n_un"], files["n_sites"],
                         files["n_peaks"])
    assert 0 < ok.sum() < 12 and ok[:6].all() and not ok[6:].any() and prof.sum() > 1000 and not np.array_equal(prof, prof[::-1])
    assert sorted(os.listdir(".")) == sorted("sample.fragments" + s for s in texts) and len(texts) == 4
    for suffix, text in texts.items():
        assert open("sample.fragments" + suffix, "rb").read() == text, suffix
    # the table of passing cells goes into cellcounts and split unchanged
    assert main(["cellcounts", "--fragments", files["frag"], "--bed", files["peaks"], "--cells", "sample.fragments.cellqc.cells.tsv", "--out", "cc"]) == 0
    assert open("cc.cellcounts.barcodes.tsv", "rb").read() == b"".join(b + b"\n" for b in files["barcodes"][:6])
    assert main(["split", "--fragments", files["frag"], "--groups", "sample.fragments.cellqc.cells.tsv", "--out", "sp"]) == 0
    assert os.path.exists("sp.selected.npz") and "selected\t6\t6\t" in open("sp.split.txt").read()
    # --peaks alone and --tss alone: the other columns hold NA, and there is no profile without sites
    assert main(base + ["--peaks", files["peaks"], "--min_frip", "0.3", "--out", "p"]) == 0
    _, texts = G.finish(files["barcodes"], files["bc_count"], None, None, ip, None, 200, 50, 40, None, 0.3, files["n_un"], 0, files["n_peaks"])
    assert sorted(x for x in os.listdir(".") if x.startswith("p.")) == sorted("p" + s for s in texts) and len(texts) == 3
    for suffix, text in texts.items():
        assert open("p" + suffix, "rb").read() == text, suffix
    assert main(base + ["--tss", files["tss"], "--strand", "6", "--out", "t"]) == 0
    ok, texts = G.finish(files["barcodes"], files["bc_count"], tc, tf, None, prof, 200, 50, 40, None, None, files["n_un"], files["n_sites"], 0)
    assert ok.all() and sorted(x for x in os.listdir(".") if x.startswith("t.")) == sorted("t" + s for s in texts) and len(texts) == 4
    for suffix, text in texts.items():
        assert open("t" + suffix, "rb").read() == text, suffix
    # without --strand every site is plus and is centred as plus
    assert main(base + ["--tss", files["tss"], "--out", "u"]) == 0
    tc, tf, _, prof_plus = files["want"][None]
    _, texts = G.finish(files["barcodes"], files["bc_count"], tc, tf, None, prof_plus, 200, 50, 40, None, None, files["n_un"], files["n_sites"], 0)
    assert not np.array_equal(prof_plus, prof)
    for suffix, text in texts.items():
        assert open("u" + suffix, "rb").read() == text, suffix
    capsys.readouterr()
