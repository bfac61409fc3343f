"""The enriched regions of a chromosome on the GPU (natac_enriched_regions, csrc/natac_peakcall.hpp; `pyatac peaks`,
nucleoatac_amd/pyatac/get_peaks.py) against the NumPy restatement of tests/peaks_ref.py.  Everything the device decides is integer
arithmetic, so every case is equality in all six arrays, without a tolerance.

The constructed cases pass tables made by hand (the device sees nothing else of the statistics): OPEN admits every count, so a base is
significant exactly when its pileup reaches min_pileup, and one insertion with half_width 1 is a run of three significant bases."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import peaks_ref as R
from conftest import ROOT
from helpers import bgzf_bytes
from peaks_ref import FIRST_CAPACITY, OPEN, SEGMENT, SHORT_MAX, at, real_tables      # (natac.h's sizes; shared with the host checks)

pytestmark = pytest.mark.gpu

DEFAULT = (75, 500, 5000, 75, 150)           # half_width, small, large, max_gap, min_length


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _i64(x):
    return np.ascontiguousarray(x, dtype=np.int64)


def assert_same(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        if isinstance(b, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), "array %d: %s != %s" % (k, a[:8], b[:8])
        else:
            assert a == b, "value %d: %s != %s" % (k, a, b)


def both(pos, tlen, n, geom, min_pile, ts, tl, **kw):
    """the device's answer, checked equal to the restatement's (with the two counts) -> the restatement's"""
    h, S, L, gap, length = geom
    want = R.enriched_regions(pos, tlen, n, h, S, L, gap, length, min_pile, ts, tl, counts=True)
    got = _ctx().enriched_regions(pos, tlen, n, ts, tl, min_pile, h, S, L, gap, length, with_counts=True, **kw)
    assert_same(got, want)
    return want


def test_constants():
    assert SEGMENT >= 1 << 20 and SHORT_MAX % 64 == 0 and FIRST_CAPACITY < 20000      # (the many-regions case must pass the first guess)


# ---- random chromosomes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_chromosomes_default_geometry(seed):
    n = 60000 - seed * 7001
    pos, tlen = R.hotspot_chromosome(seed, n=n, n_uniform=1000 + 1000 * seed)
    assert 1000 <= len(pos) <= 6000
    want = both(pos, tlen, n, DEFAULT, *real_tables(pos, tlen, n, 75, 500, 5000, 5))
    assert len(want[0]) >= 3 and want[0][0] == 0 and want[1][-1] == n         # a hotspot flush against each end


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("max_gap", [0, 3])
def test_random_chromosomes_small_geometry(seed, max_gap):
    n = 20000
    pos, tlen = R.spike_chromosome(seed)
    want = both(pos, tlen, n, (2, 5, 20, max_gap, 1), *real_tables(pos, tlen, n, 2, 5, 20, 2))
    assert len(want[0]) >= 3


# ---- chromosome ends ------------------------------------------------------------------------------------------------------------------
def test_chromosome_ends():
    n = 2000
    # insertions at base 0 and at n - 1 (as l, and as the r of records whose l = -26 is dropped); a record with r >= n, one with l < 0
    pos = _i64([-30, -30, -30, -10, -4, -4, -4, 1000, n - 5, n - 5, n - 5])
    tlen = _i64([n + 34, n + 34, n + 34, 50, 5000, 5000, 5000, 100, 100, 100, 9])
    ins = np.sort(R.insertions(pos, tlen, n))
    assert ins[:3].tolist() == [0, 0, 0] and ins[-5:].tolist() == [n - 1] * 5 and len(ins) == 2 * len(pos) - 3 - 1 - 3 - 2
    want = both(pos, tlen, n, (1, 1, 1, 0, 1), 3, OPEN, OPEN)
    assert want[0].tolist() == [0, n - 2] and want[1].tolist() == [2, n]
    want = both(pos, tlen, n, (75, 500, 5000, 0, 1), 1, OPEN, OPEN)          # windows far wider than what is left of the chromosome
    assert want[0][0] == 0 and want[1][-1] == n


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------------------
def test_degenerate_inputs():
    n = 2000
    e = _i64([])
    want = both(e, e, n, DEFAULT, 1, OPEN, OPEN)
    assert want[6:] == (0, 0) and all(len(a) == 0 for a in want[:6])
    pos, tlen = at(np.arange(0, n, 3), n)
    want = both(pos, tlen, n, (2, 5, 20, 0, 1), 5, OPEN, OPEN)               # p is 2 at the most: nothing significant
    assert want[6:] == (0, 0) and len(want[0]) == 0
    want = both(pos, tlen, n, (2, 5, 20, 0, 1), 1, OPEN, OPEN, with_kernel_ms=False)
    assert want[0].tolist() == [0] and want[1].tolist() == [n] and want[7] == n          # every base: one region [first, last + 1)
    closed = np.full(64, -1, np.int32)                                        # a negative entry admits nothing
    assert both(pos, tlen, n, (2, 5, 20, 0, 1), 1, closed, OPEN)[7] == 0 and both(pos, tlen, n, (2, 5, 20, 0, 1), 1, OPEN, closed)[7] == 0


# ---- the gap, length and summit rules, by construction ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap", [0, 1, 7, 75])
def test_gap_rule(max_gap):
    n = 3000
    # runs 999..1001 and (1002 + max_gap)..: exactly max_gap bases between them; then a pair one base further apart
    pos, tlen = at([1000, 1003 + max_gap, 2000, 2004 + max_gap], n)
    want = both(pos, tlen, n, (1, 1, 1, max_gap, 1), 1, OPEN, OPEN)
    assert want[0].tolist() == [999, 1999, 2003 + max_gap] and want[1].tolist() == [1005 + max_gap, 2002, 2006 + max_gap]


def test_length_rule():
    n = 3000
    pos, tlen = at([1000, 2000, 2003], n)                # a run of three bases and one of six
    assert both(pos, tlen, n, (1, 1, 1, 0, 3), 1, OPEN, OPEN)[0].tolist() == [999, 1999]
    want = both(pos, tlen, n, (1, 1, 1, 0, 4), 1, OPEN, OPEN)
    assert want[0].tolist() == [1999] and want[6] == 2
    assert both(pos, tlen, n, (1, 1, 1, 0, 6), 1, OPEN, OPEN)[0].tolist() == [1999]
    assert both(pos, tlen, n, (1, 1, 1, 0, 7), 1, OPEN, OPEN)[0].tolist() == []


@pytest.mark.parametrize("shift", [0, 1])
def test_plateau_summit(shift):
    n = 3000
    # p = 2 on 999..1001 and on (1019 + shift)..(1021 + shift), 1 around the single insertions that hold the region together
    pos, tlen = at([1000, 1000, 1004, 1008, 1012, 1016, 1020 + shift, 1020 + shift], n)
    want = both(pos, tlen, n, (1, 1, 1, 2, 1), 1, OPEN, OPEN)
    a, b = 999, 1021 + shift
    assert want[0].tolist() == [999] and want[1].tolist() == [b + 1] and want[2].tolist() == [(a + b) // 2] == [1010]


def test_table_cap():
    n = 5000
    pos, tlen = at([2000] * 100 + [3000] * 10, n)
    ts, tl = np.full(64, 5, np.int32), np.full(64, 5, np.int32)
    ts[63] = tl[63] = 1000                               # only the last entry admits a local count of 100
    want = both(pos, tlen, n, (2, 5, 20, 0, 1), 3, ts, tl)
    assert want[0].tolist() == [1998] and want[3].tolist() == [100]           # p = 100 > 63 reads entry 63; p = 10 reads entry 10
    ts[63] = 99
    assert len(both(pos, tlen, n, (2, 5, 20, 0, 1), 3, ts, tl)[0]) == 0


def test_table_edge():
    n = 5000
    x, k, j = 2000, 7, 4
    pos, tlen = at([x] * k + [x + 3] * j, n)             # p(x) = k, s(x) = s(x + 1) = k + j with small = 3; s(x - 1) = k
    ts = np.zeros(64, np.int32)
    ts[k] = k + j
    want = both(pos, tlen, n, (1, 3, 3, 0, 1), k, ts, OPEN)
    assert want[0].tolist() == [x - 1] and want[1].tolist() == [x + 2] and want[4].tolist() == [k + j]
    ts[k] = k + j - 1                                    # one above the entry
    want = both(pos, tlen, n, (1, 3, 3, 0, 1), k, ts, OPEN)
    assert want[0].tolist() == [x - 1] and want[1].tolist() == [x]
    tl = np.zeros(64, np.int32)                          # the same edge in the large table
    tl[k] = k + j
    assert both(pos, tlen, n, (1, 1, 3, 0, 1), k, OPEN, tl)[1].tolist() == [x + 2]
    tl[k] = k + j - 1
    assert both(pos, tlen, n, (1, 1, 3, 0, 1), k, OPEN, tl)[1].tolist() == [x]


# ---- segments ---------------------------------------------------------------------------------------------------------------------
CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from nucleoatac_amd import get_context
d = np.load(sys.argv[1])
out = {}
for k in range(int(d["n_cases"])):
    g = [int(v) for v in d["geom_%%d" %% k]]
    res = get_context().enriched_regions(d["pos_%%d" %% k], d["tlen_%%d" %% k], g[0], d["ts_%%d" %% k], d["tl_%%d" %% k], g[1], *g[2:], with_counts=True)
    for j, a in enumerate(res):
        out["r_%%d_%%d" %% (k, j)] = np.asarray(a)
np.savez(sys.argv[2], **out)
""" % ROOT


def _segment_cases():
    cases = []
    n = 52999
    pos, tlen = R.hotspot_chromosome(1, n=n, n_uniform=2000)
    cases.append((pos, tlen, n, DEFAULT) + real_tables(pos, tlen, n, 75, 500, 5000, 5))
    n = 20000
    pos, tlen = R.spike_chromosome(2)
    cases.append((pos, tlen, n, (2, 5, 20, 3, 1)) + real_tables(pos, tlen, n, 2, 5, 20, 2))
    # borders at the multiples of 1000: inside a region (998..1003), inside a gap of exactly max_gap = 5 (runs 1996..1998 and
    # 2004..2006), between a region's two maximal stretches (2 on 2996..2998 and on 3002..3004, joined over 2999..3001 by the gap rule),
    # right behind a region's last base (3999) and on a region's first base (5000)
    n = 7000
    pos, tlen = at([999, 1002, 1997, 2005, 2997, 2997, 3003, 3003, 3998, 5001, 6999], n)
    cases.append((pos, tlen, n, (1, 1, 1, 5, 1), 1, OPEN, OPEN))
    pos, tlen = at(np.arange(0, n, 2), n)                # one region over every segment
    cases.append((pos, tlen, n, (1, 1, 1, 0, 1), 1, OPEN, OPEN))
    cases += R.long_piece_cases()[0]                     # (4, 5, 6) pieces above SHORT_MAX in several segments of 3000
    return cases


@pytest.fixture(scope="module")
def segment_cases(tmp_path_factory):
    cases = _segment_cases()
    want = [R.enriched_regions(p, t, n, g[0], g[1], g[2], g[3], g[4], mp, ts, tl, counts=True) for p, t, n, g, mp, ts, tl in cases]
    arrs = dict(n_cases=len(cases))
    for k, (p, t, n, g, mp, ts, tl) in enumerate(cases):
        arrs.update({"pos_%d" % k: p, "tlen_%d" % k: t, "ts_%d" % k: ts, "tl_%d" % k: tl, "geom_%d" % k: _i64([n, mp] + list(g))})
    path = str(tmp_path_factory.mktemp("segments") / "cases.npz")
    np.savez(path, **arrs)
    return cases, want, path


def test_segment_cases_at_the_default_segment(segment_cases):
    cases, want, _ = segment_cases
    for (p, t, n, g, mp, ts, tl), w in zip(cases, want):
        assert_same(_ctx().enriched_regions(p, t, n, ts, tl, mp, *g, with_counts=True), w)
    assert want[2][0].tolist() == [998, 1996, 2996, 3997, 5000, 6998] and want[2][1].tolist() == [1004, 2007, 3005, 4000, 5003, 7000]
    assert want[2][2].tolist()[2] == 3000 and want[3][0].tolist() == [0] and want[3][1].tolist() == [7000]
    assert len(want[0][0]) >= 3 and len(want[1][0]) >= 3


@pytest.mark.parametrize("segment", [1000, 7001, 64, 3000, 2048])
def test_segment_size_changes_nothing(segment_cases, segment, tmp_path):
    """NATAC_PEAKS_SEGMENT in a fresh child process: 1000 and 7001 are below 2 * large = 10000 of the default geometry, 1000 puts the
    borders where the third case wants them, and 64 is below every halo there is.  3000 cuts the last three cases into the long and
    short pieces they are made for; at 2048 = SHORT_MAX no piece is long"""
    cases, want, path = segment_cases
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, NATAC_PEAKS_SEGMENT=str(segment))
    subprocess.run([sys.executable, "-c", CHILD, path, out], check=True, env=env, cwd=ROOT, timeout=120)
    d = np.load(out)
    for k, w in enumerate(want):
        assert_same([d["r_%d_%d" % (k, j)] if j < 6 else int(d["r_%d_%d" % (k, j)]) for j in range(8)], w)


# ---- many regions, long regions ----------------------------------------------------------------------------------------------------------
def test_many_regions_against_any_first_capacity():
    n = 2_000_000
    pos, tlen = at(np.arange(50, n, 100), n)             # 20,000 runs of three bases
    h, S, L, gap, length = geom = (1, 1, 1, 0, 1)
    want = R.enriched_regions(pos, tlen, n, h, S, L, gap, length, 1, OPEN, OPEN, counts=True)
    assert len(want[0]) == 20000 > FIRST_CAPACITY
    for capacity in (None, 0, 1, 19999, 20000, 50000):
        assert_same(_ctx().enriched_regions(pos, tlen, n, OPEN, OPEN, 1, *geom, capacity=capacity, with_counts=True), want)


def test_long_and_short_regions():
    n = 300_000
    long_run = np.arange(50_000, 170_001, 2)             # one region of 120,003 bases: 59 pieces of a wave's size and more
    xs = np.sort(np.concatenate([np.arange(100, 50_000 - 100, 997), long_run, [60_001, 160_000, 160_000], np.arange(171_000, n, 1499)]))
    pos, tlen = at(xs, n)
    want = both(pos, tlen, n, (1, 1, 1, 0, 1), 1, OPEN, OPEN)
    k = int(np.argmax(want[1] - want[0]))
    assert want[1][k] - want[0][k] == 120_003 > 100_000 > SHORT_MAX and len(want[0]) > 100
    assert want[2][k] == 160_000 and want[3][k] == 3     # p = 4 only at 159,999 and 160,001, far from where the region starts
    xs = np.sort(np.concatenate([long_run, [60_001, 160_000]]))          # two highest stretches, 100 kb apart: first and last of a workgroup
    pos, tlen = at(xs, n)
    want = both(pos, tlen, n, (1, 1, 1, 0, 1), 1, OPEN, OPEN)
    assert want[2].tolist() == [(60_001 + 160_001) // 2] and want[3].tolist() == [2]          # p = 3 at 60,001, 159,999 and 160,001


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
SENTINEL = -77


def _raw(pos, tlen, chrom_len=5000, geom=(2, 5, 20, 0, 1), min_pile=1, n_table=64, ts=OPEN, tl=OPEN, nf=None):
    from nucleoatac_amd import _lib as L
    lib = L.load()
    out = [np.full(8, SENTINEL, np.int64) for _ in range(3)] + [np.full(8, SENTINEL, np.int32) for _ in range(3)]
    n, found, nsig, ms = C.c_int64(SENTINEL), C.c_int64(SENTINEL), C.c_int64(SENTINEL), C.c_double(SENTINEL)
    rc = lib.natac_enriched_regions(_ctx()._h, len(pos) if nf is None else nf, _vp(pos), _vp(tlen), chrom_len, *geom, min_pile, n_table,
                                    _vp(ts), _vp(tl), C.byref(n), 8, *[_vp(o) for o in out], C.byref(found), C.byref(nsig), C.byref(ms))
    untouched = all(np.all(o == SENTINEL) for o in out) and n.value == found.value == nsig.value == SENTINEL and ms.value == SENTINEL
    return rc, untouched, out, n.value


def test_refusals_leave_the_outputs_as_they_were():
    pos, tlen = at([1000] * 5, 5000)
    rc, untouched, out, n = _raw(pos, tlen)
    assert rc == 0 and not untouched and n == 1 and out[0][0] == 998 and out[0][1] == SENTINEL
    bad = [dict(pos=_i64([996, 995, 996, 996, 996])),                        # unsorted pos
           dict(geom=(6, 5, 20, 0, 1)),                                       # small < half_width
           dict(geom=(0, 5, 20, 0, 1)), dict(geom=(2, 5, 4, 0, 1)), dict(geom=(2, 5, 50001, 0, 1)),
           dict(geom=(2, 5, 20, -1, 1)), dict(geom=(2, 5, 20, 0, 0)), dict(min_pile=0),
           dict(chrom_len=0), dict(chrom_len=1 << 31), dict(ts=None), dict(tl=None), dict(n_table=1), dict(nf=1 << 30), dict(nf=-1)]
    for kw in bad:
        rc, untouched, _, _ = _raw(kw.pop("pos", pos), tlen, **kw)
        assert rc == -1 and untouched, kw                       # NATAC_E_ARG
    with pytest.raises(ValueError):
        _ctx().enriched_regions(pos, tlen[:3], 5000, OPEN, OPEN, 1)
    with pytest.raises(ValueError):
        _ctx().enriched_regions(pos, tlen, 5000, OPEN, OPEN[:5], 1)


def test_more_regions_than_room_fills_nothing():
    pos, tlen = at(np.arange(100, 1100, 100), 5000)      # ten regions, room for eight
    rc, _, out, n = _raw(pos, tlen, geom=(1, 1, 1, 0, 1))
    assert rc == 0 and n == 10 and all(np.all(o == SENTINEL) for o in out)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def test_pyatac_peaks_then_counts(tmp_path):
    """`pyatac peaks` on a small BGZF fragment file, then `pyatac counts` over its fixed-width windows.  A window [summit - 100, summit +
    100) holds the pileup window [summit - 75, summit + 75] of its summit, so at least p(summit) >= min_pileup insertions; a fragment
    has two insertions, and `counts` (ATAC offsets: the same l and r, size filter wide open) counts a fragment once if either lies in
    the window: every window counts at least min_pileup / 2 fragments."""
    import gzip
    from nucleoatac_amd.pyatac.cli import main
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    lines = []
    for c, seed in (("chr1", 5), ("chr2", 6)):
        pos, tlen = R.hotspot_chromosome(seed, n=40000, n_uniform=2000, flush=False)
        keep = pos + 4 >= 0
        lines += ["%s\t%d\t%d\tAAAC-1\t1\n" % (c, s, e) for s, e in zip((pos + 4)[keep].tolist(), (pos + tlen - 4)[keep].tolist())]
    path = str(tmp_path / "tiny.fragments.tsv.gz")
    open(path, "wb").write(bgzf_bytes("".join(lines).encode()))
    base = str(tmp_path / "tiny")
    assert main(["peaks", "--bam", path, "--out", base, "--fixed_width", "200"]) == 0
    st = FragmentStore.open(path)
    from nucleoatac_amd.pyatac import get_peaks as G
    res = G.call_peaks(st, st.chrom_sizes(), regions=lambda *a: R.enriched_regions(*a, counts=True))      # the same files from the restatement
    sel = G.fixed_width_set(res["chrom"], res["summit"], res["mlog10p"], res["pileup"], st.lengths, 200)
    for suffix, text in G.texts(res, st.references, "tiny", sel + (200,)).items():
        assert open(base + suffix, "rb").read() == text, suffix
    assert res["regions_kept"] >= 6
    fixed = [l.split("\t") for l in open(base + ".peaks.fixed.bed").read().splitlines()]
    assert len(fixed) >= 6
    assert main(["counts", "--bam", path, "--bed", base + ".peaks.fixed.bed", "--out", base, "--lower", "0", "--upper", "100000"]) == 0
    counts = [int(x) for x in gzip.open(base + ".counts.txt.gz").read().split()]
    assert len(counts) == len(fixed) and min(counts) * 2 >= res["min_pileup"] >= 1
