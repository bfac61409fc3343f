"""CPU: the host part of `pyatac markers` (nucleoatac_amd/pyatac/get_markers.py) -- the statistics, Benjamini-Hochberg, the files and every
refusal -- with the restatement of tests/markers_ref.py standing in for Context.group_rank_sums (the device call is
tests/test_gpu_markers.py); that restatement itself against brute-force exact midranks and scipy's Mann-Whitney test; and the launch plan
of the device call, which needs no GPU."""
import os
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import markers_ref as R
from nucleoatac_amd.pyatac import get_markers as GM


def _args(argv):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    return pyatac_parser().parse_args(["markers"] + argv)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def _brute(case, p):
    """rank2 per group and ties of row p from the midranks of all N values, zeros included, by counting"""
    N, G = case["N"], case["G"]
    v = [Fraction(0)] * N
    for e in range(case["indptr"][p], case["indptr"][p + 1]):
        v[case["indices"][e]] = Fraction(int(case["data"][e]), int(case["depth"][case["indices"][e]]))
    size = Counter(v)
    rank2 = [0] * G
    for c in range(N):
        rank2[case["group"][c]] += 2 * sum(n for x, n in size.items() if x < v[c]) + size[v[c]] + 1
    return rank2, sum(t ** 3 - t for t in size.values())


@pytest.mark.parametrize("N,G", [(2, 1), (2, 2), (63, 5), (65, 2), (200, 255)])
def test_restatement_against_brute_force_midranks(N, G):
    case = R.make_case(11 + N + G, N, G, m=40)
    det, tot, rank2, ties = R.rank_sums(case["indptr"], case["indices"], case["data"], N, case["depth"], case["group"], G)
    assert det.dtype == np.int32 and tot.dtype == rank2.dtype == ties.dtype == np.int64
    for p in range(40):
        want, t = _brute(case, p)
        assert rank2[p].tolist() == want and int(ties[p]) == t, p
        cells = case["indices"][case["indptr"][p]:case["indptr"][p + 1]]
        a = case["data"][case["indptr"][p]:case["indptr"][p + 1]]
        for g in range(G):
            assert det[p, g] == int((case["group"][cells] == g).sum()) and tot[p, g] == int(a[case["group"][cells] == g].astype(np.int64).sum())
    # the rows the cases promise
    L = np.diff(case["indptr"])
    assert L[0] == 0 and L[1] == 1 and L[2] == N
    n_g = np.bincount(case["group"], minlength=G)
    assert rank2[0].tolist() == (n_g * (N + 1)).tolist() and ties[0] == N ** 3 - N                     # the empty row
    k = int(L[3])
    assert ties[3] == (N - k) ** 3 - (N - k) + k ** 3 - k                                             # one tie group of the row's k entries
    (a0, d0), (a1, d1) = R.COLLIDING
    assert a0 / d0 == a1 / d1 and a0 * d1 != a1 * d0                                                   # equal in fp64, different exactly
    assert ties[5] == (N - 2) ** 3 - (N - 2)                                                           # ... so row 5 has no tie among its entries
    assert case["data"].max() == R.BIG and case["depth"].max() >= R.BIG - 1


def test_statistics_against_scipy_mannwhitneyu():
    """U equal and p within rtol 1e-10 of scipy's asymptotic test with tie and continuity correction, for the restatement and for the
    command's vectorised form; the inputs are small integers, so the float quotients tie exactly where the rationals do"""
    from scipy.stats import mannwhitneyu
    rng = np.random.default_rng(8)
    N, G, m = 37, 3, 120
    depth = rng.integers(1, 50, N).astype(np.int64)
    group = rng.integers(0, G, N).astype(np.int32)
    X = rng.integers(1, 4, (m, N)) * (rng.random((m, N)) < rng.uniform(0.05, 0.9, m)[:, None])
    X[0] = 0
    X[1] = depth                                                       # every value 1: the variance is 0
    ip, ix, da = R.csr_of(X)
    ints = R.rank_sums(ip, ix, da, N, depth, group, G)
    ref = R.statistics(*ints, depth, group, G, min_cells=1)
    own = GM.statistics(*ints, depth, group, G, min_cells=1)
    assert not ref["tested"][0] and ref["tested"][1:].all() and np.array_equal(ref["tested"], own["tested"])
    assert np.isnan(ref["z"][1]).all() and np.isnan(own["p"][1]).all() and np.isnan(own["z"][0]).all()
    worst = 0.0
    for w in range(2, m):
        v = X[w] / depth
        for g in range(G):
            sel = group == g
            want = mannwhitneyu(v[sel], v[~sel], alternative="two-sided", method="asymptotic", use_continuity=True)
            U = ints[2][w, g] / 2.0 - sel.sum() * (sel.sum() + 1) / 2.0
            assert want.statistic == U
            for st in (ref, own):
                assert st["auc"][w, g] == U / (sel.sum() * (~sel).sum())
                if np.isnan(want.pvalue):
                    assert np.isnan(st["p"][w, g])
                    continue
                worst = max(worst, abs(st["p"][w, g] - want.pvalue) / want.pvalue)
    print("largest relative difference of p from scipy's: %.3g" % worst)
    assert worst <= 1e-10
    for k in ("z", "p", "auc", "pct_in", "pct_rest", "log2fc"):
        np.testing.assert_allclose(own[k], ref[k], rtol=1e-13, atol=0, equal_nan=True)
    # by hand: window w, group g
    w, g = 5, 1
    sel = group == g
    assert ref["pct_in"][w, g] == (X[w][sel] > 0).sum() / sel.sum() and ref["pct_rest"][w, g] == (X[w][~sel] > 0).sum() / (~sel).sum()
    fc = ((X[w][sel].sum() + 1) / depth[sel].sum()) / ((X[w][~sel].sum() + 1) / depth[~sel].sum())
    assert abs(ref["log2fc"][w, g] - np.log2(fc)) <= 1e-14 * max(1.0, abs(np.log2(fc)))


def test_min_cells_and_dead_groups():
    depth = np.array([3, 4, 5, 6], np.int64)
    group = np.array([0, 0, 0, 0], np.int32)
    X = np.array([[1, 1, 0, 0], [1, 1, 1, 0]])
    ints = R.rank_sums(*R.csr_of(X), 4, depth, group, 2)
    for st in (R.statistics(*ints, depth, group, 2, min_cells=3), GM.statistics(*ints, depth, group, 2, min_cells=3)):
        assert st["tested"].tolist() == [False, True]
        for k in ("z", "p", "auc", "pct_in", "pct_rest", "log2fc"):
            assert np.isnan(st[k]).all()                               # group 0 holds every cell, group 1 none


def test_benjamini_hochberg_against_scipy():
    from scipy.stats import false_discovery_control
    rng = np.random.default_rng(4)
    for n in (1, 2, 17, 400):
        p = rng.random(n) ** 3
        p[rng.integers(0, n, n // 5)] = p[0]                           # ties
        if n > 2:
            p[[1, n - 1]] = np.nan
        fin = np.isfinite(p)
        want = false_discovery_control(p[fin], method="bh")
        for q in (R.bh(p), GM.benjamini_hochberg(p)):
            assert np.isnan(q[~fin]).all()
            np.testing.assert_allclose(q[fin], want, rtol=1e-14, atol=0)
    assert GM.benjamini_hochberg(np.array([0.04, 0.01, 0.04, 0.5])).tolist() == [0.04 * 4 / 3, 0.04, 0.04 * 4 / 3, 0.5]
    assert np.isnan(GM.benjamini_hochberg(np.array([np.nan, np.nan]))).all()


# ---- the command -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("markers_host")
    X, barcodes, grp = R.planted_case(seed=3, n_groups=3, per_group=30, n_windows=150, planted=20)
    X[:, 7] = 0                                                        # a listed cell without a count
    listed = [i for i in range(len(barcodes)) if i % 10 != 9]          # every tenth cell is not in the table
    groups = str(d / "groups.tsv")
    with open(groups, "w") as f:
        f.write("barcode\tcluster\n")
        f.write("".join("%s\tc%d\n" % (barcodes[i].decode(), grp[i] + 1) for i in listed) + "ABSENT1\tc4\nABSENT2\tc2\n")
    return dict(dir=d, X=X, barcodes=barcodes, grp=grp, listed=listed, groups=groups)


def _run(world, base, fmt, extra=()):
    cx = R.write_counts(base, world["X"], world["barcodes"], fmt)
    return GM.get_markers(_args(["--counts", cx, "--groups", world["groups"], "--header", "--out", base] + list(extra)), rank=R.device_stand_in)


def test_files_of_both_forms_and_the_reference(world):
    d = world["dir"]
    outs = {}
    for fmt in ("npz", "mtx"):
        paths = _run(world, str(d / ("run_" + fmt)), fmt, ["--min_cells", "5"])
        assert [os.path.basename(p) for p in paths] == ["run_%s.markers%s" % (fmt, s) for s in (".npz", ".tsv", ".txt", ".c1.bed", ".c2.bed", ".c3.bed", ".c4.bed")]
        outs[fmt] = [open(p, "rb").read() for p in paths]
    assert outs["npz"] == outs["mtx"]
    z = np.load(str(d / "run_npz.markers.npz"))
    # the kept cells: listed and with a count
    keep = np.array([i in set(world["listed"]) and i != 7 for i in range(len(world["barcodes"]))])
    Xk, grp = world["X"][:, keep], world["grp"][keep]
    depth = Xk.sum(axis=0)
    assert z["groups"].tolist() == [b"c1", b"c2", b"c3", b"c4"] and z["n_cells"].tolist() == np.bincount(grp, minlength=4).tolist()
    ints = R.rank_sums(*R.csr_of(Xk), Xk.shape[1], depth, grp, 4)
    for k, a in zip(("detected", "total", "rank2", "ties"), ints):
        assert np.array_equal(z[k], a) and z[k].dtype == a.dtype
    st = R.statistics(*ints, depth, grp, 4, min_cells=5)
    assert np.array_equal(z["tested"], st["tested"]) and 0 < st["tested"].sum() < 150
    for k in ("z", "p", "log2fc", "auc"):
        np.testing.assert_allclose(z[k], st[k], rtol=1e-13, atol=0, equal_nan=True)
    q = np.stack([R.bh(st["p"][:, g]) for g in range(4)], axis=1)
    np.testing.assert_allclose(z["q"], q, rtol=1e-13, atol=0, equal_nan=True)
    assert np.isnan(z["q"][:, 3]).all() and np.isnan(z["z"][~st["tested"]]).all()
    chrom, start, end = R.regions(150)
    assert z["region_chrom"].tolist() == chrom and np.array_equal(z["region_start"], start) and np.array_equal(z["region_end"], end)
    # the table: the planted windows, per group by q, then auc descending, then index
    lines = outs["npz"][1].decode().split("\n")
    assert lines[0] == "group\tchrom\tstart\tend\tlog2fc\tauc\tpct_in\tpct_rest\tz\tp\tq" and lines[-1] == ""
    rows = [ln.split("\t") for ln in lines[1:-1]]
    where = {(c, int(s)): i for i, (c, s) in enumerate(zip(chrom, start))}
    for g in range(3):
        mine = [r for r in rows if r[0] == "c%d" % (g + 1)]
        wins = [where[r[1], int(r[2])] for r in mine]
        with np.errstate(invalid="ignore"):
            want = np.flatnonzero((q[:, g] <= 0.05) & (st["log2fc"][:, g] >= 0.5) & (st["auc"][:, g] > 0.5))
        want = sorted(want.tolist(), key=lambda w: (q[w, g], -st["auc"][w, g], w))
        planted = set(range(g * 20, g * 20 + 20))                      # at an FDR of 0.05 a window or two beside them is in order
        assert wins == want and len(planted & set(wins)) >= 15 and len(set(wins) - planted) <= 2
        for r, w in zip(mine, wins):
            assert r[3] == str(end[w]) and r[4:9] == ["%.4f" % v for v in (st["log2fc"][w, g], st["auc"][w, g], st["pct_in"][w, g],
                                                                             st["pct_rest"][w, g], st["z"][w, g])]
            assert r[9:] == ["%.3e" % st["p"][w, g], "%.3e" % q[w, g]]
        bed = outs["npz"][3 + g].decode().split("\n")
        assert bed[-1] == "" and len(bed) - 1 == len(wins)
        for i, (ln, w) in enumerate(zip(bed, wins), 1):
            assert ln == "%s\t%d\t%d\tc%d_marker_%d\t%d" % (chrom[w], start[w], end[w], g + 1, i, min(1000, int(-10 * np.log10(q[w, g]))))
    assert not [r for r in rows if r[0] == "c4"] and outs["npz"][6] == b""                            # a group without a cell: NA, an empty BED
    n_listed = len(world["listed"]) + 2
    txt = outs["npz"][2].decode()
    assert txt.startswith("cells_listed\t%d\ncells_in_matrix\t90\ncells_kept\t%d\ncells_dropped\t%d\nwindows\t150\nwindows_tested\t%d\n"
                          "group\tcells\ttested\tmarkers\n" % (n_listed, keep.sum(), n_listed - keep.sum(), st["tested"].sum()))
    assert txt.endswith("c4\t0\t0\t0\n") and "c1\t%d\t%d\t%d\n" % ((grp == 0).sum(), st["tested"].sum(), len([r for r in rows if r[0] == "c1"])) in txt


def test_top_cuts_the_bed_files_only(world):
    d = world["dir"]
    full = _run(world, str(d / "full"), "npz", ["--min_cells", "5"])
    cut = _run(world, str(d / "cut"), "npz", ["--min_cells", "5", "--top", "3"])
    for a, b in zip(full[:3], cut[:3]):
        assert open(a, "rb").read() == open(b, "rb").read()
    for a, b in zip(full[3:6], cut[3:6]):
        want = open(a).read().split("\n")[:3]
        assert open(b).read() == "".join(ln + "\n" for ln in want) and len(want) == 3
    assert open(cut[6]).read() == ""
    # the BED files are what the --bed readers take: chrom, start, end and two more columns
    from nucleoatac_amd.pyatac.get_deviations import _regions_bed
    chrom, start, end = _regions_bed(cut[3])
    assert len(chrom) == 3 and (end - start == 40).all()


def test_refusals(world, capsys):
    from nucleoatac_amd.pyatac.cli import pyatac_main
    d = world["dir"]
    base = str(d / "bad")
    cx = R.write_counts(base, world["X"], world["barcodes"], "npz")
    ok = ["--counts", cx, "--groups", world["groups"], "--header", "--out", base]

    def refused(argv, text):
        assert pyatac_main(_args(argv)) == 1
        cap = capsys.readouterr()
        assert cap.err.startswith("pyatac markers: ") and cap.err.endswith("\n") and cap.err.count("\n") == 1 and text in cap.err
        assert not [f for f in os.listdir(str(d)) if ".markers" in f and f.startswith("bad")]

    refused(ok + ["--min_cells", "0"], "--min_cells must be at least 1 (got 0)")
    refused(ok + ["--fdr", "0"], "--fdr must be in (0, 1]")
    refused(ok + ["--fdr", "1.5"], "--fdr must be in (0, 1]")
    refused(ok + ["--min_log2fc", "nan"], "--min_log2fc must be finite")
    refused(ok + ["--top", "0"], "--top must be at least 1 (got 0)")
    refused(["--counts", base + ".nope.npz"] + ok[2:], "bad.nope.npz: no such file")
    refused(ok[:2] + ["--groups", str(d / "nope.tsv")] + ok[4:], "nope.tsv: no such file")
    # a matrix without its regions, in either form
    refused(["--counts", R.write_counts(str(d / "bad2"), world["X"], world["barcodes"], "npz", with_regions=False)] + ok[2:], "the file carries no regions")
    refused(["--counts", R.write_counts(str(d / "bad3"), world["X"], world["barcodes"], "mtx", with_regions=False)] + ok[2:], "bad3.cellcounts.regions.bed: no such file")
    # fewer than two groups with a kept cell: one group, and two of which one has only absent or empty cells
    one = str(d / "one.tsv")
    with open(one, "w") as f:
        f.write("".join("%s\tonly\n" % b.decode() for b in world["barcodes"][:20]))
    refused(ok[:2] + ["--groups", one, "--out", base], "fewer than two groups have a cell with a count")
    with open(one, "w") as f:
        f.write("".join("%s\ta\n" % b.decode() for b in world["barcodes"][10:30]) + "ABSENT\tb\n%s\tb\n" % world["barcodes"][7].decode())
    refused(ok[:2] + ["--groups", one, "--out", base], "fewer than two groups have a cell with a count")
    with open(one, "w") as f:
        f.write("%s\ta\n%s\tb\n" % (world["barcodes"][0].decode(), world["barcodes"][0].decode()))
    refused(ok[:2] + ["--groups", one, "--out", base], "is in group b here and in group a on line 1")
    # a cell of 2^31 counts (the files hold int32 counts, so the column's sum comes from two windows)
    big = world["X"].copy()
    big[0, 0] = big[1, 0] = 1 << 30
    cx4 = R.write_counts(str(d / "bad4"), big, world["barcodes"], "npz")
    refused(["--counts", cx4] + ok[2:], "counts, 2^31 or more")


# ---- the launch plan -----------------------------------------------------------------------------------------------------------------------
def test_plan_pins_every_arm_and_the_forced_thresholds(monkeypatch):
    from nucleoatac_amd import _lib as L
    from nucleoatac_amd.device import group_rank_sums_plan as plan
    monkeypatch.delenv("NATAC_MARKERS_SHORT_MAX", raising=False)
    monkeypatch.delenv("NATAC_MARKERS_BLOCK_MAX", raising=False)
    ctr = lambda rows, G: (rows * G * 20 + 15) // 16 * 16                  # noqa: E731
    p = plan(100000, 10000, 3100000, 5000, 8)
    assert (p["short_max"], p["block_max"], p["lanes"], p["chunk"]) == (64, 8192, 64, 4096) == (L.MARKERS_SHORT_CAP, L.MARKERS_BLOCK_CAP, 64, 4096)
    assert p["wg"] == dict(short=256, block=256, long=256) and p["grid"] == dict(short=2048, block=2048)
    assert p["lds_bytes"] == dict(short=ctr(4, 8), block=ctr(1, 8) + 16 + 8192 * 9, long=0)             # 5000 entries sort as 8192
    # the lanes of the short arm follow the longest row up to short_max; the block arm's LDS follows it up to block_max
    assert [plan(1000, 2000, 9000, k, 5)["lanes"] for k in (0, 1, 16, 17, 32, 33, 64, 65, 2000)] == [16, 16, 16, 32, 32, 64, 64, 64, 64]
    assert plan(1000, 2000, 9000, 64, 5)["lds_bytes"] == dict(short=ctr(4, 5), block=0, long=0)
    assert [plan(1000, 2000, 9000, k, 5)["lds_bytes"]["block"] - ctr(1, 5) - 16 for k in (65, 128, 129, 2000)] == [128 * 9, 128 * 9, 256 * 9, 2048 * 9]
    q = plan(40, 1 << 20, 9000000, 1 << 20, 255)
    assert q["lds_bytes"] == dict(short=ctr(4, 255), block=ctr(1, 255) + 16 + 8192 * 9, long=max(4096 * 8, ctr(1, 255) + 16))
    assert q["lds_bytes"]["block"] <= 80 * 1024 and q["grid"] == dict(short=10, block=40)
    assert plan(40, 100, 900, 12, 255)["lds_bytes"]["short"] == ctr(16, 255) <= 160 * 1024
    # forced
    monkeypatch.setenv("NATAC_MARKERS_SHORT_MAX", "16")
    monkeypatch.setenv("NATAC_MARKERS_BLOCK_MAX", "64")
    f = plan(300, 200, 9000, 200, 5, n_cu=4)
    assert (f["short_max"], f["block_max"], f["lanes"], f["chunk"]) == (16, 64, 16, 64) and f["grid"] == dict(short=19, block=32)
    assert f["lds_bytes"] == dict(short=ctr(16, 5), block=ctr(1, 5) + 16 + 64 * 9, long=max(64 * 8, ctr(1, 5) + 16))
    monkeypatch.setenv("NATAC_MARKERS_BLOCK_MAX", "5")                     # below short_max: no block arm
    f = plan(300, 200, 9000, 200, 5)
    assert (f["short_max"], f["block_max"], f["chunk"]) == (16, 16, 16) and f["lds_bytes"]["block"] == 0 and f["lds_bytes"]["long"] > 0
    monkeypatch.setenv("NATAC_MARKERS_SHORT_MAX", "64")
    monkeypatch.setenv("NATAC_MARKERS_BLOCK_MAX", "100")
    f = plan(300, 1100, 90000, 1100, 2)
    assert (f["short_max"], f["block_max"], f["lanes"], f["chunk"]) == (64, 100, 64, 64)
    monkeypatch.setenv("NATAC_MARKERS_SHORT_MAX", "65")                    # outside their ranges: not taken
    monkeypatch.setenv("NATAC_MARKERS_BLOCK_MAX", "8193")
    f = plan(300, 1100, 90000, 1100, 2)
    assert (f["short_max"], f["block_max"]) == (64, 8192)
    for bad in ((0, 100, 10, 5, 2), (10, 1, 5, 1, 2), (10, (1 << 20) + 1, 5, 1, 2), (10, 100, 10, 101, 2), (10, 100, 5, 6, 2), (10, 100, 1001, 5, 2),
                (10, 100, 10, 5, 0), (10, 100, 10, 5, 256), (L.MARKERS_MAX_OUT // 2 + 1, 100, 10, 5, 2)):
        with pytest.raises(L.NatacError):
            plan(*bad)
    with pytest.raises(L.NatacError):
        plan(10, 100, 10, 5, 2, n_cu=0)


# ---- the cases of tests/test_gpu_markers_launch_edges.py: sized for the grid before they reach a GPU ------------------------------------------
def _plan_of(case, n_cu):
    from nucleoatac_amd.device import group_rank_sums_plan as plan
    L = np.diff(case["indptr"])
    return plan(len(L), case["N"], int(L.sum()), int(L.max()), case["G"], n_cu=n_cu)


@pytest.mark.parametrize("n_cu", [256, 304])
def test_stride_cases_exceed_the_grid(n_cu, monkeypatch):
    from nucleoatac_amd.device import group_rank_sums_plan as plan
    monkeypatch.delenv("NATAC_MARKERS_BLOCK_MAX", raising=False)
    for short_max, lanes, lead in ((None, 64, 40), (16, 16, None)):
        if short_max is None:
            monkeypatch.delenv("NATAC_MARKERS_SHORT_MAX", raising=False)
        else:
            monkeypatch.setenv("NATAC_MARKERS_SHORT_MAX", str(short_max))
        most = plan(1 << 20, 48, (lead or 8) << 20, lead or 8, 5, n_cu=n_cu)
        assert most["lanes"] == lanes and most["grid"]["short"] == 8 * n_cu
        per_trip = (256 // lanes) * most["grid"]["short"]
        case = R.short_stride_case(40 + lanes, per_trip + 501, per_trip, lead=lead)
        L = np.diff(case["indptr"])
        p = _plan_of(case, n_cu)
        assert p["lanes"] == lanes and p["grid"]["short"] == 8 * n_cu and len(L) > (256 // lanes) * p["grid"]["short"] + 500
        assert L.max() == (lead or 8) <= p["short_max"] and p["lds_bytes"]["block"] == 0               # every row is the short arm's
        second = np.arange(per_trip, len(L))
        assert (L[second - per_trip] == 8).sum() >= 300 and (L[second] == 0).sum() >= 150 and (L[second] == 1).sum() >= 150
        assert all(np.all(np.diff(case["indices"][a:b]) > 0) for a, b in zip(case["indptr"][:400], case["indptr"][1:401]))
    monkeypatch.setenv("NATAC_MARKERS_SHORT_MAX", "4")
    grid = plan(1 << 20, 48, 40 << 20, 40, 5, n_cu=n_cu)["grid"]["block"]
    case, where = R.block_stride_case(77, grid + 301, grid)
    L = np.diff(case["indptr"])
    p = _plan_of(case, n_cu)
    assert grid == 8 * n_cu == p["grid"]["block"] and p["short_max"] == 4 and len(where) > p["grid"]["block"] + 300
    assert (L[where] > 4).all() and L.max() == 40 and (L <= 4).sum() == len(L) - len(where) >= 500
    assert p["lds_bytes"]["block"] == (5 * 20 + 15) // 16 * 16 + 16 + 64 * 9 and p["lds_bytes"]["long"] == 0
    first, second = L[where[:len(where) - grid]], L[where[grid:]]
    assert len(second) == 301 and (first == 40).sum() >= 200 and (second <= 6).sum() >= 200 and (first != second).sum() >= 250


@pytest.mark.parametrize("n_cu", [256, 304])
def test_default_threshold_cases_plan_the_block_arm_past_64_kib(n_cu, monkeypatch):
    monkeypatch.delenv("NATAC_MARKERS_SHORT_MAX", raising=False)
    ctr = lambda G: (G * 20 + 15) // 16 * 16                                # noqa: E731
    for G in (1, 255):
        case = R.border_case(900 + G, G)
        L = np.diff(case["indptr"])
        assert L.tolist() == [0, 1, 64, 65, 4096, 4097, 8192, 8193, 9000, 8500, 8700] and case["N"] == 9000 and case["group"].max() == max(0, G - 2)
        monkeypatch.delenv("NATAC_MARKERS_BLOCK_MAX", raising=False)
        p = _plan_of(case, n_cu)
        assert (p["short_max"], p["block_max"], p["chunk"]) == (64, 8192, 4096)
        assert p["lds_bytes"]["block"] == ctr(G) + 16 + 8192 * 9 > 65536 and p["lds_bytes"]["long"] == max(4096 * 8, ctr(G) + 16)
        monkeypatch.setenv("NATAC_MARKERS_BLOCK_MAX", "4096")
        p = _plan_of(case, n_cu)
        assert (p["block_max"], p["chunk"]) == (4096, 4096) and p["lds_bytes"]["block"] == ctr(G) + 16 + 4096 * 9 < 65536
    monkeypatch.delenv("NATAC_MARKERS_BLOCK_MAX", raising=False)
    case = R.big_case(31)
    L = np.diff(case["indptr"])
    assert case["N"] == 1 << 20 and L.tolist() == [0, 1, 1, 10000, 5000, 40] and case["indices"][case["indptr"][4] - 1] == (1 << 20) - 1
    p = _plan_of(case, n_cu)
    assert p["lds_bytes"]["block"] == ctr(3) + 16 + 8192 * 9 > 65536 and p["lds_bytes"]["long"] == 4096 * 8 and p["grid"] == dict(short=2, block=6)
