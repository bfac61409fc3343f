"""CPU: the host part of `pyatac coaccess` (nucleoatac_amd/pyatac/get_coaccess.py) -- the pair lists, the correlation and its test, the
aggregation, the files and every refusal -- with the restatement of tests/coaccess_ref.py standing in for Context.window_pair_sums (the
device call is tests/test_gpu_coaccess.py); that restatement's two forms against each other; and the launch plan of the device call,
which needs no GPU."""
import os
from decimal import Decimal

import numpy as np
import pytest

import coaccess_ref as R
from nucleoatac_amd.pyatac import get_coaccess as GC


def _args(argv):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    return pyatac_parser().parse_args(["coaccess"] + argv)


# ---- the pair lists ------------------------------------------------------------------------------------------------------------------------
def _same_lists(chrom, start, end, tested, d):
    o, h = GC.pair_lists(chrom, start, end, tested, d)
    ro, rh = R.pair_lists(chrom, start, end, tested, d)
    assert o.dtype == np.int32 and h.dtype == np.int64
    assert o.tolist() == ro.tolist() and h.tolist() == rh.tolist(), d
    return o, h


def test_pair_lists_against_the_double_loop():
    rng = np.random.default_rng(3)
    n = 120
    chrom = [("chr2", "chr10", "chr1")[i] for i in rng.integers(0, 3, n)]            # first appearance, not name order
    start = rng.integers(0, 40, n) * 500                                              # many ties in centre
    end = start + rng.choice([200, 201, 400], n)
    tested = rng.random(n) < 0.8
    for d in (0, 1, 499, 500, 3000, 10 ** 8):
        o, h = _same_lists(chrom, start, end, tested, d)
        assert sorted(o.tolist()) == np.flatnonzero(tested).tolist()                  # untested windows are skipped
    # max_distance 0 pairs only equal centres
    o, h = _same_lists(chrom, start, end, tested, 0)
    a, b = R.pairs_of(o, h)
    centre = (start + end) // 2
    assert len(a) > 0 and (centre[a] == centre[b]).all() and all(chrom[x] == chrom[y] for x, y in zip(a, b))
    # ties in centre: the index decides the rank
    o, h = _same_lists(["c"] * 4, [10, 0, 10, 0], [20, 30, 20, 30], [True] * 4, 5)
    assert o.tolist() == [0, 1, 2, 3] and h.tolist() == [4, 4, 4, 4]
    # one window per chromosome: no pair
    o, h = _same_lists(["a", "b", "c"], [0, 0, 0], [10, 10, 10], [True] * 3, 10 ** 8)
    assert o.tolist() == [0, 1, 2] and h.tolist() == [1, 2, 3]
    o, h = _same_lists(["a", "a"], [0, 5], [10, 15], [False, False], 100)
    assert len(o) == 0 and len(h) == 0
    # the chromosomes go by first appearance; within one by centre
    o, h = _same_lists(["z", "a", "z", "a"], [100, 50, 0, 0], [110, 60, 10, 10], [True] * 4, 1000)
    assert o.tolist() == [2, 0, 3, 1] and h.tolist() == [2, 2, 4, 4]


# ---- the restatement and the statistics ----------------------------------------------------------------------------------------------------
def test_restatement_both_forms_and_the_planted_rows():
    case = R.make_case(7, 60, 40, 8, partners=5, long_rows=(17,))
    args = (case["indptr"], case["indices"], case["data"], 40, case["order"], case["hi"])
    sxy, both = R.pair_sums(*args)
    sxy2, both2 = R.pair_sums_sparse(*args)
    assert sxy.dtype == np.int64 and both.dtype == np.int32 and np.array_equal(sxy, sxy2) and np.array_equal(both, both2)
    a, b = R.pairs_of(case["order"], case["hi"])
    L = np.diff(case["indptr"])
    assert L[0] == 0 and L[1] == 1 and L[2] == 40 and L[7] == 17
    order, hi = case["order"].tolist(), case["hi"].tolist()
    assert order.count(3) == 2 and any(h == i + 1 for i, h in enumerate(hi[:-1])) and hi[-1] == len(order)
    pairs = list(zip(a.tolist(), b.tolist()))
    assert (3, 4) in pairs and (3, 3) in pairs and (5, 6) in pairs and (0, 2) in pairs
    assert both[pairs.index((5, 6))] == 0 and sxy[pairs.index((5, 6))] == 0          # disjoint columns
    assert both[pairs.index((0, 2))] == 0                                            # the empty row
    det, s1, s2 = R.row_sums(case["indptr"], case["data"])
    e = pairs.index((3, 4))
    assert sxy[e] == s2[3] and R.r_of(40, int(sxy[e]), s1[3], s1[4], s2[3], s2[4]) == 1.0          # identical rows
    # no pair crosses the two chromosomes: of the eight planted rows 0, 2, 5, 6 are in the first; the others go by parity
    side = lambda w: (0 if w in (0, 2, 5, 6) else 1) if w < 8 else w % 2          # noqa: E731
    assert all(side(x) == side(y) for x, y in pairs)


def test_r_within_eight_ulps_of_the_decimal_value():
    """|r - r_exact| <= 8 u |r_exact|, u = 2^-53: the three conversions of exact integers (below 2^63) to fp64, the product, the square
    root and the division each err by at most u relative, and the square root halves what its argument carries: under 5 u; 8 leaves
    room.  The counts reach 2^20 over 200 cells, so num and the D's are far past 2^53 and every conversion rounds."""
    rng = np.random.default_rng(12)
    N, m = 200, 40
    X = rng.integers(1, 1 << 20, (m, N)) * (rng.random((m, N)) < 0.6)
    X[1] = X[0]
    X[2] = 7                                                           # constant: D == 0
    ip, ix, da = R.csr_of(X)
    chrom, start = ["c"] * m, np.arange(m) * 100
    res = GC.coaccess(ip, ix, da, N, chrom, start, start + 50, min_cells=1, max_distance=10 ** 8, pairs=R.pair_sums)
    det, s1, s2 = R.row_sums(ip, da)
    assert len(res["r"]) == m * (m - 1) // 2 and res["s1"].tolist() == s1 and res["s2"].tolist() == s2 and res["detected"].tolist() == det
    u, worst = Decimal(2) ** -53, Decimal(0)
    for e, (p, q) in enumerate(zip(res["pair_a"].tolist(), res["pair_b"].tolist())):
        args = (N, int(res["sxy"][e]), s1[p], s1[q], s2[p], s2[q])
        exact = R.r_decimal(*args)
        if exact is None:
            assert 2 in (p, q) and np.isnan(res["r"][e]) and np.isnan(res["p"][e]) and np.isnan(res["q"][e])
            continue
        assert res["r"][e] == R.r_of(*args)
        assert abs(exact) <= 1                                         # Cauchy-Schwarz: the clip only ever removes rounding
        err = abs(Decimal(float(res["r"][e])) - exact)
        worst = max(worst, err / abs(exact))
        assert err <= 8 * u * abs(exact), (p, q)
    print("largest relative error of r: %.3g u" % float(worst / u))
    e = [i for i, (p, q) in enumerate(zip(res["pair_a"], res["pair_b"])) if (p, q) == (0, 1)][0]
    assert res["r"][e] == 1.0 and res["p"][e] == 0.0 and res["q"][e] == 0.0


def test_p_against_scipy_pearsonr():
    from scipy.stats import pearsonr
    rng = np.random.default_rng(5)
    N, m = 25, 12
    X = rng.poisson(rng.uniform(0.3, 3.0, (m, 1)) * rng.uniform(0.5, 2.0, (1, N)))
    X[:, 0] += 1                                                       # no constant row, no empty cell
    ip, ix, da = R.csr_of(X)
    start = np.arange(m) * 100
    res = GC.coaccess(ip, ix, da, N, ["c"] * m, start, start + 50, min_cells=1, max_distance=10 ** 8, pairs=R.pair_sums)
    worst = 0.0
    for e, (p, q) in enumerate(zip(res["pair_a"].tolist(), res["pair_b"].tolist())):
        want = pearsonr(X[p].astype(float), X[q].astype(float))
        assert abs(res["r"][e] - want[0]) <= 1e-12
        worst = max(worst, abs(res["p"][e] - want[1]) / want[1])
        assert res["p"][e] == R.p_of(float(res["r"][e]), N)
    print("largest relative difference of p from scipy's: %.3g" % worst)
    assert worst <= 1e-12
    from nucleoatac_amd.pyatac.get_markers import benjamini_hochberg
    assert np.array_equal(res["q"], benjamini_hochberg(res["p"]))
    with np.errstate(invalid="ignore"):
        want = np.flatnonzero((res["r"] >= 0.5) & (res["q"] <= 0.05))
    assert sorted(res["links"].tolist()) == want.tolist()


# ---- the command -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("coaccess_host")
    X, barcodes, grp = R.command_case()
    listed = [i for i in range(len(barcodes)) if i % 10 != 9]          # every tenth cell is not in the table
    groups = str(d / "groups.tsv")
    with open(groups, "w") as f:
        f.write("barcode\tcluster\n")
        f.write("".join("%s\tc%d\n" % (barcodes[i].decode(), grp[i] + 1) for i in listed) + "ABSENT1\tc9\n")
    return dict(dir=d, X=X, barcodes=barcodes, grp=grp, listed=listed, groups=groups)


def _run(world, base, fmt, extra=()):
    cx = R.write_counts(base, world["X"], world["barcodes"], fmt)
    return GC.get_coaccess(_args(["--counts", cx, "--out", base] + list(extra)), pairs=R.pair_sums)


def _dense_reference(X, chrom, start, end, min_cells, max_distance):
    """tested, pairs and r from a dense matrix of the kept cells, with numpy alone"""
    X = X[:, X.sum(axis=0) > 0]
    tested = (X > 0).sum(axis=1) >= min_cells
    order, hi = R.pair_lists(chrom, start, end, tested, max_distance)
    a, b = R.pairs_of(order, hi)
    N = X.shape[1]
    sxy = (X[a] * X[b]).sum(axis=1)
    both = ((X[a] > 0) & (X[b] > 0)).sum(axis=1)
    s1, s2 = X.sum(axis=1), (X * X).sum(axis=1)
    r = np.array([R.r_of(N, int(sxy[e]), int(s1[p]), int(s1[q]), int(s2[p]), int(s2[q])) for e, (p, q) in enumerate(zip(a, b))])
    return dict(N=N, tested=tested, a=a, b=b, sxy=sxy, both=both, r=r, s1=s1, s2=s2)


def test_files_of_both_forms_and_the_reference(world):
    d = world["dir"]
    outs = {}
    for fmt in ("npz", "mtx"):                                         # one file name in two directories: the links carry it
        os.mkdir(str(d / fmt))
        paths = _run(world, str(d / fmt / "run"), fmt, ["--min_cells", "5", "--max_distance", "9000", "--fdr", "0.2", "--min_cor", "0.3"])
        assert [os.path.basename(p) for p in paths] == ["run.coaccess" + s for s in (".npz", ".bedpe", ".txt")]
        outs[fmt] = [open(p, "rb").read() for p in paths]
    assert outs["npz"] == outs["mtx"]
    z = np.load(str(d / "npz" / "run.coaccess.npz"))
    chrom, start, end = R.regions(len(world["X"]))
    ref = _dense_reference(world["X"], chrom, start, end, 5, 9000)
    assert z["n_cells"] == ref["N"] == 29 and np.array_equal(z["tested"], ref["tested"]) and 0 < ref["tested"].sum()
    assert np.array_equal(z["pair_a"], ref["a"]) and np.array_equal(z["pair_b"], ref["b"]) and len(ref["a"]) > 20
    assert np.array_equal(z["sxy"], ref["sxy"]) and np.array_equal(z["both"], ref["both"]) and z["sxy"].dtype == np.int64 and z["both"].dtype == np.int32
    assert np.array_equal(z["s1"], ref["s1"]) and np.array_equal(z["s2"], ref["s2"]) and np.array_equal(z["detected"], (world["X"] > 0).sum(axis=1))
    assert np.array_equal(z["r"], ref["r"], equal_nan=True)
    assert z["region_chrom"].tolist() == chrom and np.array_equal(z["region_start"], start) and np.array_equal(z["region_end"], end)
    assert all(chrom[p] == chrom[q] for p, q in zip(ref["a"], ref["b"]))
    p = np.array([R.p_of(float(r), ref["N"]) for r in ref["r"]])
    np.testing.assert_allclose(z["p"], p, rtol=1e-13, atol=0, equal_nan=True)
    from nucleoatac_amd.pyatac.get_markers import benjamini_hochberg
    q = benjamini_hochberg(z["p"])
    assert np.array_equal(z["q"], q, equal_nan=True)
    # the links: q, then r descending, then pair index; the member with the smaller start first
    with np.errstate(invalid="ignore"):
        want = np.flatnonzero((z["r"] >= 0.3) & (q <= 0.2))
    want = sorted(want.tolist(), key=lambda e: (q[e], -z["r"][e], e))
    lines = outs["npz"][1].decode().split("\n")
    assert lines[-1] == "" and len(lines) - 1 == len(want) > 0
    for i, (ln, e) in enumerate(zip(lines, want), 1):
        a, b = int(ref["a"][e]), int(ref["b"][e])
        if start[b] < start[a]:
            a, b = b, a
        assert ln == "%s\t%d\t%d\t%s\t%d\t%d\trun_link_%d\t%d\t.\t.\t%.4f\t%d\t%.3e\t%.3e" % (
            chrom[a], start[a], end[a], chrom[b], start[b], end[b], i, min(1000, int(1000 * z["r"][e])), z["r"][e], ref["both"][e], z["p"][e], q[e])
    assert any(start[int(ref["b"][e])] < start[int(ref["a"][e])] for e in range(len(ref["a"])))        # an owner that starts later exists
    txt = outs["npz"][2].decode()
    assert txt == ("cells_listed\t30\ncells_kept\t29\ncells_dropped\t1\nwindows\t40\nwindows_tested\t%d\npairs\t%d\npairs_finite\t%d\nlinks\t%d\n"
                   "N\t29\na_max\t%d\nL_max\t%d\narm\ttable\n" % (ref["tested"].sum(), len(ref["a"]), np.isfinite(ref["r"]).sum(), len(want),
                                                                 world["X"].max(), (world["X"] > 0).sum(axis=1)[ref["tested"]].max()))


def test_aggregate_and_binarize_against_dense_numpy(world):
    d = world["dir"]
    chrom, start, end = R.regions(len(world["X"]))
    X, grp, listed = world["X"], world["grp"], world["listed"]
    for name, extra, binarize in (("agg", [], False), ("aggbin", ["--binarize"], True)):
        paths = _run(world, str(d / name), "npz", ["--aggregate", world["groups"], "--header", "--min_cells", "3", "--max_distance", "9000"] + extra)
        z = np.load(paths[0])
        B = (X > 0).astype(np.int64) if binarize else X
        M = np.stack([B[:, [i for i in listed if grp[i] == g]].sum(axis=1) for g in range(6)] + [np.zeros(len(X), np.int64)], axis=1)   # c9: no cell
        ref = _dense_reference(M, chrom, start, end, 3, 9000)
        assert z["n_cells"] == ref["N"] == 6 and np.array_equal(z["tested"], ref["tested"])
        assert np.array_equal(z["pair_a"], ref["a"]) and np.array_equal(z["sxy"], ref["sxy"]) and np.array_equal(z["both"], ref["both"])
        assert np.array_equal(z["s1"], ref["s1"]) and np.array_equal(z["r"], ref["r"], equal_nan=True) and len(ref["a"]) > 20
        assert open(paths[2]).read().startswith("cells_listed\t7\ncells_kept\t6\ncells_dropped\t1\n")
    paths = _run(world, str(d / "bin"), "npz", ["--binarize", "--min_cells", "5", "--max_distance", "9000"])
    z = np.load(paths[0])
    ref = _dense_reference((X > 0).astype(np.int64), chrom, start, end, 5, 9000)
    assert np.array_equal(z["sxy"], ref["both"]) and np.array_equal(z["both"], ref["both"]) and np.array_equal(z["s2"], ref["s1"])
    assert "a_max\t1\n" in open(paths[2]).read()


def test_no_pair_is_not_an_error(world):
    apart = dict(world, X=world["X"].copy())
    apart["X"][6] = 0                                                  # window 6 shares its centre with window 3
    paths = _run(apart, str(world["dir"] / "nopair"), "npz", ["--min_cells", "5", "--max_distance", "0"])
    z = np.load(paths[0])
    assert len(z["pair_a"]) == 0 == len(z["r"]) and open(paths[1]).read() == ""
    assert "pairs\t0\npairs_finite\t0\nlinks\t0\n" in open(paths[2]).read() and open(paths[2]).read().endswith("arm\tnone\n")


def test_refusals(world, capsys):
    from nucleoatac_amd.pyatac.cli import pyatac_main
    d = world["dir"]
    base = str(d / "bad")
    cx = R.write_counts(base, world["X"], world["barcodes"], "npz")
    ok = ["--counts", cx, "--out", base]

    def refused(argv, text):
        assert pyatac_main(_args(argv)) == 1
        cap = capsys.readouterr()
        assert cap.err.startswith("pyatac coaccess: ") and cap.err.endswith("\n") and cap.err.count("\n") == 1 and text in cap.err, cap.err
        assert not [f for f in os.listdir(str(d)) if ".coaccess" in f and f.startswith("bad")]

    refused(ok + ["--min_cells", "0"], "--min_cells must be at least 1 (got 0)")
    refused(ok + ["--max_distance", "-1"], "--max_distance must be in [0, 100000000]")
    refused(ok + ["--max_distance", "100000001"], "--max_distance must be in [0, 100000000]")
    refused(ok + ["--min_cor", "1.5"], "--min_cor must be in [-1, 1]")
    refused(ok + ["--min_cor", "nan"], "--min_cor must be in [-1, 1]")
    refused(ok + ["--fdr", "0"], "--fdr must be in (0, 1]")
    refused(["--counts", base + ".nope.npz", "--out", base], "bad.nope.npz: no such file")
    refused(ok + ["--aggregate", str(d / "nope.tsv")], "nope.tsv: no such file")
    refused(["--counts", R.write_counts(str(d / "bad2"), world["X"], world["barcodes"], "npz", with_regions=False), "--out", base],
            "the file carries no regions")
    refused(["--counts", R.write_counts(str(d / "bad3"), world["X"], world["barcodes"], "mtx", with_regions=False), "--out", base],
            "bad3.cellcounts.regions.bed: no such file")
    refused(ok + ["--min_cells", "31"], "no window has an entry in 31 cells or more")
    two = world["X"].copy()
    two[:, 2:] = 0
    refused(["--counts", R.write_counts(str(d / "bad4"), two, world["barcodes"], "npz"), "--out", base], "fewer than 3 cells have a count (2)")
    one = str(d / "one.tsv")
    with open(one, "w") as f:
        f.write("".join("%s\t%s\n" % (b.decode(), "ab"[i % 2]) for i, b in enumerate(world["barcodes"])))
    refused(ok + ["--aggregate", one], "fewer than 3 cells have a count (2)")
    # past the bound: N = 29, a_max = 2^29, L_max >= 2^4 -> at least 2^66; the one line says what to do
    big = world["X"].copy()
    big[0, 0] = 1 << 29
    refused(["--counts", R.write_counts(str(d / "bad5"), big, world["barcodes"], "npz"), "--out", base], "use --binarize")


# ---- the launch plan -----------------------------------------------------------------------------------------------------------------------
def test_plan_pins_the_arms_and_the_forced_values(monkeypatch):
    from nucleoatac_amd import _lib as L
    from nucleoatac_amd.device import window_pair_sums_plan as plan
    monkeypatch.delenv("NATAC_COACCESS_TABLE_MAX", raising=False)
    monkeypatch.delenv("NATAC_COACCESS_CHUNK", raising=False)
    assert (L.COACCESS_MAX_PAIRS, L.COACCESS_MAX_CELLS, L.COACCESS_TABLE_CAP, L.COACCESS_CHUNK_CAP) == (1 << 25, 1 << 20, 16384, 8192)
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "natac.h")).read()
    for name in ("MAX_PAIRS", "MAX_CELLS", "TABLE_CAP", "CHUNK_CAP"):
        assert "#define NATAC_COACCESS_%s %d\n" % (name, getattr(L, "COACCESS_" + name)) in h
    p = plan(100000, 10000, 8070000, 100000, 8070000)
    assert p == dict(arm="table", table_max=16384, lanes=64, chunk=8192, wg=256, lds_bytes=40000, grid=2048)
    assert plan(100000, 16384, 8070000, 100000, 8070000)["lds_bytes"] == 65536 and plan(100000, 16384, 8070000, 100000, 8070000)["arm"] == "table"
    q = plan(100000, 16385, 8070000, 100000, 8070000)
    assert (q["arm"], q["lds_bytes"], q["chunk"]) == ("search", 65536, 8192)
    assert plan(300, 63, 900, 100, 500)["lds_bytes"] == 256                      # 252 bytes rounded up to 16
    # lanes: the least of 16 / 32 / 64 that holds ceil(listed entries / k)
    assert [plan(1000, 2000, 90000, 100, e)["lanes"] for e in (0, 1600, 1601, 1700, 3200, 3201, 3300, 6400, 6401, 200000)] == \
        [16, 16, 32, 32, 32, 64, 64, 64, 64, 64]
    # the grid: at most 8 workgroups a CU, at most the listed windows
    assert plan(1000, 2000, 9000, 40, 100, n_cu=4)["grid"] == 32 and plan(1000, 2000, 9000, 7, 100, n_cu=4)["grid"] == 7
    # forced
    monkeypatch.setenv("NATAC_COACCESS_TABLE_MAX", "1")
    monkeypatch.setenv("NATAC_COACCESS_CHUNK", "16")
    f = plan(300, 200, 9000, 300, 9000)
    assert f == dict(arm="search", table_max=1, lanes=32, chunk=16, wg=256, lds_bytes=128, grid=300)
    assert plan(300, 1, 100, 300, 100)["arm"] == "table"
    monkeypatch.setenv("NATAC_COACCESS_TABLE_MAX", "199")
    monkeypatch.setenv("NATAC_COACCESS_CHUNK", "4096")
    f = plan(300, 200, 9000, 300, 9000)
    assert (f["arm"], f["chunk"], f["lds_bytes"]) == ("search", 4096, 32768) and plan(300, 199, 9000, 300, 9000)["arm"] == "table"
    for tm, ch in (("0", "8"), ("16385", "16384"), ("x", "24"), ("-3", "100")):      # outside their rules: not taken
        monkeypatch.setenv("NATAC_COACCESS_TABLE_MAX", tm)
        monkeypatch.setenv("NATAC_COACCESS_CHUNK", ch)
        f = plan(300, 20000, 9000, 300, 9000)
        assert (f["table_max"], f["chunk"], f["arm"]) == (16384, 8192, "search")
    for bad in ((0, 100, 10, 5, 10), (10, 0, 0, 5, 0), (10, (1 << 20) + 1, 5, 1, 2), (10, 100, 1001, 5, 2), (10, 100, 10, 0, 0), (10, 100, 10, 5, 501),
                (10, 100, -1, 5, 2), (1 << 31, 100, 10, 5, 2)):
        with pytest.raises(L.NatacError):
            plan(*bad)
    with pytest.raises(L.NatacError):
        plan(10, 100, 10, 5, 2, n_cu=0)


# ---- the cases of tests/test_gpu_coaccess_launch_edges.py: sized for the grid before they reach a GPU -----------------------------------------
def _plan_of(case, n_cu):
    from nucleoatac_amd.device import window_pair_sums_plan as plan
    L = np.diff(case["indptr"])
    return plan(len(L), case["N"], int(L.sum()), len(case["order"]), int(L[case["order"]].sum()), n_cu=n_cu)


@pytest.mark.parametrize("n_cu", [256, 304])
def test_stride_case_exceeds_the_grid_in_both_arms(n_cu, monkeypatch):
    from nucleoatac_amd.device import window_pair_sums_plan as plan
    monkeypatch.delenv("NATAC_COACCESS_TABLE_MAX", raising=False)
    monkeypatch.delenv("NATAC_COACCESS_CHUNK", raising=False)
    grid = plan(1 << 20, 64, 8 << 20, 1 << 20, 8 << 20, n_cu=n_cu)["grid"]
    assert grid == 8 * n_cu
    case, planted = R.stride_case(17, grid)
    k, L = len(case["order"]), np.diff(case["indptr"])
    has = case["hi"] - np.arange(k) > 1
    p = _plan_of(case, n_cu)
    assert p == dict(arm="table", table_max=16384, lanes=16, chunk=8192, wg=256, lds_bytes=256, grid=grid)
    assert has.sum() > p["grid"] + 500 and (has[grid:] & has[:k - grid]).sum() > 500 and (~has[grid:]).sum() >= 100 and (~has[:grid]).sum() >= 100
    assert [(a, b) for _, a, b in planted] == list(R.STRIDE_PLANTS) and L[[0, 1, 2, 5, 6]].tolist() == [0, 1, 64, 32, 32] and 16 < L[3] < 32
    for i, a, b in planted:
        assert case["order"][i] == a and case["order"][i + grid] == b and has[i] and has[i + grid] and i + grid < k
    assert (case["hi"] > np.arange(k)).all() and case["hi"].max() <= k and case["order"].min() >= 0 and case["order"].max() < len(L)
    monkeypatch.setenv("NATAC_COACCESS_TABLE_MAX", "1")
    assert _plan_of(case, n_cu) == dict(arm="search", table_max=1, lanes=16, chunk=8192, wg=256, lds_bytes=65536, grid=grid)
    monkeypatch.setenv("NATAC_COACCESS_CHUNK", "16")
    assert _plan_of(case, n_cu) == dict(arm="search", table_max=1, lanes=16, chunk=16, wg=256, lds_bytes=128, grid=grid)
    own = L[case["order"]] * has
    assert (own[:grid] > 16).sum() >= 5 and (own[grid:] > 16).sum() >= 3           # owners of more than one chunk on either trip


@pytest.mark.parametrize("n_cu", [256, 304])
def test_table_size_cases_plan_their_arms(n_cu, monkeypatch):
    monkeypatch.delenv("NATAC_COACCESS_TABLE_MAX", raising=False)
    monkeypatch.delenv("NATAC_COACCESS_CHUNK", raising=False)
    for n, arm, lds in ((16384, "table", 65536), (16385, "search", 65536), (5000, "table", 20000)):
        case = R.make_case(n, 40, n, 3000, partners=6)
        p = _plan_of(case, n_cu)
        assert p == dict(arm=arm, table_max=16384, lanes=64, chunk=8192, wg=256, lds_bytes=lds, grid=len(case["order"])) and p["grid"] == 41
        L, ip, ix = np.diff(case["indptr"]), case["indptr"], case["indices"]
        last = [w for w in range(40) if L[w] and ix[ip[w + 1] - 1] == n - 1]
        assert L[2] == n and 2 in last and len(last) >= 3 and set(last) <= set(case["order"].tolist()) and L[7:].max() > 4096
