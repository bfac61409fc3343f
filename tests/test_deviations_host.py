"""CPU: the host part of `pyatac deviations` (nucleoatac_amd/pyatac/get_deviations.py) -- the background table, reading both forms of both
inputs, the dropping rules, the files and every refusal -- against hand-made cases and the restatement of tests/deviations_ref.py, whose
sums stand in for Context.motif_deviations here (the device call is tests/test_gpu_deviations.py); and that restatement itself against
exact rationals."""
import os
from fractions import Fraction

import numpy as np
import pytest

import deviations_ref as R
from nucleoatac_amd.pyatac import get_deviations as GD

U = 2.0 ** -53


def _args(argv):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    return pyatac_parser().parse_args(["deviations"] + argv)


# ---- the background rule ---------------------------------------------------------------------------------------------------------------
def test_grid_reduction():
    assert GD.grid_shape(10000, 25, 25, 10) == (25, 25)
    assert GD.grid_shape(6249, 25, 25, 10) == (25, 24)              # 6249 // 625 = 9: acc_bins goes first on a tie, 6249 // 600 = 10
    assert GD.grid_shape(300, 25, 25, 10) == (6, 5)                 # 25,24 24,24 ... 6,6 6,5 -> 300 // 30 = 10
    assert GD.grid_shape(300, 3, 40, 10) == (3, 10)                 # the larger one alone comes down
    assert GD.grid_shape(5, 25, 25, 10) == (1, 1) and GD.grid_shape(9, 1, 1, 10) == (1, 1)
    assert GD.grid_shape(40, 2, 2, 10) == (2, 2) and GD.grid_shape(39, 2, 2, 10) == (2, 1)
    for P in (1, 7, 50, 299, 300, 1234):
        for g, a, mb in ((25, 25, 10), (4, 9, 3), (1, 30, 7), (30, 1, 1)):
            assert GD.grid_shape(P, g, a, mb) == R.grid_shape(P, g, a, mb)


def test_bin_borders_under_ties():
    # 12 windows, a 2 x 3 grid: gc ties are broken by index, so ranks 0..5 are the windows with gc 0.2 and the first of the 0.5s
    gc = np.array([0.5, 0.2, 0.5, 0.2, 0.5, 0.2, 0.5, 0.2, 0.5, 0.2, 0.9, 0.9])
    rs = np.array([4, 4, 4, 1, 1, 4, 4, 1, 9, 4, 4, 4])
    cell = GD.grid_cells(gc, rs, 2, 3)
    # GC bin 0: windows 1 3 5 7 9 (0.2) and 0 (the first 0.5); by (rs, index): 3 7 | 0 1 | 5 9
    # GC bin 1: windows 2 4 6 8 10 11; by (rs, index): 4 2 | 6 10 | 11 8
    assert cell.tolist() == [1, 1, 3, 0, 3, 2, 4, 0, 5, 2, 4, 5]
    bg, grid, ext = GD.background_table(gc, rs, 6, 2, 3, 2, seed=4)
    assert grid == (2, 3) and ext == (2, 2) and bg.dtype == np.int32 and bg.shape == (6, 12)
    r = np.random.default_rng(4).random((6, 12))
    cand = {0: [3, 7], 1: [0, 1], 2: [5, 9], 3: [2, 4], 4: [6, 10], 5: [8, 11]}
    for b in range(6):
        for p in range(12):
            assert bg[b, p] == cand[cell[p]][int(r[b, p] * 2)]
    ref, rgrid, rext = R.background(gc, rs, 6, 2, 3, 2, seed=4)
    assert np.array_equal(ref[1:], bg) and ref[0].tolist() == list(range(12)) and (rgrid, rext) == (grid, ext)


def test_grid_of_one_cell_and_seed():
    rng = np.random.default_rng(0)
    gc, rs = rng.random(7), rng.integers(1, 9, 7)
    bg, grid, ext = GD.background_table(gc, rs, 3, 25, 25, 10, seed=1)
    assert grid == (1, 1) and ext == (7, 7)
    assert np.array_equal(bg, (np.random.default_rng(1).random((3, 7)) * 7).astype(np.int64))      # the candidates are 0 .. 6
    gc, rs = np.round(rng.random(500), 2), rng.integers(1, 6, 500)                                  # many ties on both axes
    a = GD.background_table(gc, rs, 9, 6, 5, 10, seed=11)
    b = GD.background_table(gc, rs, 9, 6, 5, 10, seed=11)
    c = GD.background_table(gc, rs, 9, 6, 5, 10, seed=12)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[0], c[0]) and a[1:] == c[1:] == ((6, 5), (16, 17))
    assert np.array_equal(R.background(gc, rs, 9, 6, 5, 10, seed=11)[0][1:], a[0])
    cell = GD.grid_cells(gc, rs, 6, 5)
    assert np.array_equal(cell[a[0]], np.broadcast_to(cell, a[0].shape))                            # every draw stays in the window's cell


# ---- the restatement against exact rationals ---------------------------------------------------------------------------------------------
def _exact(O, E, d, T, m, c):
    B = O.shape[0] - 1
    Y = [Fraction(int(O[b, m, c]) * T - int(E[b, m]) * int(d[c]), int(E[b, m]) * int(d[c])) for b in range(B + 1)]
    mean = sum(Y[1:]) / B
    return Y[0], mean, sum((y - mean) ** 2 for y in Y[1:]), 1 + max(abs(y) for y in Y)


def test_reference_by_hand_in_rationals():
    X = np.array([[2, 0, 1], [0, 3, 0], [1, 1, 4]])
    sets = [np.array([0]), np.array([0, 2])]
    bg = np.array([[0, 1, 2], [1, 1, 0], [2, 0, 2]])
    O, E = R.sums(X, sets, bg)
    assert O[0].tolist() == [[2, 0, 1], [3, 1, 5]] and E[0].tolist() == [3, 9]
    assert O[1].tolist() == [[0, 3, 0], [2, 3, 1]] and E[1].tolist() == [3, 6]           # set 1 under bg 1: windows 1 and 0
    assert O[2].tolist() == [[1, 1, 4], [2, 2, 8]] and E[2].tolist() == [6, 12]
    raw, mean, m2, s = R.statistics(O, E, X.sum(axis=0), 12)
    # motif 1, cell 2: x = 9 * 5 / 12, Y_0 = (5 - x) / x = 1 / 3; Y_1 = (1 - 2.5) / 2.5 = -3/5, Y_2 = (8 - 5) / 5 = 3/5
    assert _exact(O, E, X.sum(axis=0), 12, 1, 2)[:3] == (Fraction(1, 3), Fraction(0), Fraction(18, 25))
    assert abs(raw[1, 2] - 1 / 3) <= 4 * U and abs(mean[1, 2]) <= 10 * U * 1.6 and abs(m2[1, 2] - 0.72) <= 10 * U * 2 * 1.6 ** 2


def test_reference_within_its_bounds_of_exact_rationals():
    """the 40-case sweep: the restatement owes the exact value 4 u (1 + |Y|), (B + 8) u s and (B + 8) u B s^2 -- the device tests allow
    twice that against the restatement"""
    worst = np.zeros(3)
    k = 0
    for N in (1, 63, 64, 65, 200):
        for M in (1, 5):
            for B in (2, 7, 50):
                for collapse in ((False, True) if (N, B) in ((65, 7), (200, 2), (1, 50), (64, 50), (63, 2)) else (False,)):
                    case = R.make_case(100 + k, P=300 - k, N=N, M=M, B=B, collapse=collapse)
                    k += 1
                    O, E, raw, mean, m2, s = R.reference_of(case)
                    d, T = case["X"].sum(axis=0), int(case["X"].sum())
                    assert T < 1 << 31
                    rng = np.random.default_rng(k)
                    for m in range(M):
                        for c in set(rng.integers(0, N, 4).tolist()):
                            y0, mu, q, big = _exact(O, E, d, T, m, c)
                            sf = float(big)
                            assert abs(s[m, c] - sf) <= 8 * U * sf
                            e = [abs(Fraction(float(raw[m, c])) - y0) / (U * (1 + abs(y0))), abs(Fraction(float(mean[m, c])) - mu) / ((B + 8) * U * big),
                                 abs(Fraction(float(m2[m, c])) - q) / ((B + 8) * U * B * big * big)]
                            worst = np.maximum(worst, [float(v) for v in e])
    print("cases %d, largest error in units of u (1 + |Y|), (B + 8) u s, (B + 8) u B s^2: %s" % (k, worst))
    assert k == 40 and worst[0] <= 4 and worst[1] <= 1 and worst[2] <= 1


# ---- the command -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("dev_host")
    rng = np.random.default_rng(21)
    P, N, M = 60, 12, 5
    X = rng.poisson(0.4, (P, N))
    X[:, 0:6] += rng.poisson(0.5, (P, 6)) * (np.arange(P) % 4 == 0)[:, None]
    X[np.arange(P), (np.arange(P) % 5) + 5] += 1
    X[7] = 0                                   # a window without a count
    X[:, 4] = 0                                # a cell without a count
    H = (rng.random((P, M)) < 0.25).astype(np.int64) * rng.integers(1, 4, (P, M))
    H[:, 2] = 0
    H[7, 2] = 3                                # motif 2 is annotated only in the dropped window
    H[:, 4] = 0                                # motif 4 has no hit at all
    barcodes = [b"BC%02d" % i for i in range(N)]
    ids, alts = ["M%d" % k for k in range(M)], ["factor %d" % k if k % 2 else "" for k in range(M)]
    seqs = R.write_fasta(str(d / "g.fa"))
    groups = str(d / "groups.tsv")
    with open(groups, "w") as f:
        f.write("".join("%s\t%s\n" % (b.decode(), "c1" if i < 6 else "c2") for i, b in enumerate(barcodes)) + "ABSENT\tc2\n")
    return dict(dir=d, X=X, H=H, barcodes=barcodes, ids=ids, alts=alts, seqs=seqs, fasta=str(d / "g.fa"), groups=groups, regions=R.regions(P))


def _run(world, base, fmt_x, fmt_h, extra=()):
    cx, ch = R.write_inputs(base, world["X"], world["H"], world["barcodes"], world["ids"], world["alts"], fmt_x, fmt_h)
    args = _args(["--counts", cx, "--motifs", ch, "--fasta", world["fasta"], "--out", base, "--iterations", "6", "--min_bin", "4"] + list(extra))
    return GD.get_deviations(args, device=R.device_standin, base_counts=R.base_counts)


def test_both_forms_give_the_same_bytes_and_the_reference_files(world):
    outs = {}
    for fx in ("npz", "mtx"):
        for fh in ("npz", "mtx"):
            base = str(world["dir"] / ("run_%s_%s" % (fx, fh)))
            paths = _run(world, base, fx, fh, ["--groups", world["groups"]])
            assert [os.path.basename(p) for p in paths] == ["run_%s_%s.deviations%s" % (fx, fh, s)
                                                            for s in (".npz", ".variability.tsv", ".txt", ".groups.tsv")]
            outs[fx, fh] = [open(p, "rb").read() for p in paths]
    first = outs["npz", "npz"]
    assert all(o == first for o in outs.values())
    chrom, start, end = world["regions"]
    gc = [R.gc_content(world["seqs"][c], s, e) for c, s, e in zip(chrom, start, end)]
    res = R.deviations(world["X"], world["H"], gc, B=6, min_bin=4)
    want = R.file_contents(res, world["ids"], world["alts"], world["barcodes"], 6, 1,
                           groups=[("c1", world["barcodes"][:6]), ("c2", world["barcodes"][6:] + [b"ABSENT"])])
    assert first[1].decode() == want["variability"] and first[2].decode() == want["summary"] and first[3].decode() == want["groups"]
    assert first[0] == R.npz_bytes(want["npz"])
    # dropped rows and columns, NA rows
    assert res["win_keep"].sum() == 59 and res["cell_keep"].sum() == 11 and res["motif_keep"].tolist() == [True, True, False, True, False]
    lines = first[1].decode().split("\n")
    assert lines[0] == "id\talt\twindows\tvariability\trank" and [ln.split("\t")[4] for ln in lines[1:4]] == ["1", "2", "3"]
    assert lines[4] == "M2\t\t0\tNA\tNA" and lines[5] == "M4\t\t0\tNA\tNA" and lines[6] == ""
    v = [float(ln.split("\t")[3]) for ln in lines[1:4]]
    assert v == sorted(v, reverse=True)
    z = np.load(str(world["dir"] / "run_npz_npz.deviations.npz"))
    assert z["z"].shape == (5, 11) and np.isnan(z["z"][2]).all() and np.isnan(z["deviations"][4]).all() and np.isfinite(z["z"][0]).any()
    assert z["barcodes"].tolist() == [b for i, b in enumerate(world["barcodes"]) if i != 4]
    assert z["windows_annotated"].tolist() == [int(((world["H"][:, k] > 0) & res["win_keep"]).sum()) for k in range(5)]
    g = first[3].decode().split("\n")
    assert g[0] == "id\tc1\tc2" and g[3] == "M2\tNA\tNA" and "windows_dropped\t1\n" in first[2].decode() and "cells_dropped\t1\n" in first[2].decode()
    assert "gc_bins\t4\nacc_bins\t3\nsmallest_bin\t4\nlargest_bin\t5\nseed\t1\n" in first[2].decode()


def test_group_means_by_hand():
    from nucleoatac_amd.pyatac.cellgroups import CellGroups
    z = np.array([[1.0, 2.0, np.nan, 6.0, -1.0], [np.nan, np.nan, 3.0, np.inf, 0.5]])
    groups = CellGroups(["a", "b", "c"], [b"k0", b"k1", b"k3", b"gone", b"k2", b"k4", b"k9"], [0, 0, 0, 0, 1, 1, 2])
    names, out = GD.group_means(z, [b"k0", b"k1", b"k2", b"k3", b"k4"], groups)
    assert names == ["a", "b", "c"]
    assert out[0].tolist()[:2] == [3.0, -1.0] and np.isnan(out[0, 2])               # (1 + 2 + 6) / 3; the NaN cell of b does not count
    assert np.isnan(out[1, 0]) and out[1, 1] == 1.75 and np.isnan(out[1, 2])         # a: no finite z; b: (3 + 0.5) / 2


def test_refusals(world, capsys):
    from nucleoatac_amd.pyatac.cli import pyatac_main
    d = world["dir"]
    base = str(d / "bad")
    cx, ch = R.write_inputs(base, world["X"], world["H"], world["barcodes"], world["ids"], world["alts"], "npz", "mtx")
    ok = ["--counts", cx, "--motifs", ch, "--fasta", world["fasta"], "--out", base]

    def refused(argv, text, **kw):
        with pytest.raises(GD.DeviationsError) as e:
            GD.get_deviations(_args(argv), device=kw.get("device", R.device_standin), base_counts=R.base_counts)
        assert text in str(e.value) and "\n" not in str(e.value)
        assert not [f for f in os.listdir(str(d)) if f.startswith("bad.deviations")]

    refused(ok + ["--iterations", "1"], "--iterations must be in [2, 1024] (got 1)")
    refused(ok + ["--iterations", "1025"], "--iterations must be in [2, 1024] (got 1025)")
    refused(ok + ["--gc_bins", "0"], "--gc_bins, --acc_bins and --min_bin must be at least 1")
    refused(ok + ["--acc_bins", "-3"], "must be at least 1")
    refused(ok + ["--min_bin", "0"], "must be at least 1")
    refused(["--counts", base + ".nope.npz"] + ok[2:], "bad.nope.npz: no such file")
    refused(ok[:2] + ["--motifs", base + ".nope.mtx.gz"] + ok[4:], "bad.nope.mtx.gz: no such file")
    refused(ok[:4] + ["--fasta", str(d / "nope.fa")] + ok[6:], "nope.fa: no such file")
    refused(ok + ["--groups", str(d / "nope.tsv")], "nope.tsv: no such file")
    # region lists that differ: in a coordinate, and in length
    chrom, start, end = world["regions"]
    other = start.copy()
    other[13] += 1
    cx2, ch2 = R.write_inputs(str(d / "bad2"), world["X"], world["H"], world["barcodes"], world["ids"], world["alts"], "mtx", "npz",
                             regions_h=(chrom, other, end))
    refused(["--counts", cx2, "--motifs", ch2] + ok[4:],
            "differ at row 14 (%s:%d-%d against %s:%d-%d): give `cellcounts` and `motifs` the same BED" % (chrom[13], start[13], end[13], chrom[13], other[13], end[13]))
    cx3, ch3 = R.write_inputs(str(d / "bad3"), world["X"], world["H"][:50], world["barcodes"], world["ids"], world["alts"], "npz", "npz",
                             regions_h=(chrom[:50], start[:50], end[:50]))
    refused(["--counts", cx3, "--motifs", ch3] + ok[4:], "differ at row 51 (%s:%d-%d against no such row)" % (chrom[50], start[50], end[50]))
    # nothing left
    cx4, ch4 = R.write_inputs(str(d / "bad4"), world["X"] * 0, world["H"], world["barcodes"], world["ids"], world["alts"], "npz", "npz")
    refused(["--counts", cx4, "--motifs", ch4] + ok[4:], "no window or no cell with a count is left")
    cx5, ch5 = R.write_inputs(str(d / "bad5"), world["X"], world["H"] * (np.arange(5) == 2), world["barcodes"], world["ids"], world["alts"], "npz", "npz")
    refused(["--counts", cx5, "--motifs", ch5] + ok[4:], "no motif with an annotated window is left")
    # a total of 2^31
    big = world["X"].copy()
    big[0, 0] = (1 << 31) - int(world["X"].sum()) + int(world["X"][0, 0])
    cx6, ch6 = R.write_inputs(str(d / "bad6"), big, world["H"], world["barcodes"], world["ids"], world["alts"], "npz", "npz")
    refused(["--counts", cx6, "--motifs", ch6] + ok[4:], "the counts add up to 2147483648, 2^31 or more")
    # a window outside the FASTA, and a chromosome it does not have
    far = (chrom, start + 480, end + 480)
    cx7, ch7 = R.write_inputs(str(d / "bad7"), world["X"], world["H"], world["barcodes"], world["ids"], world["alts"], "npz", "npz", regions_x=far)
    refused(["--counts", cx7, "--motifs", ch7] + ok[4:], "reaches past the chromosome (500 bases)")
    cx8, ch8 = R.write_inputs(str(d / "bad8"), world["X"], world["H"], world["barcodes"], world["ids"], world["alts"], "npz", "npz",
                             regions_x=(["chrZ"] * 60, start, end))
    refused(["--counts", cx8, "--motifs", ch8] + ok[4:], "no chromosome chrZ")
    # through the command line: one line on stderr, exit status 1
    assert pyatac_main(_args(ok + ["--iterations", "1"])) == 1
    err = capsys.readouterr().err
    assert err == "pyatac deviations: --iterations must be in [2, 1024] (got 1)\n"
    for n in range(2, 9):
        assert not [f for f in os.listdir(str(d)) if f.startswith("bad%d.deviations" % n)]


def test_host_matches_reference_on_a_larger_case():
    """the command's own dropping, renumbering, transposition and statistics against the dense restatement"""
    case = R.make_case(77, P=140, N=30, M=5, B=5, big=False)
    X, H = case["X"].copy(), case["H"].copy()
    X[[3, 90]] = 0
    X[:, [0, 17]] = 0
    gc = np.round(np.random.default_rng(2).random(140), 1)
    ip, ix, da = R.csr_of(X)
    hp, hx, hd = R.csr_of(H)
    res = GD.motif_deviations(ip, ix, da, 30, hp, hx, hd, 5, lambda wins: gc[wins], iterations=5, gc_bins=4, acc_bins=4, min_bin=5, seed=9,
                              device=R.device_standin)
    ref = R.deviations(X, H, gc, B=5, gc_bins=4, acc_bins=4, min_bin=5, seed=9)
    for k in ("win_keep", "cell_keep", "motif_keep", "rs", "d", "annotated"):
        assert np.array_equal(res[k], ref[k])
    assert np.array_equal(res["bg"], ref["bg"][1:]) and res["grid"] == ref["grid"] and res["grid_extremes"] == ref["extremes"]
    for k in ("raw", "bg_mean", "bg_m2", "deviations", "z", "variability"):
        assert np.array_equal(res[k], ref[k], equal_nan=True)
