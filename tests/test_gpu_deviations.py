"""The device part of `pyatac deviations` on the GPU (natac_motif_deviations and natac_window_base_counts, csrc/natac_deviations.hpp;
Context.motif_deviations, Context.base_counts(per_range=True)) against the NumPy restatement of tests/deviations_ref.py, and the command
end to end.

Shapes: about 300 windows; 1, 63, 64, 65 and 200 cells with the tile forced to 64, so that a tile border, a tile of one cell and rows that
straddle tiles all occur; 1 and 5 motifs, one with a single window and one with every window; 2, 7 and 50 background sets; counts from a
mix of rates with one entry near 2^30; and a bg that maps every window to the window of that entry, which takes a counter past 2^32.

Bounds, with u = 2^-53 and s = 1 + max_b |Y_b| per element: |raw - ref| <= 8 u (1 + |ref|), |bg_mean - ref| <= 2 (B + 8) u s,
|bg_m2 - ref| <= 2 (B + 8) u B s^2 -- twice what each evaluation owes the exact value; tests/test_deviations_host.py holds the restatement
to the single bounds against exact rationals.  The integer sums are compared for equality."""
import ctypes as C
import os

import numpy as np
import pytest

import deviations_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
_REF = {}


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _case(seed, **kw):
    """a case and its reference, computed once and shared"""
    key = (seed,) + tuple(sorted(kw.items()))
    if key not in _REF:
        case = R.make_case(seed, **kw)
        _REF[key] = (case, R.reference_of(case))
    return _REF[key]


def _call(case, N, M, **kw):
    ip, ix, da = case["csr"]
    hp, hx = case["hits"]
    return _ctx().motif_deviations(ip, ix, da, N, hp, hx, M, case["bg"], **kw)


def _check(got, ref, B, report=None):
    raw, mean, m2, O, E = got
    O0, E0, raw0, mean0, m20, s = ref
    assert np.array_equal(O, O0) and np.array_equal(E, E0)
    ratios = (np.abs(raw - raw0) / (U * (1 + np.abs(raw0))), np.abs(mean - mean0) / ((B + 8) * U * s),
              np.abs(m2 - m20) / ((B + 8) * U * B * s * s))
    worst = [float(r.max()) for r in ratios]
    equal = all(np.array_equal(a, b) for a, b in ((raw, raw0), (mean, mean0), (m2, m20)))
    print("largest |raw - ref| / (u (1 + |ref|)) %.3g, |mean - ref| / ((B + 8) u s) %.3g, |m2 - ref| / ((B + 8) u B s^2) %.3g; bit-equal: %s"
          % (worst[0], worst[1], worst[2], equal))
    assert worst[0] <= 8 and worst[1] <= 2 and worst[2] <= 2
    return worst


@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("B", [2, 7, 50])
def test_against_the_restatement(N, M, B, monkeypatch):
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "64")
    case, ref = _case(1000 + 31 * N + 7 * M + B, P=300 - (N + B) % 9, N=N, M=M, B=B)
    _check(_call(case, N, M, with_sums=True), ref, B)


@pytest.mark.parametrize("N,M,B", [(65, 5, 7), (200, 1, 2), (1, 5, 50)])
def test_every_window_to_one_window(N, M, B, monkeypatch):
    """bg maps every window to the window that holds the entry near 2^30: with every window annotated a counter reaches 300 x 2^30"""
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "64")
    case, ref = _case(2000 + N + B, P=300, N=N, M=M, B=B, collapse=True)
    assert ref[0].max() >= 1 << 32
    _check(_call(case, N, M, with_sums=True), ref, B)


def test_same_bytes_twice_and_under_every_tile(monkeypatch):
    case, ref = _case(3000, P=301, N=200, M=5, B=7)
    outs = []
    for tile in ("64", "64", "4096", None, "1", "37"):
        if tile is None:
            monkeypatch.delenv("NATAC_DEVIATIONS_CELL_TILE", raising=False)
        else:
            monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", tile)
        outs.append(_call(case, 200, 5, with_sums=True))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert a.tobytes() == b.tobytes()
    _check(outs[0], ref, 7)
    # a matrix wider than the default tile: the last tile is partial, and the forced tiles agree with it
    case, ref = _case(3001, P=60, N=4100, M=2, B=2, big=False)
    monkeypatch.delenv("NATAC_DEVIATIONS_CELL_TILE", raising=False)
    wide = _call(case, 4100, 2, with_sums=True)
    _check(wide, ref, 2)
    for tile in ("64", "4096"):
        monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", tile)
        for a, b in zip(_call(case, 4100, 2, with_sums=True), wide):
            assert a.tobytes() == b.tobytes()


def test_kernel_ms_and_no_motif():
    case, ref = _case(3000, P=301, N=200, M=5, B=7)
    out = _call(case, 200, 5, with_kernel_ms=True)
    assert len(out) == 4 and out[3] > 0 and np.array_equal(out[0], _call(case, 200, 5)[0])
    ip, ix, da = case["csr"]
    raw, mean, m2 = _ctx().motif_deviations(ip, ix, da, 200, np.zeros(302, np.int64), np.zeros(0, np.int64), 0, case["bg"])
    assert raw.shape == mean.shape == m2.shape == (0, 200)


def test_refusals_leave_the_outputs_untouched():
    """every operand check: NATAC_E_ARG, a message that names the index, sentinels intact, and the context works afterwards"""
    from nucleoatac_amd import _lib as L
    ctx = _ctx()
    lib = ctx._lib
    X = np.array([[1, 0, 2], [0, 3, 0], [4, 0, 0], [0, 1, 1]], np.int64)
    good = dict(m=4, n=3, ptr=np.array([0, 2, 3, 4, 6], np.int64), col=np.array([0, 2, 1, 0, 1, 2], np.int32),
                cnt=np.array([1, 2, 3, 4, 1, 1], np.int32), M=2, mp=np.array([0, 1, 3], np.int64), mw=np.array([2, 0, 3], np.int32), B=2,
                bg=np.array([[1, 0, 3, 2], [0, 0, 0, 0]], np.int32), sums=True)

    def call(**kw):
        a = dict(good, **kw)
        outs = [np.full((a["M"], a["n"]), -7.0) for _ in range(3)]
        O, E = np.full((a["B"] + 1, a["M"], a["n"]), -7, np.int64), np.full((a["B"] + 1, a["M"]), -7, np.int64)
        rc = lib.natac_motif_deviations(ctx._h, a["m"], a["n"], _vp(a["ptr"]), _vp(a["col"]), _vp(a["cnt"]), a["M"], _vp(a["mp"]), _vp(a["mw"]),
                                        a["B"], _vp(a["bg"]), _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(O) if a["sums"] else None,
                                        _vp(E) if a["sums"] is True else None, None)
        return rc, outs + [O, E], lib.natac_last_error().decode()

    rc, outs, _ = call()
    assert rc == 0
    sets = [np.array([2]), np.array([0, 3])]
    full = np.vstack([np.arange(4)[None, :], good["bg"]])
    O0, E0 = R.sums(X, sets, full)
    assert np.array_equal(outs[3], O0) and np.array_equal(outs[4], E0)
    raw0, mean0, m20, _ = R.statistics(O0, E0, X.sum(axis=0), int(X.sum()))
    assert np.allclose(outs[0], raw0, rtol=1e-14, atol=1e-15) and np.allclose(outs[1], mean0, rtol=1e-13, atol=1e-15)
    huge = good["cnt"].copy()
    huge[0] = (1 << 31) - 11                                  # the others add up to 11
    bad = [
        ("B below 2", dict(B=1, bg=good["bg"][:1]), "[2, 1024] (got 1)"),
        ("B above 1024", dict(B=1025, bg=np.zeros((1025, 4), np.int32)), "[2, 1024] (got 1025)"),
        ("row_ptr not monotone", dict(ptr=np.array([0, 2, 1, 4, 6], np.int64)), "not monotone (row 1)"),
        ("row_ptr[0] negative", dict(ptr=np.array([-1, 2, 3, 4, 6], np.int64)), "row_ptr[0] is negative"),
        ("column out of range", dict(col=np.array([0, 3, 1, 0, 1, 2], np.int32)), "row 0: column 3 outside [0, 3)"),
        ("columns not ascending", dict(col=np.array([0, 2, 1, 0, 2, 1], np.int32)), "row 3: columns must be strictly ascending"),
        ("count below 1", dict(cnt=np.array([1, 2, 0, 4, 1, 1], np.int32)), "row 1: count 0 is below 1"),
        ("a window without an entry", dict(ptr=np.array([0, 2, 2, 4, 6], np.int64)), "window 1 has no entry"),
        ("a cell without an entry", dict(col=np.array([0, 1, 1, 0, 0, 1], np.int32)), "cell 2 has no entry"),
        ("an empty motif set", dict(mp=np.array([0, 0, 3], np.int64)), "motif 0 has no window"),
        ("an unsorted motif set", dict(mw=np.array([2, 3, 0], np.int32)), "motif 1: windows must be strictly ascending"),
        ("a repeated window", dict(mw=np.array([2, 3, 3], np.int32)), "motif 1: windows must be strictly ascending"),
        ("a motif window out of range", dict(mw=np.array([4, 0, 3], np.int32)), "motif 0: window 4 outside [0, 4)"),
        ("bg out of range", dict(bg=np.array([[1, 0, 3, 2], [0, 4, 0, 0]], np.int32)), "bg[5] = 4 outside [0, 4)"),
        ("bg negative", dict(bg=np.array([[1, -1, 3, 2], [0, 0, 0, 0]], np.int32)), "bg[1] = -1 outside [0, 4)"),
        ("total of 2^31", dict(cnt=huge), "the total count reaches 2^31"),
        ("null col", dict(col=None), "null argument"),
        ("null bg", dict(bg=None), "null argument"),
        ("null mot_win", dict(mw=None), "null argument"),
        ("obs without expect", dict(sums="half"), "obs and expect go together"),
        ("negative m", dict(m=-1), "m and n must be in [0, 2^31)"),
    ]
    for name, kw, text in bad:
        rc, outs, err = call(**kw)
        assert rc == -1 and text in err, (name, rc, err)                                   # NATAC_E_ARG
        assert all((o == -7).all() for o in outs), name
    # the testing output is refused past 2^24 values, and a NULL output where the size is positive
    rc, _, err = call(B=1024, bg=np.zeros((1024, 4), np.int32), n=3, M=2, sums=False)
    assert rc == 0
    n_big = 8192
    ptr = np.array([0, n_big], np.int64)
    outs = [np.full((2, n_big), -7.0) for _ in range(3)]
    O, E = np.full(4, -7, np.int64), np.full(4, -7, np.int64)
    rc = lib.natac_motif_deviations(ctx._h, 1, n_big, _vp(ptr), _vp(np.arange(n_big, dtype=np.int32)), _vp(np.ones(n_big, np.int32)), 2,
                                    _vp(np.array([0, 1, 2], np.int64)), _vp(np.zeros(2, np.int32)), 1024, _vp(np.zeros((1024, 1), np.int32)),
                                    _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(O), _vp(E), None)
    assert rc == -1 and "holds at most 16777216 values (asked for 16793600)" in lib.natac_last_error().decode() and (O == -7).all()
    assert L.DEVIATIONS_MAX_DEBUG == 1 << 24
    with pytest.raises(L.NatacError):
        ctx.motif_deviations(good["ptr"], good["col"], good["cnt"], 3, np.array([0, 1, 1, 2, 3]), np.array([1, 0, 1]), 3, good["bg"])   # motif 2 empty
    rc, outs, _ = call()
    assert rc == 0 and np.array_equal(outs[3], O0)                                         # the context works afterwards


def test_window_base_counts():
    rng = np.random.default_rng(8)
    seq = rng.choice(np.frombuffer(b"ACGTacgtNnRX-", np.uint8), 5000)
    seq[:70] = np.frombuffer(b"acgtn" * 14, np.uint8)                                      # a lower-case start
    starts = [0, 0, 10, 10, 4999, 5000, 4930, 0, 2500, 100, 100, 64, 63, 3000]
    ends = [5000, 1, 10, 75, 5000, 5000, 5000, 70, 2500, 164, 165, 128, 129, 3001]        # whole, one base, empty, overlapping, both ends
    starts += rng.integers(0, 4000, 300).tolist()
    ends += [s + int(w) for s, w in zip(starts[14:], rng.integers(0, 900, 300))]
    got = _ctx().base_counts(seq, starts, ends, per_range=True)
    want = R.base_counts(seq, starts, ends)
    assert got.dtype == np.int64 and got.shape == (314, 4) and np.array_equal(got, want)
    assert want[2].tolist() == [0, 0, 0, 0] and want[7].tolist() == [14, 14, 14, 14] and want[0].sum() < 5000
    assert np.array_equal(_ctx().base_counts(seq, starts, ends), want.sum(axis=0))           # the default form is the sum, unchanged
    assert np.array_equal(_ctx().base_counts(seq), want[0])
    assert _ctx().base_counts(seq, [], [], per_range=True).shape == (0, 4)
    from nucleoatac_amd import _lib as L
    for s, e in (([0, -1], [5, 5]), ([0, 7], [5, 6]), ([0, 10], [5, 5001])):
        with pytest.raises(L.NatacError) as err:
            _ctx().base_counts(seq, s, e, per_range=True)
        assert "range 1 " in str(err.value)


# ---- the command end to end ---------------------------------------------------------------------------------------------------------------
def test_command_on_a_planted_case(tmp_path):
    """two cell groups; the windows of motif PLANT carry three times the counts in group A: PLANT ranks first by variability, its group
    means have opposite signs, and the four files equal those made from the restatement.  One accessibility bin: the planted windows are
    the most accessible ones, so a grid that matches accessibility finely draws their background mostly from themselves."""
    from nucleoatac_amd.pyatac.cli import main
    rng = np.random.default_rng(12)
    P, N = 240, 40
    H = np.zeros((P, 3), np.int64)
    H[rng.choice(P, 40, replace=False), 0] = 1
    H[rng.random(P) < 0.2, 1] = 1
    H[rng.random(P) < 0.15, 2] = 2
    rate = np.full((P, N), 0.5)
    rate[np.ix_(H[:, 0] > 0, np.arange(N) < 20)] *= 3.0
    X = rng.poisson(rate)
    X[np.arange(P), rng.integers(0, N, P)] += 1
    barcodes = [b"CELL%03d" % i for i in range(N)]
    ids, alts = ["PLANT", "RND.1", "RND.2"], ["planted factor", "", "other"]
    seqs = R.write_fasta(str(tmp_path / "g.fa"))
    chrom, start, end = R.regions(P)
    base = str(tmp_path / "planted")
    cx, ch = R.write_inputs(base, X, H, barcodes, ids, alts, "mtx", "npz")
    groups = str(tmp_path / "clusters.tsv")
    with open(groups, "w") as f:
        f.write("".join("%s\t%s\n" % (b.decode(), "A" if i < 20 else "B") for i, b in enumerate(barcodes)))
    assert main(["deviations", "--counts", cx, "--motifs", ch, "--fasta", str(tmp_path / "g.fa"), "--groups", groups, "--iterations", "20",
                 "--gc_bins", "4", "--acc_bins", "1", "--seed", "3", "--out", base]) == 0
    gc = [R.gc_content(seqs[c], s, e) for c, s, e in zip(chrom, start, end)]
    res = R.deviations(X, H, gc, B=20, gc_bins=4, acc_bins=1, seed=3)
    want = R.file_contents(res, ids, alts, barcodes, 20, 3, groups=[("A", barcodes[:20]), ("B", barcodes[20:])])
    var = open(base + ".deviations.variability.tsv").read()
    grp = open(base + ".deviations.groups.tsv").read()
    assert var.split("\n")[1].split("\t")[:2] == ["PLANT", "planted factor"] and var.split("\n")[1].split("\t")[4] == "1"
    a, b = (float(v) for v in grp.split("\n")[1].split("\t")[1:])
    assert grp.split("\n")[0] == "id\tA\tB" and a > 0 > b
    assert var == want["variability"] and grp == want["groups"] and open(base + ".deviations.txt").read() == want["summary"]
    assert open(base + ".deviations.npz", "rb").read() == R.npz_bytes(want["npz"])
    # the other forms of the inputs give the same bytes
    cx2, ch2 = R.write_inputs(str(tmp_path / "other"), X, H, barcodes, ids, alts, "npz", "mtx")
    assert main(["deviations", "--counts", cx2, "--motifs", ch2, "--fasta", str(tmp_path / "g.fa"), "--groups", groups, "--iterations", "20",
                 "--gc_bins", "4", "--acc_bins", "1", "--seed", "3", "--out", str(tmp_path / "other")]) == 0
    for suffix in (".npz", ".variability.tsv", ".groups.tsv", ".txt"):
        assert open(base + ".deviations" + suffix, "rb").read() == open(str(tmp_path / "other") + ".deviations" + suffix, "rb").read()
    # a refusal through the command line leaves nothing behind
    assert main(["deviations", "--counts", cx, "--motifs", ch, "--fasta", str(tmp_path / "g.fa"), "--iterations", "1", "--out", str(tmp_path / "no")]) == 1
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("no.")]
