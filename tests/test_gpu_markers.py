"""The device part of `pyatac markers` on the GPU (natac_group_rank_sums, csrc/natac_markers.hpp; Context.group_rank_sums) against the
exact restatement of tests/markers_ref.py -- all four arrays are integers and are compared for equality -- and the command end to end.

Shapes: 300 windows; 2, 63, 64, 65, 200 and 1100 cells (a lane group's and a wave's border, more than one chunk and more than one
workgroup in the long arm); 1, 2, 5 and 255 groups.  Every case holds an empty row, a row of one entry, a dense row, rows whose values are
all equal through different (a, d), the pair that collides in fp64, counts and depths next to 2^31 - 1 (markers_ref.make_case).  A case
cannot hold a group without a cell and a group with every cell unless G == 2 leaves it nothing else, so: G == 1 is the group that holds
every cell, the cases with G > 2 end in a group without a cell, and two more cases put every cell into one group of several.
The thresholds are forced (NATAC_MARKERS_SHORT_MAX / NATAC_MARKERS_BLOCK_MAX) so that at 200 and 1100 cells every arm takes rows with the
short / block border at 16 and at 64; the long arm's chunk follows the block border (16, 32, 64, 128 and 512 entries here), so its rows
have up to 18 chunks with a last one that is not full."""
import ctypes as C
import os

import numpy as np
import pytest

import markers_ref as R

pytestmark = pytest.mark.gpu

_REF = {}
NAMES = ("detected", "total", "rank2", "ties")
# (NATAC_MARKERS_SHORT_MAX, NATAC_MARKERS_BLOCK_MAX); None: the defaults
SETTINGS = {2: [None, (1, 1)], 63: [None, (16, 32)], 64: [None, (16, 32)], 65: [None, (16, 64)], 200: [(16, 64), (64, 128), None],
            1100: [(16, 64), (64, 512), None]}


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _case(N, G, **kw):
    """a case and its reference, computed once and shared"""
    key = (N, G) + tuple(sorted(kw.items()))
    if key not in _REF:
        case = R.make_case(5000 + 7 * N + G, N, G, **kw)
        _REF[key] = (case, R.rank_sums(case["indptr"], case["indices"], case["data"], N, case["depth"], case["group"], G))
    return _REF[key]


def _force(monkeypatch, setting):
    for name, v in zip(("NATAC_MARKERS_SHORT_MAX", "NATAC_MARKERS_BLOCK_MAX"), setting or (None, None)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _call(case, **kw):
    return _ctx().group_rank_sums(case["indptr"], case["indices"], case["data"], case["N"], case["depth"], case["group"], case["G"], **kw)


def _arms_of(case, setting):
    s, b = setting or (64, 8192)
    L = np.diff(case["indptr"])
    return [int((L <= s).sum()), int(((L > s) & (L <= b)).sum()), int((L > max(s, b)).sum())]


def _check(case, ref, monkeypatch, setting):
    _force(monkeypatch, setting)
    got = _call(case, with_arm_rows=True)
    for name, a, b in zip(NAMES, got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = np.argwhere(a != b)
        assert len(bad) == 0, "%s under %s: %d differ, the first at %s: %d against %d" % (name, setting, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])
    assert got[4].tolist() == _arms_of(case, setting), setting
    return got[4]


@pytest.mark.parametrize("G", [1, 2, 5, 255])
@pytest.mark.parametrize("N", [2, 63, 64, 65, 200, 1100])
def test_against_the_restatement(N, G, monkeypatch):
    case, ref = _case(N, G)
    (a0, d0), (a1, d1) = R.COLLIDING
    assert a0 / d0 == a1 / d1 and a0 * d1 != a1 * d0                   # row 5: equal as fp64 quotients, different exactly
    assert case["depth"][:2].tolist() == [d0, d1] and case["data"][case["indptr"][5]:case["indptr"][6]].tolist() == [a0, a1]
    n_g = np.bincount(case["group"], minlength=G)
    assert (n_g[-1] == 0) if G > 2 else (n_g.min() > 0 or N == 2)
    for setting in SETTINGS[N]:
        arms = _check(case, ref, monkeypatch, setting)
        if N >= 200 and setting is not None:
            assert (arms > 0).all(), (setting, arms)
    if N == 65:                                                        # the defaults at 65 cells: the dense row is the block arm's only one
        assert _arms_of(case, None)[1] >= 1 and _arms_of(case, (16, 64))[2] >= 1


@pytest.mark.parametrize("N,G", [(65, 5), (200, 2)])
def test_every_cell_in_one_group(N, G, monkeypatch):
    case, ref = _case(N, G, all_in_one=True)
    assert np.bincount(case["group"], minlength=G).tolist().count(0) == G - 1
    for setting in SETTINGS[N]:
        _check(case, ref, monkeypatch, setting)


def test_same_bytes_twice_and_under_every_threshold(monkeypatch):
    case, ref = _case(200, 5)
    _force(monkeypatch, None)
    first = _call(case)
    again = _call(case)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    seen = set()
    for setting in ((16, 64), (64, 128), (1, 1), (32, 8192), (64, 64)):
        _force(monkeypatch, setting)
        got = _call(case, with_arm_rows=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, got[:4])), setting
        seen.add(tuple(got[4].tolist()))
    assert len(seen) == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(first, ref))


def test_row_blocks_do_not_change_the_result(monkeypatch):
    from nucleoatac_amd import _lib as L
    case, ref = _case(200, 5)
    _force(monkeypatch, (16, 64))
    got = _call(case, with_arm_rows=True, max_out=5 * 7)              # 43 calls of 7 rows
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], ref)) and got[4].tolist() == _arms_of(case, (16, 64))
    got = _call(case, max_out=1)                                       # never below a row
    assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    with pytest.raises(ValueError):
        _call(case, max_out=L.MARKERS_MAX_OUT + 1)
    # a matrix without a row is an answer without a row
    empty = _ctx().group_rank_sums(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), 3, [1, 2, 3], [0, 1, 0], 2)
    assert [a.shape for a in empty] == [(0, 2), (0, 2), (0, 2), (0,)]


def test_bad_operands_are_refused_with_the_outputs_untouched():
    from nucleoatac_amd import _lib as L
    ctx = _ctx()
    lib = L.load()
    good = dict(ptr=np.array([0, 2, 2, 5], np.int64), col=np.array([0, 2, 0, 1, 3], np.int32), cnt=np.array([1, 2, 3, 1, 1], np.int32),
                depth=np.array([4, 1, 9, 2], np.int64), group=np.array([0, 1, 1, 0], np.int32), n=4, G=2)

    def call(**kw):
        a = dict(good, **kw)
        m = len(a["ptr"]) - 1
        outs = [np.full((m, 256), -7, np.int32), np.full((m, 256), -7, np.int64), np.full((m, 256), -7, np.int64), np.full(m, -7, np.int64)]
        rc = lib.natac_group_rank_sums(ctx._h, m, a["n"], _vp(a["ptr"]), _vp(a["col"]), _vp(a["cnt"]), _vp(a["depth"]), _vp(a["group"]), a["G"],
                                       _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(outs[3]), None, None)
        return rc, outs, lib.natac_last_error().decode()

    rc, outs, _ = call()
    want = R.rank_sums(good["ptr"], good["col"], good["cnt"], 4, good["depth"], good["group"], 2)
    assert rc == 0 and all(np.array_equal(o.reshape(-1)[:w.size], w.reshape(-1)) for o, w in zip(outs, want))
    bad = [
        ("unsorted columns", dict(col=np.array([0, 2, 1, 0, 3], np.int32)), "row 2: columns must be strictly ascending"),
        ("a repeated column", dict(col=np.array([2, 2, 0, 1, 3], np.int32)), "row 0: columns must be strictly ascending"),
        ("a column out of range", dict(col=np.array([0, 4, 0, 1, 3], np.int32)), "row 0: column 4 outside [0, 4)"),
        ("count below 1", dict(cnt=np.array([1, 2, 3, 0, 1], np.int32)), "row 2: count 0 is below 1"),
        ("depth 0", dict(depth=np.array([4, 1, 0, 2], np.int64)), "depth[2] = 0 outside [1, 2^31)"),
        ("depth 2^31", dict(depth=np.array([4, 1 << 31, 9, 2], np.int64)), "depth[1] = 2147483648 outside [1, 2^31)"),
        ("group == n_groups", dict(group=np.array([0, 1, 1, 2], np.int32)), "group[3] = 2 outside [0, 2)"),
        ("a negative group", dict(group=np.array([-1, 1, 1, 0], np.int32)), "group[0] = -1 outside [0, 2)"),
        ("n = 1", dict(n=1), "n must be in [2, 1048576] (got 1)"),
        ("n above 2^20", dict(n=(1 << 20) + 1), "n must be in [2, 1048576]"),
        ("n_groups = 256", dict(G=256), "n_groups must be in [1, 255] (got 256)"),
        ("n_groups = 0", dict(G=0), "n_groups must be in [1, 255] (got 0)"),
        ("row_ptr not monotone", dict(ptr=np.array([0, 2, 1, 5], np.int64)), "row_ptr is not monotone (row 1)"),
        ("null depth", dict(depth=None), "null argument"),
        ("null col", dict(col=None), "null argument"),
    ]
    for name, kw, text in bad:
        rc, outs, err = call(**kw)
        assert rc == -1 and text in err, (name, rc, err)               # NATAC_E_ARG
        assert all((o == -7).all() for o in outs), name
    rc = lib.natac_group_rank_sums(ctx._h, L.MARKERS_MAX_OUT // 2 + 1, 4, _vp(np.zeros(2, np.int64)), None, None, _vp(good["depth"]),
                                   _vp(good["group"]), 2, None, None, None, None, None, None)
    assert rc == -1 and "m x n_groups at most 33554432" in lib.natac_last_error().decode()
    with pytest.raises(L.NatacError):
        ctx.group_rank_sums(good["ptr"], good["col"], good["cnt"], 4, good["depth"], good["group"], 1)      # group 1 with one group
    rc, outs, _ = call()
    assert rc == 0 and np.array_equal(outs[3], want[3])                # the context works afterwards


# ---- the command end to end ---------------------------------------------------------------------------------------------------------------
def test_command_on_a_planted_case(tmp_path):
    """three groups of 60 cells; windows 40 g .. 40 g + 39 are 8 times more open in group g: the device run's files equal the files of
    the run with the restatement in the device's place byte for byte, and every planted window is a marker of its group"""
    from nucleoatac_amd.pyatac import get_markers as GM
    from nucleoatac_amd.pyatac.cli import main, pyatac_parser
    X, barcodes, grp = R.planted_case(seed=3, n_groups=3, per_group=60, n_windows=400, planted=40, fold=8.0)
    groups = str(tmp_path / "clusters.tsv")
    with open(groups, "w") as f:
        f.write("".join("%s\tc%d\n" % (b.decode(), g + 1) for b, g in zip(barcodes, grp)))
    cx = R.write_counts(str(tmp_path / "dev"), X, barcodes, "mtx")
    assert main(["markers", "--counts", cx, "--groups", groups, "--fdr", "0.01", "--out", str(tmp_path / "dev")]) == 0
    host = GM.get_markers(pyatac_parser().parse_args(["markers", "--counts", R.write_counts(str(tmp_path / "host"), X, barcodes, "npz"),
                                                       "--groups", groups, "--fdr", "0.01", "--out", str(tmp_path / "host")]), rank=R.device_stand_in)
    assert [os.path.basename(p) for p in host] == ["host.markers" + s for s in (".npz", ".tsv", ".txt", ".c1.bed", ".c2.bed", ".c3.bed")]
    for p in host:
        assert open(p, "rb").read() == open(p.replace("host.markers", "dev.markers"), "rb").read(), p
    chrom, start, end = R.regions(400)
    for g in range(3):
        found = {(ln.split("\t")[0], int(ln.split("\t")[1])) for ln in open(str(tmp_path / ("dev.markers.c%d.bed" % (g + 1)))) if ln}
        planted = {(chrom[w], int(start[w])) for w in range(40 * g, 40 * g + 40)}
        assert planted <= found and len(found - planted) <= 2          # at an FDR of 0.01 a window beside the 40 is in order
    # a refusal through the command line leaves nothing behind
    assert main(["markers", "--counts", cx, "--groups", groups, "--fdr", "0", "--out", str(tmp_path / "no")]) == 1
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("no.")]
