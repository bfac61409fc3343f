"""The device part of `pyatac coaccess` on the GPU (natac_window_pair_sums, csrc/natac_coaccess.hpp; Context.window_pair_sums) against the
exact restatement of tests/coaccess_ref.py -- both arrays are integers and are compared for equality -- and the command end to end.

Shapes: 300 windows x 200 cells with about 10 partners an owner and mean row lengths of about 8, 24 and 50 (lane groups of 16, 32 and 64
lanes), and 63, 64 and 65 cells (a lane group's and a wave's border); every case holds an empty listed row, a row of one entry, a row with
every cell, two identical rows, two rows with disjoint columns, a window listed twice, owners without partners and two chromosomes
(coaccess_ref.make_case).  Each runs through the table arm and, with NATAC_COACCESS_TABLE_MAX=1, through the search arm; one case of
20,000 cells takes the search arm by itself.  NATAC_COACCESS_CHUNK=16 walks owners of 15, 16, 17, 33 and 100 entries in up to 7 chunks.
arm_owners is asserted everywhere, so that the arm under test demonstrably ran."""
import ctypes as C
import os

import numpy as np
import pytest

import coaccess_ref as R

pytestmark = pytest.mark.gpu

_REF = {}
SHAPES = [(200, 8), (200, 24), (200, 50), (63, 8), (64, 24), (65, 40)]          # (cells, mean row length)


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _case(N, mean_len, m=300, **kw):
    """a case and its reference, computed once and shared"""
    key = (N, mean_len, m) + tuple(sorted(kw.items()))
    if key not in _REF:
        case = R.make_case(900 + 3 * N + mean_len, m, N, mean_len, **kw)
        _REF[key] = (case, R.pair_sums_sparse(case["indptr"], case["indices"], case["data"], N, case["order"], case["hi"]))
    return _REF[key]


def _force(monkeypatch, table_max=None, chunk=None):
    for name, v in (("NATAC_COACCESS_TABLE_MAX", table_max), ("NATAC_COACCESS_CHUNK", chunk)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _call(case, **kw):
    return _ctx().window_pair_sums(case["indptr"], case["indices"], case["data"], case["N"], case["order"], case["hi"], **kw)


def _with_partners(case):
    return int((case["hi"] - np.arange(len(case["hi"])) > 1).sum())


def _check(case, ref, arm, **kw):
    sxy, both, arms = _call(case, with_arm_owners=True, **kw)
    for name, a, b in (("sxy", sxy, ref[0]), ("both", both, ref[1])):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, "%s in the %s arm: %d of %d differ, the first at %d: %d against %d" % (name, arm, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]])
    want = [_with_partners(case), 0] if arm == "table" else [0, _with_partners(case)]
    assert arms.tolist() == want, arm
    return sxy, both


def _lanes(case):
    from nucleoatac_amd.device import window_pair_sums_plan
    L = np.diff(case["indptr"])
    return window_pair_sums_plan(len(L), case["N"], int(L.sum()), len(case["order"]), int(L[case["order"]].sum()))["lanes"]


def test_the_shapes_cover_every_lane_group(monkeypatch):
    _force(monkeypatch)
    assert [_lanes(_case(N, ml)[0]) for N, ml in SHAPES] == [16, 32, 64, 16, 32, 64]


@pytest.mark.parametrize("N,mean_len", SHAPES)
def test_table_arm_against_the_restatement(N, mean_len, monkeypatch):
    case, ref = _case(N, mean_len)
    assert len(ref[0]) > 2000 and ref[1].max() > 0
    _force(monkeypatch)
    _check(case, ref, "table")


@pytest.mark.parametrize("N,mean_len", SHAPES)
def test_search_arm_against_the_restatement(N, mean_len, monkeypatch):
    case, ref = _case(N, mean_len)
    _force(monkeypatch, table_max=1)
    _check(case, ref, "search")


def test_search_arm_by_itself_past_the_table(monkeypatch):
    case, ref = _case(20000, 50, m=64, partners=6)
    assert np.diff(case["indptr"]).max() == 20000
    _force(monkeypatch)
    _check(case, ref, "search")


def test_chunk_loop_gives_the_bytes_of_one_chunk(monkeypatch):
    case, ref = _case(200, 24, long_rows=(15, 16, 17, 33, 100))
    L = np.diff(case["indptr"])
    assert L[7:12].tolist() == [15, 16, 17, 33, 100] and L[2] == 200
    own = case["order"][case["hi"] - np.arange(len(case["hi"])) > 1]
    assert set(range(7, 12)) <= set(own.tolist())                      # each of them owns pairs
    _force(monkeypatch, table_max=1)
    whole = _check(case, ref, "search")
    for chunk in (16, 64):
        _force(monkeypatch, table_max=1, chunk=chunk)
        got = _check(case, ref, "search")
        assert got[0].tobytes() == whole[0].tobytes() and got[1].tobytes() == whole[1].tobytes(), chunk
    _force(monkeypatch, table_max=1, chunk=24)                         # not a power of two: ignored
    _check(case, ref, "search")


def _big(count):
    ptr = np.array([0, 2, 4, 6, 8], np.int64)
    col = np.array([0, 1, 0, 1, 1, 2, 2, 3], np.int32)
    return dict(indptr=ptr, indices=col, data=np.full(8, count, np.int32), N=4, order=np.arange(4, dtype=np.int32), hi=np.full(4, 4, np.int64))


def test_sums_past_32_bits_and_the_bound(monkeypatch):
    case = _big(1 << 29)                                               # 4 * 2^58 * 2 = 2^61 < 2^62
    want = (np.array([1 << 59, 1 << 58, 0, 1 << 58, 0, 1 << 58], np.int64), np.array([2, 1, 0, 1, 0, 1], np.int32))
    ref = R.pair_sums(case["indptr"], case["indices"], case["data"], 4, case["order"], case["hi"])
    assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[1], want[1])
    _force(monkeypatch)
    _check(case, want, "table")
    _force(monkeypatch, table_max=1, chunk=16)
    _check(case, want, "search")
    with pytest.raises(ValueError, match="below 2\\^62"):             # 4 * 2^60 * 2 = 2^63
        _call(_big(1 << 30))
    # the entry itself refuses it too, with the three numbers
    from nucleoatac_amd import _lib as L
    bad = _big(1 << 30)
    out = [np.full(6, -7, np.int64), np.full(6, -7, np.int32)]
    ptr = np.array([0, 3, 5, 6, 6], np.int64)
    rc = L.load().natac_window_pair_sums(_ctx()._h, 4, 4, _vp(bad["indptr"]), _vp(bad["indices"]), _vp(bad["data"]), 4, _vp(bad["order"]), _vp(bad["hi"]),
                                         _vp(ptr), _vp(out[0]), _vp(out[1]), None, None)
    err = L.load().natac_last_error().decode()
    assert rc == -1 and "N = 4" in err and "a_max = 1073741824" in err and "L_max = 2" in err and (out[0] == -7).all() and (out[1] == -7).all()


def test_block_cut_does_not_change_the_result(monkeypatch):
    from nucleoatac_amd import _lib as L
    case, ref = _case(200, 24)
    _force(monkeypatch)
    n_part = case["hi"] - np.arange(len(case["hi"])) - 1
    for cap in (len(ref[0]) // 3, int(n_part.max())):                  # at most a third of the pairs a call: three calls or more
        _check(case, ref, "table", max_pairs=cap)
    _force(monkeypatch, table_max=1, chunk=16)
    _check(case, ref, "search", max_pairs=len(ref[0]) // 5)
    with pytest.raises(ValueError, match="alone has"):
        _call(case, max_pairs=int(n_part.max()) - 1)
    with pytest.raises(ValueError):
        _call(case, max_pairs=L.COACCESS_MAX_PAIRS + 1)
    # nothing listed is an answer without a pair
    none = _ctx().window_pair_sums(case["indptr"], case["indices"], case["data"], 200, np.zeros(0, np.int32), np.zeros(0, np.int64))
    assert none[0].shape == (0,) and none[1].shape == (0,)


def test_same_bytes_twice_and_in_both_arms(monkeypatch):
    case, ref = _case(200, 50)
    _force(monkeypatch)
    first = _call(case)
    again = _call(case)
    _force(monkeypatch, table_max=1)
    other = _call(case)
    for got in (again, other, ref):
        assert first[0].tobytes() == got[0].tobytes() and first[1].tobytes() == got[1].tobytes()


def test_bad_operands_are_refused_and_the_context_goes_on():
    from nucleoatac_amd import _lib as L
    ctx = _ctx()
    lib = L.load()
    good = dict(ptr=np.array([0, 2, 2, 5], np.int64), col=np.array([0, 2, 0, 1, 3], np.int32), cnt=np.array([1, 2, 3, 1, 1], np.int32),
                order=np.array([2, 0, 1, 0], np.int32), hi=np.array([3, 4, 4, 4], np.int64), pp=np.array([0, 2, 4, 5, 5], np.int64), n=4)
    want = R.pair_sums(good["ptr"], good["col"], good["cnt"], 4, good["order"], good["hi"])

    def call(**kw):
        a = dict(good, **kw)
        outs = [np.full(8, -7, np.int64), np.full(8, -7, np.int32)]
        rc = lib.natac_window_pair_sums(ctx._h, len(a["ptr"]) - 1, a["n"], _vp(a["ptr"]), _vp(a["col"]), _vp(a["cnt"]), len(a["order"]),
                                        _vp(a["order"]), _vp(a["hi"]), _vp(a["pp"]), _vp(outs[0]), _vp(outs[1]), None, None)
        return rc, outs, lib.natac_last_error().decode()

    rc, outs, _ = call()
    assert rc == 0 and np.array_equal(outs[0][:5], want[0]) and np.array_equal(outs[1][:5], want[1]) and (outs[0][5:] == -7).all()
    bad = [
        ("unsorted columns", dict(col=np.array([0, 2, 1, 0, 3], np.int32)), "row 2: columns must be strictly ascending"),
        ("a column out of range", dict(col=np.array([0, 4, 0, 1, 3], np.int32)), "row 0: column 4 outside [0, 4)"),
        ("count below 1", dict(cnt=np.array([1, 2, 3, 0, 1], np.int32)), "row 2: count 0 is below 1"),
        ("hi[i] <= i", dict(hi=np.array([3, 1, 4, 4], np.int64)), "hi[1] = 1 outside (1, 4]"),
        ("hi[i] > k", dict(hi=np.array([3, 4, 5, 4], np.int64)), "hi[2] = 5 outside (2, 4]"),
        ("order == m", dict(order=np.array([2, 3, 1, 0], np.int32)), "order[1] = 3 outside [0, 3)"),
        ("a negative order", dict(order=np.array([2, 0, -1, 0], np.int32)), "order[2] = -1 outside [0, 3)"),
        ("pair_ptr[0] != 0", dict(pp=np.array([1, 3, 5, 6, 6], np.int64)), "pair_ptr[0] must be 0"),
        ("an inconsistent pair_ptr", dict(pp=np.array([0, 2, 3, 4, 4], np.int64)), "owner 1 has 2 partners"),
        ("n = 0", dict(n=0), "n must be in [1, 1048576] (got 0)"),
        ("n above 2^20", dict(n=(1 << 20) + 1), "n must be in [1, 1048576]"),
        ("row_ptr not monotone", dict(ptr=np.array([0, 2, 1, 5], np.int64)), "row_ptr is not monotone (row 1)"),
        ("null hi", dict(hi=None), "null argument"),
        ("null col", dict(col=None), "null argument"),
    ]
    for name, kw, text in bad:
        rc, outs, err = call(**kw)
        assert rc == -1 and text in err, (name, rc, err)               # NATAC_E_ARG
        assert all((o == -7).all() for o in outs), name
    # through the binding every one raises, and a good call follows on the same context
    args = (good["ptr"], good["col"], good["cnt"], 4, good["order"], good["hi"])
    for i, v in ((1, np.array([0, 2, 1, 0, 3], np.int32)), (1, np.array([0, 4, 0, 1, 3], np.int32)), (2, np.array([1, 2, 3, 0, 1], np.int32))):
        with pytest.raises(L.NatacError):
            ctx.window_pair_sums(*(args[:i] + (v,) + args[i + 1:]))
    for i, v in ((5, np.array([3, 1, 4, 4])), (5, np.array([3, 4, 5, 4])), (4, np.array([2, 3, 1, 0]))):
        with pytest.raises(ValueError):
            ctx.window_pair_sums(*(args[:i] + (v,) + args[i + 1:]))
        got = ctx.window_pair_sums(*args)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the command end to end ---------------------------------------------------------------------------------------------------------------
def test_command_on_a_tiny_matrix(tmp_path):
    """2 chromosomes, 40 windows, 30 cells: the device run's three files equal the files of the run with the restatement in the device's
    place byte for byte, as single cells and with --aggregate"""
    from nucleoatac_amd.pyatac import get_coaccess as GC
    from nucleoatac_amd.pyatac.cli import main, pyatac_parser
    X, barcodes, grp = R.command_case()
    groups = str(tmp_path / "clusters.tsv")
    with open(groups, "w") as f:
        f.write("".join("%s\tc%d\n" % (b.decode(), g + 1) for b, g in zip(barcodes, grp)))
    os.mkdir(str(tmp_path / "dev"))
    os.mkdir(str(tmp_path / "host"))
    for name, extra in (("cells", ["--min_cells", "5", "--max_distance", "9000", "--fdr", "0.2", "--min_cor", "0.3"]),
                        ("meta", ["--aggregate", groups, "--min_cells", "3", "--max_distance", "9000", "--fdr", "0.5", "--min_cor", "0.2"])):
        dev, host = str(tmp_path / "dev" / name), str(tmp_path / "host" / name)
        assert main(["coaccess", "--counts", R.write_counts(dev, X, barcodes, "mtx"), "--out", dev] + extra) == 0
        paths = GC.get_coaccess(pyatac_parser().parse_args(["coaccess", "--counts", R.write_counts(host, X, barcodes, "npz"), "--out", host] + extra),
                                pairs=R.pair_sums)
        assert [os.path.basename(p) for p in paths] == [name + ".coaccess" + s for s in (".npz", ".bedpe", ".txt")]
        for p in paths:
            assert open(p, "rb").read() == open(p.replace(host, dev), "rb").read(), p
        assert len(open(paths[1]).read().split("\n")) > 3 and "arm\ttable\n" in open(paths[2]).read()
    # a refusal through the command line leaves nothing behind
    no = str(tmp_path / "no")
    assert main(["coaccess", "--counts", R.write_counts(str(tmp_path / "in"), X, barcodes, "npz"), "--fdr", "0", "--out", no]) == 1
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("no.")]
