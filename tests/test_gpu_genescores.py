"""natac_gene_cell_scores (csrc/natac_genescores.hpp) and `pyatac genescores` on the GPU against the NumPy restatement of
tests/genescores_ref.py: both arms under the default and the forced thresholds, one and several cell tiles, a hand-made gene whose
expectation is written here, the sizing call and the capacity, every operand rule, the 2^31 bound, determinism, and the command followed
by `markers` on planted cell groups.  All comparisons are == on integers; arm_rows is asserted everywhere, so the arm under test ran."""
import ctypes as C
import functools

import numpy as np
import pytest

import genescores_ref as R

pytestmark = pytest.mark.gpu

ENV = ("NATAC_GENESCORES_SHORT_MAX", "NATAC_GENESCORES_TILE")
E_ARG = -1


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _force(monkeypatch, short_max=None, tile=None):
    for name, v in zip(ENV, (short_max, tile)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


@functools.lru_cache(maxsize=None)
def _case(n_cells, n_genes=120):
    """a crafted chromosome and its restatement, formed once: (case, (indptr, indices, data, hits))"""
    case = R.make_case(seed=n_cells, n_cells=n_cells, n_genes=n_genes)
    want = R.gene_cell_scores(*R.case_args(case), with_hits=True)
    for a in list(case.values()) + list(want):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case, want


def _run(case):
    return _ctx().gene_cell_scores(*R.case_args(case), with_hits=True, with_arm_rows=True)


def _same(got, want):
    return all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


def _arms(hits, short_max):
    return [int(np.count_nonzero((hits > 0) & (hits <= short_max))), int(np.count_nonzero(hits > short_max))]


def test_the_crafted_case_holds_what_it_promises():
    case, (ptr, col, val, hits) = _case(200)
    sp = case["special"]
    assert hits[sp["none"]] == 0 and hits[sp["one"]] == 1 and hits[sp["h64"]] == 64 and hits[sp["h65"]] == 65
    ilen = case["tlen"] - 8
    sized = (ilen >= 0) & (ilen < 1000)
    assert hits[sp["all"]] == 2 * sized.sum() and (ilen < 0).any() and (ilen >= 1000).any() and (ilen == 0).any() and (ilen == 1).any()
    a, b = sp["twin_a"], sp["twin_b"]
    assert a != b and np.array_equal(col[ptr[a]:ptr[a + 1]], col[ptr[b]:ptr[b + 1]]) and np.array_equal(val[ptr[a]:ptr[a + 1]], val[ptr[b]:ptr[b + 1]])
    assert hits[a] > 0 and hits[sp["lap_a"]] > 0 and hits[sp["lap_b"]] > 0 and hits[sp["empty_body"]] > 0 and hits[sp["flush"]] > 0
    assert case["body_lo"][sp["empty_body"]] == case["body_hi"][sp["empty_body"]] and case["win_lo"][sp["flush"]] == case["body_lo"][sp["flush"]]
    assert not np.all(np.diff(case["win_lo"]) >= 0) and 199 not in case["cell"] and 199 not in col
    assert (case["body_lo"] - case["win_lo"]).max() <= R.REACH and (case["win_hi"] - case["body_hi"]).max() <= R.REACH and len(case["weight"]) == R.REACH + 1
    # the record planted with both insertions inside `both` gives its cell two weights of the body
    g = sp["both"]
    row = dict(zip(col[ptr[g]:ptr[g + 1]].tolist(), val[ptr[g]:ptr[g + 1]].tolist()))
    assert row[0] >= 2 * int(case["weight"][0])


@pytest.mark.parametrize("n_cells", (63, 64, 65, 200))
def test_both_arms_against_the_restatement(n_cells, monkeypatch):
    case, want = _case(n_cells)
    hits = want[3]
    _force(monkeypatch)
    got = _run(case)
    assert _same(got[:4], want) and got[4].tolist() == _arms(hits, 64) and got[4].min() >= 10
    assert all(np.all(np.diff(got[1][a:b]) > 0) for a, b in zip(got[0][:-1], got[0][1:])) and got[2].min() >= 1
    _force(monkeypatch, short_max=1)
    forced = _run(case)
    assert _same(forced[:4], want) and forced[4].tolist() == _arms(hits, 1) and forced[4][0] >= 1 and forced[4][1] > got[4][1]


@pytest.mark.parametrize("n_cells,tile", ((65, 64), (200, 64), (63, 16)))
def test_cell_tiles_give_the_bytes_of_one_tile(n_cells, tile, monkeypatch):
    from nucleoatac_amd.device import gene_cell_scores_plan as plan
    case, want = _case(n_cells)
    _force(monkeypatch)
    one = _run(case)
    assert plan(120, n_cells, 10)["n_tiles"] == 1
    for short_max in (None, 1):
        _force(monkeypatch, short_max=short_max, tile=tile)
        assert plan(120, n_cells, 10)["n_tiles"] == -(-n_cells // tile) > 1
        got = _run(case)
        assert _same(got[:4], want) and _same(got[:4], one[:4]) and got[4].tolist() == _arms(want[3], short_max or 64)


def test_twenty_thousand_cells_take_two_tiles(monkeypatch):
    from nucleoatac_amd.device import gene_cell_scores_plan as plan
    case, want = _case(20000, 40)
    _force(monkeypatch)
    p = plan(40, 20000, 5)
    assert (p["tile"], p["n_tiles"]) == (16384, 2)
    got = _run(case)
    assert _same(got[:4], want) and got[4].tolist() == _arms(want[3], 64) and got[4][1] >= 2
    ptr, col = got[0], got[1]
    sp = case["special"]
    row_all, row_top = col[ptr[sp["all"]]:ptr[sp["all"] + 1]], col[ptr[sp["h65"]]:ptr[sp["h65"] + 1]]
    assert row_all.min() < 16384 <= row_all.max() and len(row_top) > 0 and row_top.min() >= 16384 and want[3][sp["h65"]] == 65
    _force(monkeypatch, short_max=1)
    got = _run(case)
    assert _same(got[:4], want) and got[4].tolist() == _arms(want[3], 1)


@pytest.mark.parametrize("ends", ("left", "right", "both"))
def test_hand_made_gene_pins_the_borders(ends, monkeypatch):
    """one gene, window [100, 130), body [110, 120), weight[d] = 1000 + d, insertions at 99, 100, 109, 110, 119, 120, 129, 130 in distinct
    cells: 99 and 130 are outside; 100 is 10 left of the body, 109 is 1; 110 and 119 are in it; 120 is 1 right of it (x - body_hi + 1) and
    129 is 10"""
    x = np.array([99, 100, 109, 110, 119, 120, 129, 130], np.int64)
    worth = [1010, 1001, 1000, 1000, 1001, 1010]                      # of 100 .. 129
    left = (x - 4, np.full(8, 208, np.int64), np.arange(8, dtype=np.int32))                 # l = x, r = x + 199
    right = (x - 199 - 4, np.full(8, 208, np.int64), np.arange(8, 16, dtype=np.int32))      # l = x - 199, r = x
    if ends == "left":
        pos, tlen, cell, cols = left + ([1, 2, 3, 4, 5, 6],)
    elif ends == "right":
        pos, tlen, cell, cols = right + ([9, 10, 11, 12, 13, 14],)
    else:
        pos, tlen, cell = (np.concatenate([b, a]) for a, b in zip(left, right))
        cols, worth = [1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14], worth + worth
    weight = (1000 + np.arange(11)).astype(np.int32)
    g = [np.array([v], np.int64) for v in (100, 130, 110, 120)]
    for short_max, arms in ((None, [1, 0]), (1, [0, 1])):
        _force(monkeypatch, short_max=short_max)
        ptr, col, val, hits, arm = _ctx().gene_cell_scores(pos, tlen, cell, 16, g[0], g[1], g[2], g[3], weight, 0, 1000, with_hits=True,
                                                           with_arm_rows=True)
        assert ptr.tolist() == [0, len(cols)] and col.tolist() == cols and val.tolist() == worth and hits.tolist() == [len(cols)] and arm.tolist() == arms


# ---- the entry itself --------------------------------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


SENTINEL = -7


def _raw(case, cap=0, with_col=False, **change):
    """natac_gene_cell_scores called directly on the case with operands replaced -> (rc, message, row_ptr, col, val, hits, arms); every
    output starts as SENTINEL"""
    from nucleoatac_amd import _lib as L
    lib = L.load()
    a = dict(case, **change)
    i64 = lambda k: None if a[k] is None else np.ascontiguousarray(a[k], np.int64)
    pos, tlen, wl, wh, bs, be = (i64(k) for k in ("pos", "tlen", "win_lo", "win_hi", "body_lo", "body_hi"))
    cell, weight = np.ascontiguousarray(a["cell"], np.int32), np.ascontiguousarray(a["weight"], np.int32)
    ng = len(wl)
    row_ptr, hits, arms = np.full(ng + 1, SENTINEL, np.int64), np.full(ng, SENTINEL, np.int64), np.full(2, SENTINEL, np.int64)
    col = np.full(max(cap, 1), SENTINEL, np.int32) if with_col else None
    val = np.full(max(cap, 1), SENTINEL, np.int32) if with_col and not a.get("no_val") else None
    rc = lib.natac_gene_cell_scores(_ctx()._h, len(pos), _vp(pos), _vp(tlen), _vp(cell), a["n_cells"], ng, _vp(wl), _vp(wh), _vp(bs), _vp(be),
                                    a.get("n_w", len(weight)), _vp(weight), a["lower"], a["upper"], _vp(row_ptr), cap, _vp(col), _vp(val),
                                    _vp(hits), _vp(arms), None)
    return rc, lib.natac_last_error().decode(), row_ptr, col, val, hits, arms


def _untouched(out):
    return all(a is None or (a == SENTINEL).all() for a in out[2:])


def test_sizing_call_and_capacity(monkeypatch):
    _force(monkeypatch)
    case, want = _case(65)
    nnz = int(want[0][-1])
    rc, _, row_ptr, col, val, hits, arms = _raw(case)
    assert rc == 0 and np.array_equal(row_ptr, want[0]) and np.array_equal(hits, want[3]) and arms.tolist() == _arms(want[3], 64)
    rc, msg, row_ptr, col, val, _, _ = _raw(case, cap=nnz - 1, with_col=True)
    assert rc == E_ARG and "cap %d is less than the %d entries" % (nnz - 1, nnz) in msg
    assert np.array_equal(row_ptr, want[0]) and (col == SENTINEL).all() and (val == SENTINEL).all()
    rc, _, row_ptr, col, val, _, arms = _raw(case, cap=nnz, with_col=True)
    assert rc == 0 and np.array_equal(col, want[1]) and np.array_equal(val, want[2]) and arms.tolist() == _arms(want[3], 64)
    # nothing to do: zeros, no launch
    empty = dict(case, pos=case["pos"][:0], tlen=case["tlen"][:0], cell=case["cell"][:0])
    rc, _, row_ptr, _, _, hits, arms = _raw(empty)
    assert rc == 0 and not row_ptr.any() and not hits.any() and arms.tolist() == [0, 0]
    none = dict(case, win_lo=case["win_lo"][:0], win_hi=case["win_hi"][:0], body_lo=case["body_lo"][:0], body_hi=case["body_hi"][:0])
    rc, _, row_ptr, _, _, _, arms = _raw(none)
    assert rc == 0 and row_ptr.tolist() == [0] and arms.tolist() == [0, 0]


def test_every_operand_rule_refuses_and_touches_nothing(monkeypatch):
    _force(monkeypatch)
    case, want = _case(65)

    def bumped(key, i, v):
        a = case[key].copy()
        a[i] = v
        return {key: a}

    n = len(case["pos"])
    g = 17
    wl, bs, be, wh = (int(case[k][g]) for k in ("win_lo", "body_lo", "body_hi", "win_hi"))
    for change, text in ((bumped("pos", 1000, int(case["pos"][999]) - 1), "record 1000"), (bumped("cell", 77, 65), "record 77"),
                         (bumped("cell", n - 1, -1), "record %d" % (n - 1)), (dict(n_cells=0), "n_cells"), (dict(n_cells=(1 << 23) + 1), "n_cells"),
                         (bumped("win_lo", g, bs + 1), "gene 17"), (bumped("body_lo", g, be + 1), "gene 17"), (bumped("win_hi", g, be - 1), "gene 17"),
                         (bumped("win_lo", g, bs - R.REACH - 1), "gene 17"), (bumped("win_hi", g, be + R.REACH + 1), "gene 17"),
                         (bumped("win_hi", 119, 1 << 61), "gene 119"), (dict(n_w=0), "n_w"), (dict(n_w=(1 << 20) + 2), "n_w"),
                         (bumped("weight", 5, 0), "weight[5]"), (bumped("weight", 3000, (1 << 20) + 1), "weight[3000]"), (dict(lower=-1), "lower"),
                         (dict(lower=1000), "lower"), (dict(upper=50001), "upper")):
        out = _raw(case, **change)
        assert out[0] == E_ARG and text in out[1] and _untouched(out), (change.keys(), out[1])
    out = _raw(case, cap=5)                                            # a capacity without arrays
    assert out[0] == E_ARG and _untouched(out)
    out = _raw(case, cap=5, with_col=True, no_val=True)                # col without val
    assert out[0] == E_ARG and _untouched(out)
    # the largest weight the rule allows is taken (on the genes whose hits keep hits x 2^20 below 2^31)
    few = np.flatnonzero(want[3] < 2000)
    small = dict(case, **{k: case[k][few] for k in ("win_lo", "win_hi", "body_lo", "body_hi")})
    ok = _raw(small, **bumped("weight", 5, 1 << 20))
    assert ok[0] == 0 and np.array_equal(ok[5], want[3][few]) and len(few) > 100


def test_the_bound_of_two_to_the_31(monkeypatch):
    _force(monkeypatch)
    n = 1100
    pos = np.full(n, 5000 - 4, np.int64) + np.arange(n) % 50           # l in [5000, 5050), r = l + 99: both inside the second gene
    pos.sort()
    tlen = np.full(n, 108, np.int64)
    cell = (np.arange(n) % 3).astype(np.int32)
    case = dict(pos=pos, tlen=tlen, cell=cell, n_cells=3, win_lo=[100, 4000], win_hi=[200, 6000], body_lo=[150, 4500], body_hi=[160, 5500],
                weight=np.full(1001, 1 << 20, np.int32), lower=0, upper=1000)
    out = _raw(case)
    assert out[0] == E_ARG and "gene 1:" in out[1] and "2200 insertions" in out[1] and "2^31" in out[1] and _untouched(out)
    with pytest.raises(Exception) as e:
        _ctx().gene_cell_scores(*R.case_args(case))
    assert "gene 1:" in str(e.value)
    case["weight"] = np.ones(1001, np.int32)
    ptr, col, val, hits, arms = _ctx().gene_cell_scores(*R.case_args(case), with_hits=True, with_arm_rows=True)
    per_cell = 2 * np.bincount(cell, minlength=3)
    assert ptr.tolist() == [0, 0, 3] and col.tolist() == [0, 1, 2] and val.tolist() == per_cell.tolist() and hits.tolist() == [0, 2200] and arms.tolist() == [0, 1]
    # 2047 hits of weight 2^20 stay below the bound and do not wrap
    case["weight"] = np.full(1001, 1 << 20, np.int32)
    keep = np.r_[np.arange(1023), 1099]
    case.update(pos=pos[keep], tlen=np.r_[tlen[:1023], 8 + 2000], cell=np.zeros(1024, np.int32), upper=3000)     # the last record's right end lies beyond the window: one hit
    ptr, col, val, hits = _ctx().gene_cell_scores(*R.case_args(case), with_hits=True)
    assert hits.tolist() == [0, 2047] and col.tolist() == [0] and val.tolist() == [2047 << 20]


def test_determinism_permutation_and_split(monkeypatch):
    _force(monkeypatch)
    case, want = _case(200)
    a, b = _run(case), _run(case)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and _same(a[:4], want)
    perm = np.random.default_rng(1).permutation(120)
    shuffled = dict(case, **{k: case[k][perm] for k in ("win_lo", "win_hi", "body_lo", "body_hi")})
    got = _run(shuffled)
    assert np.array_equal(got[3], want[3][perm]) and got[4].tolist() == a[4].tolist()
    for j, g in enumerate(perm):
        assert np.array_equal(got[1][got[0][j]:got[0][j + 1]], want[1][want[0][g]:want[0][g + 1]])
        assert np.array_equal(got[2][got[0][j]:got[0][j + 1]], want[2][want[0][g]:want[0][g + 1]])
    halves = [_run(dict(case, **{k: case[k][s] for k in ("win_lo", "win_hi", "body_lo", "body_hi")})) for s in (slice(0, 47), slice(47, 120))]
    assert np.array_equal(np.concatenate([halves[0][0], halves[1][0][1:] + halves[0][0][-1]]), want[0])
    for k in (1, 2, 3):
        assert np.array_equal(np.concatenate([halves[0][k], halves[1][k]]), want[k])
    assert (halves[0][4] + halves[1][4]).tolist() == a[4].tolist()


# ---- the command, then `markers` on its matrix ----------------------------------------------------------------------------------------------
def test_command_end_to_end_names_the_planted_genes(tmp_path, monkeypatch):
    _force(monkeypatch)
    w, (ip, ix, da), found = R.planted_chain(tmp_path, None, None)
    assert found == {"g%d" % k: {"GENE%d" % i for i in w["sets"][k]} for k in range(3)}
    z = np.load(str(tmp_path / "planted.genescores.npz"))
    pos, tlen, cell = w["records"]["chrP"]
    want = R.gene_cell_scores(pos, tlen, cell, 90, z["window_start"], z["window_end"], z["body_start"], z["body_end"],
                              R.weight_table(100000, 5000, 256), 0, 1000, with_hits=True, with_arm_rows=True)
    assert np.array_equal(ip, want[0]) and np.array_equal(ix, want[1]) and np.array_equal(da, want[2]) and len(da) > 2000
    summary = dict(x.split("\t") for x in open(str(tmp_path / "planted.genescores.txt")).read().splitlines())
    assert summary["hits"] == str(want[3].sum()) and [summary["rows_short"], summary["rows_table"]] == [str(v) for v in want[4]] and want[4][1] == 30
