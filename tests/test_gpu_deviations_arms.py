"""Every geometry-selected arm of natac_motif_deviations (dev_motif_tiles<unsigned> / <unsigned long long>, csrc/natac_deviations.hpp)
and natac_window_base_counts past its grid cap, each pinned through the library's own launch plan.

The entry picks, per call: the cell tile (NATAC_DEVIATIONS_CELL_TILE, else 4096 halved down to 256 while motifs x tiles is below twice
the compute units, then evened out to a multiple of 64), `lanes` = the smallest power of two with lanes * m * n_tiles >= nnz (at most 64)
and 64-bit counters when max_set * max_count >= 2^32.  test_plan_is_the_rule (CPU) restates that rule and compares it field by field
with natac_motif_deviations_plan; every GPU test first asks the plan which arm its operands select and asserts that this is the arm it
was written for, so a later change to the rule cannot quietly move a test to another arm.

What the cases reach that tests/test_gpu_deviations.py does not: lane groups of 2 and 4 (and every group in both counter widths);
motifs of more than 1024 windows, where a wave takes a second trip of the `base` loop and waves 5 .. 15 work, in both widths; a 32-bit
counter in [2^31, 2^32) and the switch at exactly 2^32; row_ptr[0] > 0; the statistics at B = 1024; the 64-bit arm at a tile of 4096
(98,432 bytes of LDS); a wave of dev_window_base_count that takes a second range.

Bounds: those of tests/test_gpu_deviations.py (its _check): O and E equal; with u = 2^-53 and s = 1 + max_b |Y_b| per element,
|raw - ref| <= 8 u (1 + |ref|), |bg_mean - ref| <= 2 (B + 8) u s, |bg_m2 - ref| <= 2 (B + 8) u B s^2."""
import ctypes as C

import numpy as np
import pytest

import deviations_ref as R
from test_gpu_deviations import _check

gpu = pytest.mark.gpu       # every test but the CPU check of the plan

_REF = {}
LADDER = {1: 0.002, 2: 0.75 * 2 / 64, 4: 0.75 * 4 / 64, 8: 0.75 * 8 / 64, 16: 0.75 * 16 / 64, 32: 0.75 * 32 / 64, 64: 0.75}   # lanes: density
LONG = [1023, 1024, 1025, 1087, 1088, 1089, 2048, 2049, 2200]    # a wave's second trip starts empty, with one window, full


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _case(seed, **kw):
    """a make_arm_case() case and its reference, computed once and shared"""
    key = (seed,) + tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in sorted(kw.items()))
    if key not in _REF:
        case = R.make_arm_case(seed, **kw)
        _REF[key] = (case, R.reference_of(case))
    return _REF[key]


def _plan(case, n_cu=256):
    """the library's plan for a case's operands, under the environment's tile"""
    from nucleoatac_amd.device import motif_deviations_plan
    ip, ix, da = case["csr"]
    P, N = case["X"].shape
    return motif_deviations_plan(P, N, len(da), len(case["sets"]), max(len(s) for s in case["sets"]), int(da.max()), n_cu)


def _call(case, **kw):
    ip, ix, da = case["csr"]
    hp, hx = case["hits"]
    return _ctx().motif_deviations(ip, ix, da, case["X"].shape[1], hp, hx, len(case["sets"]), case["bg"], **kw)


def _raw_call(case, ip, ix, da):
    """natac_motif_deviations itself on the given CSR arrays: (rc, (raw, mean, m2, O, E))"""
    ctx = _ctx()
    N, M, B = case["X"].shape[1], len(case["sets"]), case["bg"].shape[0]
    mp = np.concatenate(([0], np.cumsum([len(s) for s in case["sets"]]))).astype(np.int64)
    mw = np.concatenate(case["sets"]).astype(np.int32)
    outs = [np.full((M, N), -7.0) for _ in range(3)] + [np.full((B + 1, M, N), -7, np.int64), np.full((B + 1, M), -7, np.int64)]
    rc = ctx._lib.natac_motif_deviations(ctx._h, len(ip) - 1, N, _vp(ip), _vp(ix), _vp(da), M, _vp(mp), _vp(mw), B,
                                         _vp(np.ascontiguousarray(case["bg"], np.int32)), *[_vp(o) for o in outs], None)
    return rc, tuple(outs)


# ---- the plan, without a GPU ---------------------------------------------------------------------------------------------------------------
def _rule(m, n, nnz, M, max_set, max_count, n_cu, env):
    """the entry's rule, restated: (tile, n_tiles, lanes, wide, lds_bytes); env: the value of NATAC_DEVIATIONS_CELL_TILE or None"""
    if env is not None and 1 <= env <= 4096:
        tile = env
    else:
        tile = 4096
        while tile > 256 and M * -(-n // tile) < 2 * n_cu:
            tile //= 2
        n_tiles = -(-n // tile)
        tile = min(tile, (-(-n // n_tiles) + 63) // 64 * 64)
        assert tile % 64 == 0 and 64 <= tile <= 4096
    n_tiles = -(-n // tile)
    assert n_tiles * tile >= n > (n_tiles - 1) * tile
    lanes = 1
    while lanes < 64 and lanes * m * n_tiles < nnz:
        lanes *= 2
    wide = max_set * max_count >= 1 << 32
    return dict(tile=tile, n_tiles=n_tiles, lanes=lanes, wide=wide, lds_bytes=tile * (16 + (8 if wide else 4)) + 128)


def test_plan_is_the_rule(monkeypatch):
    """CPU: natac_motif_deviations_plan == the rule written out above, field by field, over cell counts around every tile border, motif
    counts and compute units on both sides of the halving, nnz at and one past every lane group's limit, max_set * max_count around
    2^32, and the environment's tile valid, invalid and absent"""
    from nucleoatac_amd import _lib as L
    from nucleoatac_amd.device import motif_deviations_plan
    ns, n = [], 1
    while n <= 9000:
        ns.append(n)
        n += 1 + (n * 7 + n // 3) % 291
    ns = sorted(set(ns + [63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 9000]))
    assert len(ns) > 60
    seen = dict(tile=set(), lanes=set(), wide=set())
    n_plans = 0
    for env in (None, 1, 37, 64, 4096, 0, 4097):
        if env is None:
            monkeypatch.delenv("NATAC_DEVIATIONS_CELL_TILE", raising=False)
        else:
            monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", str(env))
        for i, n in enumerate(ns):
            m = (1, 7, 1100, 100003)[i % 4]
            for M in (1, 2, 7, 500, 5000):
                for n_cu in (1, 64, 256):
                    n_tiles = _rule(m, n, 1, M, 1, 1, n_cu, env)["n_tiles"]
                    cases = [(nnz, 3, 5) for lanes in (1, 2, 4, 8, 16, 32, 64) for nnz in (lanes * m * n_tiles, lanes * m * n_tiles + 1)]
                    cases += [(m * n_tiles * 3, a, b) for a, b in ((65537, 65535), (65536, 65536), (641, 6700417))]   # 2^32 - 1, 2^32, 2^32 + 1
                    for nnz, max_set, max_count in cases:
                        want = _rule(m, n, nnz, M, max_set, max_count, n_cu, env)
                        got = motif_deviations_plan(m, n, nnz, M, max_set, max_count, n_cu)
                        assert got == want, (env, m, n, nnz, M, max_set, max_count, n_cu)
                        for k in seen:
                            seen[k].add(got[k])
                        n_plans += 1
    assert seen["lanes"] == {1, 2, 4, 8, 16, 32, 64} and seen["wide"] == {False, True}
    assert {1, 37, 64, 128, 192, 256, 512, 1024, 2048, 4096} <= seen["tile"]
    print("%d plans compared" % n_plans)
    # 2^32 - 1, 2^32 and 2^32 + 1 as products
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "64")
    assert 65537 * 65535 == (1 << 32) - 1 and 641 * 6700417 == (1 << 32) + 1
    assert [motif_deviations_plan(70000, 65, 70000, 3, a, b)["wide"] for a, b in ((65537, 65535), (65536, 65536), (641, 6700417))] == \
        [False, True, True]
    assert motif_deviations_plan(300, 65, 5000, 2, 4, (1 << 30) - 1)["lds_bytes"] == 64 * 20 + 128
    assert motif_deviations_plan(300, 65, 5000, 2, 4, 1 << 30)["lds_bytes"] == 64 * 24 + 128
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "4096")
    assert motif_deviations_plan(300, 200, 5000, 5, 300, 1 << 30)["lds_bytes"] == 98432
    # refusals: sizes below 1, and the shapes the call refuses as too many for one call -- with plain integers, nothing is allocated
    good = [300, 65, 5000, 2, 4, 7, 256]
    for k in range(7):
        for v in (0, -1):
            with pytest.raises(L.NatacError):
                motif_deviations_plan(*(good[:k] + [v] + good[k + 1:]))
    big = (1 << 31) - 1
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "1")
    assert motif_deviations_plan(big, 3, big, 1, 1, 1)["n_tiles"] == 3                      # m * (n_tiles + 1) = 2^33 - 4
    assert motif_deviations_plan(1 << 30, 7, big, 1, 1, 1)["n_tiles"] == 7                  # exactly 2^33
    assert motif_deviations_plan(5, 1, 5, big, 1, 1)["n_tiles"] == 1                        # motifs x tiles = 2^31 - 1
    for args in ((big, 4, big, 1, 1, 1), ((1 << 30) + 1, 7, big, 1, 1, 1), (5, 2, 5, big, 1, 1), (5, 3, 5, 1 << 30, 1, 1)):
        with pytest.raises(L.NatacError) as err:
            motif_deviations_plan(*args)
        assert "too many for one call" in str(err.value)
    monkeypatch.delenv("NATAC_DEVIATIONS_CELL_TILE")
    assert motif_deviations_plan(big, 3 * 4096, big, 5000, 1, 1)["n_tiles"] == 3
    with pytest.raises(L.NatacError):
        motif_deviations_plan(big, 3 * 4096 + 1, big, 5000, 1, 1)
    with pytest.raises(L.NatacError):
        motif_deviations_plan(1 << 31, 65, 1 << 31, 2, 4, 7)


# ---- every lane group, both counter widths ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("lanes", [1, 2, 4, 8, 16, 32, 64])
def test_every_lane_group(lanes, wide, monkeypatch):
    """1100 windows x 130 cells in tiles of 64 (the last of 2 cells), 1 % of the windows full: pieces of 64 entries next to empty ones;
    motifs of 1, 63, 64, 65 and 1100 windows.  wide: one count near 2^30 makes 1100 x max_count pass 2^32"""
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "64")
    case, ref = _case(5000 + lanes, P=1100, N=130, B=3, sizes=[1, 63, 64, 65, 1100], density=LADDER[lanes],
                      planted=(1 << 30) - 77 - lanes if wide else None)
    plan = _plan(case)
    assert plan == dict(tile=64, n_tiles=3, lanes=lanes, wide=wide, lds_bytes=64 * (24 if wide else 20) + 128)
    assert np.diff(case["csr"][0]).max() == 130 and int(case["X"].sum()) < 1 << 31
    _check(_call(case, with_sums=True), ref, 3)
    if lanes == 64:                                         # one tile: a piece of 130 entries, longer than a wave
        monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "4096")
        plan = _plan(case)
        assert (plan["tile"], plan["n_tiles"], plan["lanes"], plan["wide"]) == (4096, 1, 64, wide)
        _check(_call(case, with_sums=True), ref, 3)


# ---- motifs of more than 1024 windows -----------------------------------------------------------------------------------------------------
def _long_case(wide):
    return _case(6000, P=2200, N=130, B=3, sizes=LONG, density=LADDER[16], planted=(1 << 30) - 5 if wide else None)


@gpu
@pytest.mark.parametrize("wide", [False, True])
def test_long_motifs(wide, monkeypatch):
    """a workgroup's 16 waves cover 1024 windows a trip: motifs that end one short of, at and one past a trip, and inside the second trip
    one short of, at and one past its first wave; every wave works and the waves' sums of rs meet in LDS"""
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "64")
    case, ref = _long_case(wide)
    assert _plan(case) == dict(tile=64, n_tiles=3, lanes=16, wide=wide, lds_bytes=64 * (24 if wide else 20) + 128)
    _check(_call(case, with_sums=True), ref, 3)


@gpu
def test_long_motifs_same_bytes_under_every_tile(monkeypatch):
    """the 32-bit arm at 2200 windows: tiles of 64, 1, 37 cells and the default give the same bytes"""
    case, ref = _long_case(False)
    n_cu = _ctx().device_info()["n_cu"]
    outs, plans = [], []
    for tile in ("64", "1", "37", None):
        if tile is None:
            monkeypatch.delenv("NATAC_DEVIATIONS_CELL_TILE", raising=False)
        else:
            monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", tile)
        plans.append(_plan(case, n_cu))
        assert not plans[-1]["wide"]
        outs.append(_call(case, with_sums=True))
    assert [p["tile"] for p in plans[:3]] == [64, 1, 37] and plans[3]["tile"] % 64 == 0 and plans[3]["tile"] > 64
    assert [p["lanes"] for p in plans[:3]] == [16, 1, 8]
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert a.tobytes() == b.tobytes()
    _check(outs[0], ref, 3)


# ---- a 32-bit counter above 2^31, and the switch at 2^32 ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B", [2, 7])
@pytest.mark.parametrize("planted,wide", [((1 << 30) - 1, False), (1 << 30, True)])
def test_counter_up_to_two_to_the_32(planted, wide, B, monkeypatch):
    """set 1 maps every window to the window of the one large entry: motifs of 3 and 4 windows take that cell's counter to 3 and 4 times
    the entry -- 3 (2^30 - 1) and 2^32 - 4 in 32 bits, and with an entry of 2^30 the product reaches 2^32 and the counters are 64-bit"""
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "64")
    case, ref = _case(7000 + B, P=300, N=65, B=B, sizes=[3, 4], density=0.05, planted=planted, to_planted=True)
    plan = _plan(case)
    assert (plan["tile"], plan["n_tiles"], plan["wide"]) == (64, 2, wide)
    O = ref[0]
    assert O.max() == 4 * planted == O[1, 1, case["heavy_cell"]] and O[1, 0, case["heavy_cell"]] == 3 * planted >= 1 << 31
    assert O.max() == ((1 << 32) if wide else (1 << 32) - 4)
    got = _call(case, with_sums=True)
    assert got[3].max() == O.max()
    _check(got, ref, B)


# ---- row_ptr[0] > 0 ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wide", [False, True])
def test_row_ptr_from_an_offset(wide, monkeypatch):
    """five entries before row_ptr[0], with columns out of range and counts below 1: never read, and the outputs are the bytes of the
    call without them"""
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "64")
    case, ref = _case(5004, P=1100, N=130, B=3, sizes=[1, 63, 64, 65, 1100], density=LADDER[4], planted=(1 << 30) - 81 if wide else None)
    assert (_plan(case)["lanes"], _plan(case)["wide"]) == (4, wide)
    ip, ix, da = case["csr"]
    rc, plain = _raw_call(case, ip, ix, da)
    assert rc == 0
    junk_col, junk_cnt = np.array([-1, 130, 1 << 30, -(1 << 31), 64], np.int32), np.array([-5, 0, -(1 << 31), -1, -9], np.int32)
    rc, shifted = _raw_call(case, ip + 5, np.concatenate((junk_col, ix)), np.concatenate((junk_cnt, da)))
    assert rc == 0
    for a, b in zip(shifted, plain):
        assert a.tobytes() == b.tobytes()
    _check(shifted, ref, 3)


# ---- B = 1024 ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_statistics_at_the_most_background_sets(monkeypatch):
    monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", "64")
    case, ref = _case(8000, P=150, N=65, B=1024, sizes=[40, 150], density=0.1)
    plan = _plan(case)
    assert (plan["tile"], plan["n_tiles"], plan["wide"]) == (64, 2, False)
    _check(_call(case, with_sums=True), ref, 1024)


# ---- the 64-bit arm at a tile of 4096 ------------------------------------------------------------------------------------------------------
@gpu
def test_wide_arm_at_the_largest_tile(monkeypatch):
    """98,432 bytes of dynamic LDS: past the 64 KiB a kernel gets without asking"""
    case = R.make_case(3100, P=300, N=200, M=5, B=7, big=True)
    ref = R.reference_of(case)
    outs = []
    for tile, lds in (("4096", 98432), ("64", 64 * 24 + 128)):
        monkeypatch.setenv("NATAC_DEVIATIONS_CELL_TILE", tile)
        plan = _plan(case)
        assert (plan["tile"], plan["wide"], plan["lds_bytes"]) == (int(tile), True, lds)
        outs.append(_call(case, with_sums=True))
    _check(outs[0], ref, 7)
    for a, b in zip(outs[0], outs[1]):
        assert a.tobytes() == b.tobytes()


# ---- base counts past the grid cap ---------------------------------------------------------------------------------------------------------
@gpu
def test_window_base_counts_past_the_grid_cap():
    """70,000 ranges: the grid stops at 16,384 workgroups of 4 waves, so the first 4,464 waves take a second range"""
    rng = np.random.default_rng(9)
    seq = rng.choice(np.frombuffer(b"ACGTacgtNnRX-", np.uint8), 5000)
    length = rng.integers(0, 71, 70000)
    length[:8] = [0, 63, 64, 65, 70, 0, 1, 64]
    length[65536:65540] = [65, 0, 64, 63]                                                # the first ranges of a second trip
    starts = rng.integers(0, 5000 - 70, 70000)
    starts[0], starts[6] = 0, 4999
    ends = starts + length
    assert ends.max() <= 5000 and set(length.tolist()) == set(range(71))
    want = R.base_counts(seq, starts, ends)
    got = _ctx().base_counts(seq, starts, ends, per_range=True)
    assert got.dtype == np.int64 and got.shape == (70000, 4) and np.array_equal(got, want)
    assert want[0].tolist() == [0, 0, 0, 0] and want[65536:].sum() > 0
    assert np.array_equal(_ctx().base_counts(seq, starts, ends), want.sum(axis=0))
