"""natac_group_rank_sums (csrc/natac_markers.hpp) where tests/test_gpu_markers.py does not reach: the second trip of mk_short's and
mk_block's grid-stride loops, the default thresholds with the block arm's LDS past 64 KiB, and the widest integers at 2^20 cells.  All
four arrays are compared for equality with the exact restatement of tests/markers_ref.py; arm_rows is asserted everywhere.

A stride case is sized from the grid that natac_group_rank_sums_plan reports for the device's own CU count, and the test asserts that the
rows exceed a trip of that grid by 500 (short arm) or 300 (block arm).  A workgroup's second row follows a longer one of other cells and
groups; two of three are empty or hold one entry (short arm) or the fewest the arm takes (block arm), so counters that were not cleared
would be counted (markers_ref.short_stride_case / block_stride_case).  tests/test_markers_host.py checks the sizing for 256 and 304 CUs
without a GPU."""
import numpy as np
import pytest

import markers_ref as R

pytestmark = pytest.mark.gpu

_REF = {}
NAMES = ("detected", "total", "rank2", "ties")
ENV = ("NATAC_MARKERS_SHORT_MAX", "NATAC_MARKERS_BLOCK_MAX")


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _n_cu():
    return _ctx().device_info()["n_cu"]


def _force(monkeypatch, short_max=None, block_max=None):
    for name, v in zip(ENV, (short_max, block_max)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _plan(case):
    """the plan of the case on this device, under the environment as it stands"""
    from nucleoatac_amd.device import group_rank_sums_plan
    L = np.diff(case["indptr"])
    return group_rank_sums_plan(len(L), case["N"], int(L.sum()), int(L.max()), case["G"], n_cu=_n_cu())


def _most(N, longest, G):
    """the plan of 2^20 rows: the most workgroups this device is given"""
    from nucleoatac_amd.device import group_rank_sums_plan
    return group_rank_sums_plan(1 << 20, N, longest << 20, longest, G, n_cu=_n_cu())


def _shared(key, make):
    """a case and its reference, computed once and shared"""
    if key not in _REF:
        made = make()
        case = made[0] if isinstance(made, tuple) else made
        ref = R.rank_sums(case["indptr"], case["indices"], case["data"], case["N"], case["depth"], case["group"], case["G"])
        _REF[key] = (made, ref)
    return _REF[key]


def _check(case, ref, arms, what=""):
    got = _ctx().group_rank_sums(case["indptr"], case["indices"], case["data"], case["N"], case["depth"], case["group"], case["G"], with_arm_rows=True)
    for name, a, b in zip(NAMES, got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = np.argwhere(a != b)
        assert len(bad) == 0, "%s %s: %d differ, the first at %s: %d against %d" % (name, what, len(bad), bad[0], a[tuple(bad[0])], b[tuple(bad[0])])
    assert got[4].tolist() == arms, what
    return got


def _arms_of(case, short_max, block_max):
    L = np.diff(case["indptr"])
    return [int((L <= short_max).sum()), int(((L > short_max) & (L <= block_max)).sum()), int((L > max(short_max, block_max)).sum())]


# ---- the short arm's second trip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short_max,lanes,lead", [(None, 64, 40), (16, 16, None)])
def test_short_arm_second_trip(short_max, lanes, lead, monkeypatch):
    _force(monkeypatch, short_max=short_max)
    slots = 256 // lanes
    cap = _most(48, lead or 8, 5)
    assert cap["lanes"] == lanes
    per_trip = slots * cap["grid"]["short"]
    case, ref = _shared(("short", lanes, per_trip), lambda: R.short_stride_case(40 + lanes, per_trip + 501, per_trip, lead=lead))
    p = _plan(case)
    L = np.diff(case["indptr"])
    assert p["lanes"] == lanes and len(L) > slots * p["grid"]["short"] + 500                    # 501 lane groups serve a second row
    second = np.arange(per_trip, len(L))
    assert (L[second - per_trip] == 8).sum() >= 300 and (L[second] == 0).sum() >= 150 and (L[second] == 1).sum() >= 150 and (L[second] > 1).sum() >= 80
    assert L.max() == (lead or 8) and len(np.unique(case["group"])) == 5
    _check(case, ref, [len(L), 0, 0], "with %d lanes a row" % lanes)
    # the rows of the second trip are not all alike: an empty one has ties of N^3 - N, the others less
    assert len(np.unique(ref[3][second])) >= 5 and (ref[0][second].sum(axis=1) == L[second]).all()


# ---- the block arm's second trip ---------------------------------------------------------------------------------------------------------
def test_block_arm_second_trip(monkeypatch):
    _force(monkeypatch, short_max=4)
    grid = _most(48, 40, 5)["grid"]["block"]
    (case, where), ref = _shared(("block", grid), lambda: R.block_stride_case(77, grid + 301, grid))
    p = _plan(case)
    L = np.diff(case["indptr"])
    arms = _arms_of(case, 4, 8192)
    assert p["short_max"] == 4 and p["grid"]["block"] == grid and arms[1] == len(where) > p["grid"]["block"] + 300 and arms[2] == 0
    assert (L[where] > 4).all() and arms[0] >= 500 and sorted(set(L[L <= 4].tolist())) == [0, 1, 2, 3, 4]
    first, second = L[where[:len(where) - grid]], L[where[grid:]]
    assert len(second) == 301 and (first == 40).sum() >= 200 and (second <= 6).sum() >= 200 and (first != second).sum() >= 250
    _check(case, ref, arms, "under NATAC_MARKERS_SHORT_MAX=4")


# ---- the default thresholds ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 255])
def test_default_thresholds_at_nine_thousand_cells(G, monkeypatch):
    case, ref = _shared(("border", G), lambda: R.border_case(900 + G, G))
    L = np.diff(case["indptr"])
    assert L.tolist() == list(R.BORDER_ROWS) + [8500, 8700] and case["N"] == 9000
    # row 9: one tie group of 8500 entries; row 10: the colliding pair is no tie
    (a0, d0), (a1, d1) = R.COLLIDING
    assert ref[3][9] == 500 ** 3 - 500 + 8500 ** 3 - 8500 and a0 / d0 == a1 / d1 and a0 * d1 != a1 * d0
    e = case["indptr"][10]
    assert case["indices"][e:e + 2].tolist() == [0, 1] and case["data"][e:e + 2].tolist() == [a0, a1] and case["depth"][:2].tolist() == [d0, d1]
    _force(monkeypatch)
    p = _plan(case)
    assert (p["short_max"], p["block_max"], p["chunk"]) == (64, 8192, 4096) and p["lds_bytes"]["block"] > 65536       # block_cap 8192
    assert p["lds_bytes"]["block"] == (G * 20 + 15) // 16 * 16 + 16 + 8192 * 9
    whole = _check(case, ref, [3, 4, 4], "at the defaults")
    _force(monkeypatch, block_max=4096)
    p = _plan(case)
    assert (p["block_max"], p["chunk"]) == (4096, 4096) and p["lds_bytes"]["block"] == (G * 20 + 15) // 16 * 16 + 16 + 4096 * 9       # block_cap 4096
    got = _check(case, ref, [3, 2, 6], "under NATAC_MARKERS_BLOCK_MAX=4096")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(whole[:4], got[:4]))


# ---- the widest integers ---------------------------------------------------------------------------------------------------------------------
def test_two_to_the_twenty_cells(monkeypatch):
    N = 1 << 20
    case, ref = _shared("big", lambda: R.big_case(31))
    L = np.diff(case["indptr"])
    assert case["N"] == N == 1048576 and L.tolist() == [0, 1, 1, 10000, 5000, 40] and case["indices"][0] == N - 1 and case["indices"][1] == 0
    assert case["indices"][case["indptr"][4] - 1] == N - 1                                     # the long row reaches the last cell
    n_g = np.bincount(case["group"], minlength=3)
    assert int(ref[3][0]) == 1152921504605798400 == 2 ** 60 - 2 ** 20                          # the empty row: z0^3 - z0 with z0 = 2^20
    assert ref[2][0].tolist() == [int(n) * 1048577 for n in n_g] and ref[3][1] == (N - 1) ** 3 - (N - 1)
    _force(monkeypatch)
    p = _plan(case)
    assert p["lds_bytes"]["block"] > 65536 and p["lds_bytes"]["long"] == 4096 * 8
    got = _check(case, ref, [4, 1, 1], "at 2^20 cells")
    assert int(got[3][0]) == 1152921504605798400 and got[2][0].tolist() == [int(n) * 1048577 for n in n_g]
