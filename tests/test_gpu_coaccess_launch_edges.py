"""natac_window_pair_sums (csrc/natac_coaccess.hpp) where tests/test_gpu_coaccess.py does not reach: the second trip of ca_table's and
ca_search's grid-stride loops -- the table's zeros go back at the owner's columns only, the search arm overwrites the owner's chunk -- and
the table's last size, 16,384 cells in exactly 64 KiB of LDS, beside the first size of the search arm and one in the untested middle.
Both arrays are compared for equality with the restatement of tests/coaccess_ref.py; arm_owners is asserted everywhere.

The stride case is sized from the grid that natac_window_pair_sums_plan reports for the device's own CU count, and the test asserts that
the owners with a partner exceed it by 500.  Every seventh owner has no partner (the workgroup-uniform `continue`), and at six places
owner i + grid follows owner i with planted rows: every cell followed by the empty row and by one entry, and the reverse
(coaccess_ref.stride_case).  tests/test_coaccess_host.py checks the sizing for 256 and 304 CUs without a GPU."""
import numpy as np
import pytest

import coaccess_ref as R

pytestmark = pytest.mark.gpu

_REF = {}


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _n_cu():
    return _ctx().device_info()["n_cu"]


def _force(monkeypatch, table_max=None, chunk=None):
    for name, v in (("NATAC_COACCESS_TABLE_MAX", table_max), ("NATAC_COACCESS_CHUNK", chunk)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def _plan(case):
    """the plan of the case on this device, under the environment as it stands"""
    from nucleoatac_amd.device import window_pair_sums_plan
    L = np.diff(case["indptr"])
    return window_pair_sums_plan(len(L), case["N"], int(L.sum()), len(case["order"]), int(L[case["order"]].sum()), n_cu=_n_cu())


def _shared(key, make):
    """a case and its reference, computed once and shared"""
    if key not in _REF:
        made = make()
        case = made[0] if isinstance(made, tuple) else made
        _REF[key] = (made, R.pair_sums_sparse(case["indptr"], case["indices"], case["data"], case["N"], case["order"], case["hi"]))
    return _REF[key]


def _with_partners(case):
    return int((case["hi"] - np.arange(len(case["hi"])) > 1).sum())


def _check(case, ref, arm):
    sxy, both, arms = _ctx().window_pair_sums(case["indptr"], case["indices"], case["data"], case["N"], case["order"], case["hi"], with_arm_owners=True)
    for name, a, b in (("sxy", sxy, ref[0]), ("both", both, ref[1])):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        bad = np.flatnonzero(a != b)
        assert len(bad) == 0, "%s in the %s arm: %d of %d differ, the first at %d: %d against %d" % (name, arm, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]])
    assert arms.tolist() == ([_with_partners(case), 0] if arm == "table" else [0, _with_partners(case)]), arm
    return sxy, both


# ---- both arms' second trip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm,table_max,chunk", [("table", None, None), ("search", 1, None), ("search", 1, 16)])
def test_second_trip(arm, table_max, chunk, monkeypatch):
    from nucleoatac_amd.device import window_pair_sums_plan
    _force(monkeypatch, table_max=table_max, chunk=chunk)
    grid = window_pair_sums_plan(1 << 20, 64, 8 << 20, 1 << 20, 8 << 20, n_cu=_n_cu())["grid"]          # the most workgroups of this device
    (case, planted), ref = _shared(("stride", grid), lambda: R.stride_case(17, grid))
    p = _plan(case)
    k, L = len(case["order"]), np.diff(case["indptr"])
    has = case["hi"] - np.arange(k) > 1
    assert (p["arm"], p["grid"], p["lanes"], p["chunk"]) == (arm, grid, 16, chunk or 8192)
    assert has.sum() > p["grid"] + 500 and (has[grid:] & has[:k - grid]).sum() > 500                   # owners with partners, trip after trip
    assert (~has[grid:]).sum() >= 100 and (~has[:grid]).sum() >= 100 and len(ref[0]) > 3 * grid
    # what is planted: (the row of owner i, the row of owner i + grid), each with partners
    assert [(a, b) for _, a, b in planted] == list(R.STRIDE_PLANTS) and L[[0, 1, 2, 5, 6]].tolist() == [0, 1, 64, 32, 32] and 16 < L[3] < 32
    for i, a, b in planted:
        assert case["order"][i] == a and case["order"][i + grid] == b and has[i] and has[i + grid] and i + grid < k
    if chunk:                                                          # owners of more than one chunk on either trip
        own = L[case["order"]] * has
        assert (own[:grid] > chunk).sum() >= 5 and (own[grid:] > chunk).sum() >= 3
    _check(case, ref, arm)


# ---- the table's last size -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,arm,lds", [(16384, "table", 65536), (16385, "search", 65536), (5000, "table", 20000)])
def test_table_sizes(n, arm, lds, monkeypatch):
    _force(monkeypatch)
    case, ref = _shared(("size", n), lambda: R.make_case(n, 40, n, 3000, partners=6))
    p = _plan(case)
    assert (p["arm"], p["lds_bytes"], p["table_max"], p["chunk"], p["lanes"]) == (arm, lds, 16384, 8192, 64)
    L = np.diff(case["indptr"])
    ip, ix = case["indptr"], case["indices"]
    last = [w for w in range(40) if L[w] and ix[ip[w + 1] - 1] == n - 1]
    assert L[2] == n and 2 in last and len(last) >= 3                  # rows that hold the last cell: the row with every cell and others
    assert np.array_equal(ix[ip[3]:ip[4]], ix[ip[4]:ip[5]]) and not set(ix[ip[5]:ip[6]].tolist()) & set(ix[ip[6]:ip[7]].tolist())
    owners = case["order"][case["hi"] - np.arange(len(case["hi"])) > 1]
    assert set(range(7)) <= set(owners.tolist()) and set(last) <= set(case["order"].tolist()) and L.max() == n and L[7:].max() > 4096
    _check(case, ref, arm)
