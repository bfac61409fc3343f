"""natac_knn (csrc/natac_knn.hpp) on the GPU against the NumPy restatement of tests/knn_ref.py: shapes around the wave width and the tiles,
both arms, ties, separate queries, adversarial orders, forced tiles, a grid stride, blocks of queries, extreme magnitudes, every refusal
and determinism.  idx is compared for equality and dist2 bit for bit: the rule is exact.  arm_queries is asserted everywhere, so the arm
under test ran."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_ref as R

pytestmark = pytest.mark.gpu

ENV = ("NATAC_KNN_WAVE_K_MAX", "NATAC_KNN_QUERY_TILE", "NATAC_KNN_REF_TILE")
E_ARG = -1


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _force(monkeypatch, wave_k_max=None, query_tile=None, ref_tile=None):
    for name, v in zip(ENV, (wave_k_max, query_tile, ref_tile)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


@functools.lru_cache(maxsize=None)
def _case(nr, dim, k, seed=0):
    """points and their restatement, formed once"""
    x = R.gauss(nr, dim, seed=seed + 1000 * nr + dim)
    want = R.knn(x, k)
    for a in (x,) + want:
        a.setflags(write=False)
    return x, want


def _run(x, k, arm, **kw):
    """Context.knn with the arm asserted: all queries took `arm`"""
    got = _ctx().knn(x, k, with_arm_queries=True, **kw)
    nq = len(kw["queries"]) if kw.get("queries") is not None else len(x)
    assert got[2].tolist() == ([nq, 0] if arm == "wave" else [0, nq]) and got[0].dtype == np.int32 and got[1].dtype == np.float64
    return got[:2]


SHAPES = ((1, 1, 1), (2, 2, 5), (63, 7, 64), (64, 30, 65), (65, 64, 200), (257, 2, 1024), (257, 7, 1), (1000, 30, 5), (1000, 64, 64),
          (1000, 7, 200), (1000, 1, 1024))


@pytest.mark.parametrize("nr,dim,k", SHAPES)
def test_shapes_under_the_default_plan(nr, dim, k, monkeypatch):
    _force(monkeypatch)
    x, want = _case(nr, dim, k)
    assert R.same(_run(x, k, "wave" if k <= 64 else "lds"), want)
    if k > nr - 1:
        assert np.all(want[0][:, nr - 1:] == -1) and np.all(np.isinf(want[1][:, nr - 1:]))


@pytest.mark.parametrize("nr,dim,k", [s for s in SHAPES if 1 < s[2] <= 64])
def test_small_k_through_the_lds_arm(nr, dim, k, monkeypatch):
    _force(monkeypatch, wave_k_max=1)
    x, want = _case(nr, dim, k)
    assert R.same(_run(x, k, "lds"), want)


@pytest.mark.parametrize("arm", ("wave", "lds"))
def test_ties_go_to_the_lower_index(arm, monkeypatch):
    _force(monkeypatch, wave_k_max=1 if arm == "lds" else None)
    lat = R.lattice(16)
    for k in (3, 6, 11):                        # 4 neighbours at distance 1, 4 at 2, 4 at 4: every k cuts through a group
        assert R.same(_run(lat, k, arm), R.knn(lat, k))
    twice = np.concatenate([R.gauss(150, 3, seed=4)] * 2)
    got = _run(twice, 7, arm)
    assert R.same(got, R.knn(twice, 7)) and np.all(got[1][:, 0] == 0.0) and np.array_equal(got[0][:150, 0], np.arange(150, 300))
    equal = np.full((130, 5), 0.25)
    got = _run(equal, 40, arm)
    assert R.same(got, R.knn(equal, 40)) and got[0][0].tolist() == list(range(1, 41)) and got[0][129].tolist() == list(range(40))


def test_ties_in_a_long_list(monkeypatch):
    _force(monkeypatch)
    lat = R.lattice(16)
    assert R.same(_run(lat, 100, "lds"), R.knn(lat, 100))


@pytest.mark.parametrize("arm,k", (("wave", 9), ("lds", 9), ("lds", 70)))
def test_separate_queries(arm, k, monkeypatch):
    _force(monkeypatch, wave_k_max=1 if (arm == "lds" and k <= 64) else None)
    x = R.gauss(500, 7, seed=11)
    q = R.gauss(100, 7, seed=12)
    assert R.same(_run(x, k, arm, queries=q, self_offset=-1), R.knn(x, k, queries=q))
    assert R.same(_run(x, k, arm, queries=q), R.knn(x, k, queries=q))
    own = _run(x, k, arm, queries=x[300:400], self_offset=300)
    assert R.same(own, tuple(v[300:400] for v in R.knn(x, k)))
    kept = _run(x, k, arm, queries=x[300:400])                 # nothing excluded: every query finds itself first
    assert np.array_equal(kept[0][:, 0], np.arange(300, 400)) and R.same(kept, R.knn(x, k, queries=x[300:400]))


@pytest.mark.parametrize("arm,k", (("wave", 64), ("wave", 10), ("lds", 65), ("lds", 10)))
@pytest.mark.parametrize("farthest_first", (True, False))
def test_adversarial_orders(arm, k, farthest_first, monkeypatch):
    _force(monkeypatch, wave_k_max=1 if (arm == "lds" and k <= 64) else None)
    pts = R.gauss(700, 3, seed=21)
    q = np.zeros((1, 3))
    x = R.ordered_from(pts, q[0], farthest_first)
    want = R.knn(x, k, queries=q)
    assert want[0][0].tolist() == (list(range(699, 699 - k, -1)) if farthest_first else list(range(k)))
    assert R.same(_run(x, k, arm, queries=q), want)


@pytest.mark.parametrize("k", (5, 200))
def test_forced_tiles_give_the_bytes_of_the_default(k, monkeypatch):
    from nucleoatac_amd.device import knn_plan
    arm = "wave" if k <= 64 else "lds"
    x, want = _case(3 * 64 + 17, 7, k)
    _force(monkeypatch)
    assert R.same(_run(x, k, arm), want)
    for rt in (64, 128, 256):
        _force(monkeypatch, ref_tile=rt)
        assert knn_plan(len(x), len(x), 7, k)["ref_tile"] == rt and R.same(_run(x, k, arm), want)
    fits = (4, 8, 16, 32) if k <= 64 else (4, 8, 16)          # 32 queries of k = 200 would pass the LDS cap: that value is ignored
    for qt in fits:
        _force(monkeypatch, query_tile=qt)
        assert knn_plan(len(x), len(x), 7, k)["query_tile"] == qt and R.same(_run(x, k, arm), want)
    _force(monkeypatch, query_tile=32, ref_tile=64)
    assert knn_plan(len(x), len(x), 7, k)["query_tile"] == (32 if k <= 64 else 4) and R.same(_run(x, k, arm), want)


def test_more_query_tiles_than_workgroups(monkeypatch):
    """the grid is at most 8 workgroups a compute unit: with 4 queries a tile, nq above 4 x grid makes every workgroup stride"""
    from nucleoatac_amd.device import knn_plan
    _force(monkeypatch, query_tile=4)
    n_cu = _ctx().device_info()["n_cu"]
    nq = 4 * 8 * n_cu + 4 * n_cu + 3
    p = knn_plan(nq, 300, 2, 3, n_cu=n_cu)
    assert p["grid"] == 8 * n_cu and nq > p["grid"] * p["query_tile"]
    x = R.gauss(300, 2, seed=31)
    q = R.gauss(nq, 2, seed=32)
    assert R.same(_run(x, 3, "wave", queries=q), R.knn(x, 3, queries=q))


@pytest.mark.parametrize("k", (5, 70))
def test_blocks_of_queries_give_the_same_bytes(k, monkeypatch):
    _force(monkeypatch)
    x, want = _case(257, 7, k)
    arm = "wave" if k <= 64 else "lds"
    assert R.same(_run(x, k, arm, max_out=k * 100), want)              # 100 + 100 + 57 queries
    assert R.same(_run(x, k, arm, queries=x[50:250], self_offset=50, max_out=k * 70), tuple(v[50:250] for v in want))


@pytest.mark.parametrize("arm", ("wave", "lds"))
def test_magnitudes(arm, monkeypatch):
    _force(monkeypatch, wave_k_max=1 if arm == "lds" else None)
    for scale, zeros in ((1e-160, 0), (1e-162, 2000)):        # squares are subnormal, then mostly zero: ties go to the index
        tiny = R.gauss(200, 4, seed=41, scale=scale)
        want = R.knn(tiny, 12)
        assert want[1].max() < 1e-300 and np.count_nonzero(want[1] == 0.0) >= zeros and R.same(_run(tiny, 12, arm), want)
    huge = np.random.default_rng(42).choice([-1.0, -0.5, 0.0, 0.5, 1.0], (200, 64)) * 2.0 ** 500
    want = R.knn(huge, 12)
    assert np.all(np.isfinite(want[1])) and want[1].max() > 2.0 ** 1005 and R.same(_run(huge, 12, arm), want)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(q, x, k, self_offset=-1, dim=None, nq=None, nr=None):
    """the entry point itself with filled outputs -> (rc, message, the outputs are untouched)"""
    from nucleoatac_amd import _lib as L
    ctx = _ctx()
    nq = len(q) if nq is None else nq
    idx, d2 = np.full((max(nq, 1), max(k, 1)), 77, np.int32), np.full((max(nq, 1), max(k, 1)), 7.5)
    arms, ms = np.full(2, 77, np.int64), C.c_double(7.5)
    rc = ctx._lib.natac_knn(ctx._h, nq, len(x) if nr is None else nr, x.shape[1] if dim is None else dim, _vp(q), _vp(x), self_offset, k,
                            _vp(idx), _vp(d2), _vp(arms), C.byref(ms))
    return rc, ctx._lib.natac_last_error().decode(), bool(np.all(idx == 77) and np.all(d2 == 7.5) and np.all(arms == 77) and ms.value == 7.5)


def test_bad_values_are_refused_with_their_index(monkeypatch):
    _force(monkeypatch)
    x = np.ascontiguousarray(R.gauss(50, 3, seed=51))
    q = np.ascontiguousarray(R.gauss(10, 3, seed=52))
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 501, -(2.0 ** 501)):
        xb = x.copy()
        xb[40, 1] = bad
        xb[45, 0] = bad
        rc, msg, untouched = _raw(q, xb, 4)
        assert rc == E_ARG and msg.startswith("x[121] = ") and "2^500" in msg and untouched
        qb = q.copy()
        qb[7, 2] = bad
        rc, msg, untouched = _raw(qb, x, 4)
        assert rc == E_ARG and msg.startswith("q[23] = ") and untouched
    edge = x.copy()
    edge[3, 1] = 2.0 ** 500
    assert _raw(q, edge, 4)[0] == 0


def test_bad_sizes_are_refused(monkeypatch):
    _force(monkeypatch)
    x = np.ascontiguousarray(R.gauss(50, 3, seed=53))
    q = np.ascontiguousarray(x[:10])
    wide = np.zeros((4, 65))
    for kw, message in ((dict(q=wide, x=wide, k=1), "dim must be in [1, 64]"), (dict(q=q, x=x, k=0), "k must be in [1, 1024]"),
                        (dict(q=q, x=x, k=1025), "k must be in [1, 1024]"), (dict(q=q, x=x, k=3, self_offset=41), "self_offset must be -1 or in [0, nr - nq]"),
                        (dict(q=q, x=x, k=3, self_offset=-2), "self_offset must be -1 or in [0, nr - nq]"),
                        (dict(q=q, x=x, k=3, nr=0), "nr must be in [1, 16777216]"), (dict(q=q, x=x, k=3, nq=-1), "nq must be at least 0")):
        rc, msg, untouched = _raw(**kw)
        assert rc == E_ARG and message in msg and untouched
    assert _raw(q, x, 3, self_offset=40)[0] == 0 and _raw(q, x, 3, self_offset=0)[0] == 0
    # no queries: fine, and nothing is launched or written but the zeros of arm_queries and kernel_ms
    from nucleoatac_amd import _lib as L
    got = _ctx().knn(x, 3, queries=np.zeros((0, 3)), with_arm_queries=True, with_kernel_ms=True)
    assert got[0].shape == (0, 3) and got[2].tolist() == [0, 0] and got[3] == 0.0
    with pytest.raises(L.NatacError, match="dim must be in"):
        _ctx().knn(wide, 1)
    with pytest.raises(ValueError, match="k must be in"):
        _ctx().knn(x, 0)


def test_two_calls_give_the_same_bytes(monkeypatch):
    _force(monkeypatch)
    for k, arm in ((30, "wave"), (300, "lds")):
        x, want = _case(1000, 30, k, seed=9)
        a, b = _run(x, k, arm), _run(x, k, arm)
        assert R.same(a, b) and R.same(a, want)
