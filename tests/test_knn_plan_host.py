"""CPU: the launch plan of natac_knn (natac_knn_plan needs no GPU), its three environment overrides and its argument limits, and the NumPy
restatement of tests/knn_ref.py against a loop over Python floats."""
import numpy as np
import pytest

import knn_ref as R
from nucleoatac_amd import _lib as L
from nucleoatac_amd.device import knn_plan

ENV = ("NATAC_KNN_WAVE_K_MAX", "NATAC_KNN_QUERY_TILE", "NATAC_KNN_REF_TILE")


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


def test_the_arm_turns_at_64():
    a, b = knn_plan(1000, 1000, 30, 64), knn_plan(1000, 1000, 30, 65)
    assert (a["arm"], a["capacity"], a["wave_k_max"]) == ("wave", 64, 64)
    assert (b["arm"], b["capacity"]) == ("lds", 256 - 65)                    # the power of two >= k + 64, less the list
    assert knn_plan(1000, 1000, 30, 1024)["capacity"] == 1024 and knn_plan(1000, 1000, 30, 1)["arm"] == "wave"
    assert a["wg"] == b["wg"] == 256


def test_default_tiles_and_grid():
    # fewer query tiles than 4 n_cu (wave arm) or 8 n_cu (lds arm): a wave takes fewer queries, down to one; many queries: eight
    assert knn_plan(1000, 1000, 2, 5) == dict(arm="wave", wave_k_max=64, query_tile=4, ref_tile=256, capacity=64, wg=256,
                                              lds_bytes=8 * 2 * 257 + 8 * 4 * 2 + 12 * 4 * 65, grid=250)
    p = knn_plan(100000, 300000, 30, 64)
    assert (p["query_tile"], p["ref_tile"], p["grid"]) == (32, 64, 2048) and p["lds_bytes"] <= 80 * 1024
    assert knn_plan(100000, 300000, 30, 64, n_cu=8)["grid"] == 64
    assert knn_plan(100000, 1000, 64, 5)["ref_tile"] == 64 and knn_plan(100000, 1000, 11, 5)["ref_tile"] == 256
    # the selection arrays of a large k leave room for fewer queries
    assert knn_plan(100000, 300000, 30, 1024)["query_tile"] < 32
    assert knn_plan(0, 10, 3, 2)["grid"] == 1
    assert knn_plan(10000, 30000, 30, 64)["query_tile"] == 8 and knn_plan(10000, 30000, 30, 150)["query_tile"] == 4


def test_lds_stays_within_the_cap_at_the_largest_shape(monkeypatch):
    assert L.KNN_LDS_CAP == 160 * 1024
    p = knn_plan(200000, 1000000, 64, 1024)
    assert p["arm"] == "lds" and p["lds_bytes"] <= L.KNN_LDS_CAP
    for qt in (4, 8, 16, 32):
        for rt in (64, 128, 256):
            monkeypatch.setenv("NATAC_KNN_QUERY_TILE", str(qt))
            monkeypatch.setenv("NATAC_KNN_REF_TILE", str(rt))
            for dim, k in ((64, 1024), (64, 65), (30, 200), (1, 1)):
                assert knn_plan(200000, 1000000, dim, k)["lds_bytes"] <= L.KNN_LDS_CAP


def test_overrides_are_honoured_by_their_rules(monkeypatch):
    monkeypatch.setenv("NATAC_KNN_WAVE_K_MAX", "1")
    assert knn_plan(100, 100, 3, 1)["arm"] == "wave" and knn_plan(100, 100, 3, 2)["arm"] == "lds"
    assert knn_plan(100, 100, 3, 2)["capacity"] == 126 and knn_plan(100, 100, 3, 2)["wave_k_max"] == 1
    monkeypatch.setenv("NATAC_KNN_WAVE_K_MAX", "10")
    assert knn_plan(100, 100, 3, 10)["arm"] == "wave" and knn_plan(100, 100, 3, 11)["arm"] == "lds"
    for qt in (4, 8, 16, 32):
        monkeypatch.setenv("NATAC_KNN_QUERY_TILE", str(qt))
        p = knn_plan(1000, 1000, 7, 5)
        assert p["query_tile"] == qt and p["grid"] == (1000 + qt - 1) // qt
    monkeypatch.delenv("NATAC_KNN_QUERY_TILE")
    for rt in (64, 128, 256):
        monkeypatch.setenv("NATAC_KNN_REF_TILE", str(rt))
        assert knn_plan(1000, 1000, 7, 5)["ref_tile"] == rt


def test_overrides_outside_their_rules_are_ignored(monkeypatch):
    base = knn_plan(1000, 1000, 7, 5)
    for name, bad in (("NATAC_KNN_WAVE_K_MAX", ("0", "65", "-3", "x")), ("NATAC_KNN_QUERY_TILE", ("0", "2", "12", "64", "x")),
                      ("NATAC_KNN_REF_TILE", ("0", "32", "96", "512", "x"))):
        for v in bad:
            monkeypatch.setenv(name, v)
            assert knn_plan(1000, 1000, 7, 5) == base
        monkeypatch.delenv(name)
    # a tile whose LDS would pass the cap is not taken: 64 columns x 257 rows and the arrays of k = 1024
    monkeypatch.setenv("NATAC_KNN_REF_TILE", "256")
    assert knn_plan(1000, 1000, 64, 1024)["ref_tile"] == 64 and knn_plan(1000, 1000, 64, 5)["ref_tile"] == 256
    monkeypatch.delenv("NATAC_KNN_REF_TILE")
    monkeypatch.setenv("NATAC_KNN_QUERY_TILE", "32")
    assert knn_plan(1000, 1000, 64, 1024)["query_tile"] == 4 and knn_plan(1000, 1000, 64, 5)["query_tile"] == 32


@pytest.mark.parametrize("args,message", (((10, 10, 0, 1), "dim must be in [1, 64]"), ((10, 10, 65, 1), "dim must be in [1, 64]"),
                                          ((10, 10, 3, 0), "k must be in [1, 1024]"), ((10, 10, 3, 1025), "k must be in [1, 1024]"),
                                          ((10, 0, 3, 1), "nr must be in [1, 16777216]"), ((10, 2 ** 24 + 1, 3, 1), "nr must be in [1, 16777216]"),
                                          ((-1, 10, 3, 1), "nq must be at least 0"), ((2 ** 18 + 1, 10, 3, 1024), "nq * k must be at most 268435456"),
                                          ((10, 10, 3, 1, 0), "n_cu must be at least 1")))
def test_every_argument_limit_is_refused(args, message):
    with pytest.raises(L.NatacError) as e:
        knn_plan(*args)
    assert e.value.code == -1 and message in str(e.value)


def test_the_limits_at_their_edges_pass():
    assert knn_plan(2 ** 18, 2 ** 24, 64, 1024)["arm"] == "lds" and knn_plan(0, 1, 1, 1)["arm"] == "wave"
    assert (L.KNN_MAX_DIM, L.KNN_MAX_K, L.KNN_MAX_REFS, L.KNN_MAX_OUT, L.KNN_MAX_EXP) == (64, 1024, 2 ** 24, 2 ** 28, 500)


def test_the_restatement_agrees_with_python_floats():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20, 3))
    x[7] = x[3]                                  # a tie: the lower index first
    for k in (1, 4, 19, 25):
        assert R.same(R.knn(x, k), R.knn_loops(x, k))
    idx, d2 = R.knn(x, 25)
    assert np.all(idx[:, 19:] == -1) and np.all(np.isinf(d2[:, 19:])) and idx[3, 0] == 7 and idx[7, 0] == 3 and d2[3, 0] == 0.0
    # separate queries with and without an excluded reference
    a = R.knn(x, 3, queries=x[5:9], self_offset=5)
    assert R.same(a, tuple(v[5:9] for v in R.knn(x, 3)))
    b = R.knn(x, 3, queries=x[5:9])
    assert b[0][:, 0].tolist() == [5, 6, 3, 8] and np.all(b[1][:, 0] == 0.0)
