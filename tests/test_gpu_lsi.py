"""The truncated SVD of the weighted cell-by-window matrix on the GPU (natac_sparse_lsi, csrc/natac_lsi.hpp; Context.sparse_lsi) against the
NumPy / scipy restatement of tests/lsi_ref.py and numpy.linalg.svd.

Tolerances: the project's default tier, 1e-10, taken relative to sigma[0] -- the largest-singular-value form of the 1e-10 relative +
1e-12 absolute of the parity tests.  A backward-stable pipeline errs by about r * eps * sigma[0], some 1e-14 * sigma[0]; CholeskyQR2 and
Householder QR agree to 3e-16 in sigma and 2e-15 in U on the planted matrix on a CPU.  Vectors are unit vectors whose error scales with
sigma[0] / gap: they are compared at 1e-8 absolute after the sign rule, and only where both neighbouring gaps are at least
1e-3 * sigma[0] by the dense SVD; the tests assert how many components qualify.  Where no dense SVD is at hand (the row-length ladder is
4,400 x 4,400) or the gaps are not the point, the vectors are compared through U diag(sigma) V^T applied to a few fixed probe vectors from
both sides: that operator is X Q Q^T, a function of the iterated subspace alone, its norm is sigma[0], and every row of U and of V takes
part in it -- so the bound is again 1e-10 * sigma[0] for probes of unit length."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import lsi_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

_HDR = open(os.path.join(ROOT, "include", "natac.h")).read()
MAX_R = int(re.search(r"#define NATAC_LSI_MAX_R (\d+)", _HDR).group(1))
SHORT_MAX = int(re.search(r"#define NATAC_LSI_SHORT_MAX (\d+)", _HDR).group(1))
WAVE_MAX = int(re.search(r"#define NATAC_LSI_WAVE_MAX (\d+)", _HDR).group(1))
LADDER = sorted({0, 1, 2, 63, 64, 65, SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1, WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1})
TOL, VEC_TOL = 1e-10, 1e-8


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _probe_check(got, want, n, m):
    """sigma, and U diag(sigma) V^T from both sides on fixed unit probes, to TOL * sigma[0]; the bases are orthonormal"""
    (s, U, V), (s0, U0, V0) = got, want
    assert s.shape == s0.shape and U.shape == U0.shape == (n, len(s)) and V.shape == V0.shape == (m, len(s))
    assert np.all(np.diff(s) <= 0) and np.abs(s - s0).max() <= TOL * s0[0]
    rng = np.random.default_rng(77)
    Zm, Zn = rng.standard_normal((m, 3)), rng.standard_normal((n, 3))
    Zm, Zn = Zm / np.linalg.norm(Zm, axis=0), Zn / np.linalg.norm(Zn, axis=0)
    assert np.abs(U.dot(s[:, None] * V.T.dot(Zm)) - U0.dot(s0[:, None] * V0.T.dot(Zm))).max() <= TOL * s0[0]
    assert np.abs(V.dot(s[:, None] * U.T.dot(Zn)) - V0.dot(s0[:, None] * U0.T.dot(Zn))).max() <= TOL * s0[0]


def _orthonormal(U, V):
    r = U.shape[1]
    assert np.abs(U.T.dot(U) - np.eye(r)).max() <= TOL and np.abs(V.T.dot(V) - np.eye(r)).max() <= TOL


def _signs_fixed(U):
    top = np.argmax(np.abs(U), axis=0)
    assert np.all(U[top, np.arange(U.shape[1])] > 0)


def test_constants_are_what_the_arms_need():
    assert MAX_R == 64 and 1 <= SHORT_MAX < 63 and 65 < WAVE_MAX <= 1 << 16


# ---- exact rank ----
@pytest.fixture(scope="module")
def exact():
    """counts = 6 outer products of small positive integer vectors on overlapping supports: 500 windows x 300 cells, rank 6"""
    rng = np.random.default_rng(11)
    A = np.zeros((500, 300), np.int64)
    for k in range(6):
        u, v = np.zeros(500, np.int64), np.zeros(300, np.int64)
        u[k * 60:k * 60 + 200] = rng.integers(1, 4, 200)
        v[k * 40:k * 40 + 100] = rng.integers(1, 4, 100)
        A += np.outer(u, v)
    ip, ix, da = R.csr_of(A)
    rw, cs = rng.uniform(0.5, 2.0, 500), rng.uniform(0.5, 2.0, 300)
    X = R.weighted_matrix(ip, ix, da, 300, rw, cs, transform="linear").toarray()
    assert np.linalg.matrix_rank(X) == 6
    return dict(ip=ip, ix=ix, da=da, rw=rw, cs=cs, X=X, s=np.linalg.svd(X, compute_uv=False), q0=rng.standard_normal((500, 6)))


@pytest.mark.parametrize("n_iter", [1, 3])
def test_exact_rank(exact, n_iter):
    e = exact
    s, U, V = _ctx().sparse_lsi(e["ip"], e["ix"], e["da"], 300, e["rw"], e["cs"], 6, n_iter, e["q0"], transform="linear")
    print("sigma error / sigma[0]:", np.abs(s - e["s"][:6]).max() / e["s"][0], " reconstruction:", np.abs((U * s).dot(V.T) - e["X"]).max() / e["s"][0])
    assert np.abs(s - e["s"][:6]).max() <= TOL * e["s"][0]
    assert np.abs((U * s).dot(V.T) - e["X"]).max() <= TOL * e["s"][0]
    _orthonormal(U, V)
    _signs_fixed(U)


# ---- parity on the planted matrix ----
@pytest.fixture(scope="module")
def planted():
    A, group = R.planted()
    ip, ix, da = R.csr_of(A)
    n = A.shape[1]
    tot, rw, cs = R.weights(ip, ix, da, n)
    X = R.weighted_matrix(ip, ix, da, n, rw, cs)
    s_all = np.linalg.svd(X.toarray(), compute_uv=False)
    return dict(ip=ip, ix=ix, da=da, n=n, m=A.shape[0], rw=rw, cs=cs, s_all=s_all,
                q0=np.random.default_rng(1).standard_normal((A.shape[0], 20)))


@pytest.mark.parametrize("n_iter", [1, 4])
def test_parity_on_planted_matrix(planted, n_iter):
    p = planted
    want = R.sparse_lsi(p["ip"], p["ix"], p["da"], p["n"], p["rw"], p["cs"], 20, n_iter, p["q0"])
    got = _ctx().sparse_lsi(p["ip"], p["ix"], p["da"], p["n"], p["rw"], p["cs"], 20, n_iter, p["q0"])
    qual = R.qualifying(p["s_all"], 10)
    assert qual[:4] == [0, 1, 2, 3]                          # the depth component and the three group contrasts
    print("sigma:", np.abs(got[0][:10] - want[0][:10]).max() / want[0][0], " U:", np.abs(got[1][:, qual] - want[1][:, qual]).max(),
          " V:", np.abs(got[2][:, qual] - want[2][:, qual]).max())
    assert np.abs(got[0][:10] - want[0][:10]).max() <= TOL * want[0][0]
    assert np.abs(got[1][:, qual] - want[1][:, qual]).max() <= VEC_TOL and np.abs(got[2][:, qual] - want[2][:, qual]).max() <= VEC_TOL
    _orthonormal(got[1], got[2])
    _signs_fixed(got[1])
    _probe_check(got, want, p["n"], p["m"])


# ---- the arms of the sparse kernel, both orientations ----
@pytest.fixture(scope="module")
def ladder():
    """windows x cells: a block whose rows have exactly the LADDER lengths, a block whose columns have them, and a random block that
    gives the matrix rank enough for r = 40"""
    rng = np.random.default_rng(21)
    W = max(LADDER)
    rows, cols = [], []
    for i, L in enumerate(LADDER):                           # block 1: row i has L entries
        c = np.sort(rng.choice(W, L, replace=False))
        rows += [i] * L
        cols += c.tolist()
    r0, c0 = len(LADDER), W
    for j, L in enumerate(LADDER):                           # block 2: column c0 + j has L entries
        w = np.sort(rng.choice(W, L, replace=False))
        rows += (r0 + w).tolist()
        cols += [c0 + j] * L
    r1, c1 = r0 + W, c0 + len(LADDER)
    F = sp.random(300, 300, density=0.05, random_state=5, format="coo")
    rows += (r1 + F.row).tolist()
    cols += (c1 + F.col).tolist()
    m, n = r1 + 300, c1 + 300
    A = sp.csr_matrix((rng.integers(1, 5, len(rows)), (rows, cols)), shape=(m, n))
    ip, ix, da = R.csr_of(A)
    row_len, col_len = np.diff(ip), np.bincount(ix, minlength=n)
    assert row_len[:r0].tolist() == LADDER and col_len[c0:c1].tolist() == LADDER
    return dict(ip=ip, ix=ix, da=da, m=m, n=n, rw=rng.uniform(0.5, 2.0, m), cs=rng.uniform(0.5, 2.0, n))


@pytest.mark.parametrize("r", [5, 24, 40])                   # 4, 2 and 1 lane groups per wave
def test_row_length_ladder(ladder, r):
    d = ladder
    q0 = np.random.default_rng(r).standard_normal((d["m"], r))
    want = R.sparse_lsi(d["ip"], d["ix"], d["da"], d["n"], d["rw"], d["cs"], r, 1, q0)
    got = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], d["n"], d["rw"], d["cs"], r, 1, q0)
    _probe_check(got, want, d["n"], d["m"])
    _orthonormal(got[1], got[2])
    # the empty row and the empty column have zero vectors
    assert not got[2][LADDER.index(0)].any() and not got[1][max(LADDER) + LADDER.index(0)].any()


# ---- every block width ----
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(31)
    A = sp.random(300, 200, density=0.2, random_state=7, format="csr")
    A.data = rng.integers(1, 6, len(A.data)).astype(np.float64)
    ip, ix, da = R.csr_of(A)
    tot, rw, cs = R.weights(ip, ix, da, 200)
    return dict(ip=ip, ix=ix, da=da, rw=rw, cs=cs, q0=rng.standard_normal((300, 64)),
                s_all=np.linalg.svd(R.weighted_matrix(ip, ix, da, 200, rw, cs).toarray(), compute_uv=False))


@pytest.mark.parametrize("r", [1, 2, 15, 16, 17, 32, 33, 63, 64])
def test_width_ladder(small, r):
    d = small
    q0 = np.ascontiguousarray(d["q0"][:, :r])
    want = R.sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], r, 2, q0)
    got = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], r, 2, q0)
    _probe_check(got, want, 200, 300)
    _orthonormal(got[1], got[2])
    _signs_fixed(got[1])
    qual = [j for j in R.qualifying(d["s_all"], r) if j < 3]
    assert np.abs(got[1][:, qual] - want[1][:, qual]).max(initial=0.0) <= VEC_TOL and np.abs(got[2][:, qual] - want[2][:, qual]).max(initial=0.0) <= VEC_TOL


def test_kernel_ms_is_reported(small):
    d = small
    out = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 8, 1, d["q0"][:, :8], with_kernel_ms=True)
    assert len(out) == 4 and out[3] > 0


# ---- determinism ----
def test_two_calls_give_the_same_bytes(small, planted):
    d, p = small, planted
    for args in ((d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 24, 2, np.ascontiguousarray(d["q0"][:, :24])),
                 (p["ip"], p["ix"], p["da"], p["n"], p["rw"], p["cs"], 20, 2, p["q0"])):
        a, b = _ctx().sparse_lsi(*args), _ctx().sparse_lsi(*args)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # the same entries stored behind others (row_ptr[0] > 0): nothing changes
    ip, ix, da = d["ip"] + 5, np.concatenate([np.zeros(5, np.int32), d["ix"]]), np.concatenate([np.ones(5, np.int32), d["da"]])
    a = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 24, 2, np.ascontiguousarray(d["q0"][:, :24]))
    b = _ctx().sparse_lsi(ip, ix, da, 200, d["rw"], d["cs"], 24, 2, np.ascontiguousarray(d["q0"][:, :24]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_two_equal_length_rows_exchanged(small):
    """Windows 10 and 11 are given the same number of entries and exchanged with their weights and their rows of q0: the rows of V are
    exchanged and nothing else changes.  Not byte for byte: a cell that holds both windows now adds them in the other order, and so does
    the Gram sum over the rows of Q -- a change of summation order, inside the tier the rest of the file uses."""
    d = small
    A = sp.csr_matrix((d["da"], d["ix"], d["ip"]), shape=(300, 200)).tolil()
    A[11] = 0
    A[11, sorted(np.random.default_rng(2).choice(200, A[10].nnz, replace=False).tolist())] = 3
    A = A.tocsr()
    perm = np.arange(300)
    perm[[10, 11]] = [11, 10]
    q0 = np.ascontiguousarray(d["q0"][:, :12])
    ip, ix, da = R.csr_of(A)
    assert ip[11] - ip[10] == ip[12] - ip[11]
    a = _ctx().sparse_lsi(ip, ix, da, 200, d["rw"], d["cs"], 12, 2, q0)
    ip2, ix2, da2 = R.csr_of(A[perm])
    b = _ctx().sparse_lsi(ip2, ix2, da2, 200, d["rw"][perm], d["cs"], 12, 2, np.ascontiguousarray(q0[perm]))
    assert np.array_equal(np.diff(ip), np.diff(ip2))
    _probe_check((b[0], b[1], b[2][perm]), a, 200, 300)
    assert np.abs(b[0] - a[0]).max() <= TOL * a[0][0]


# ---- dropped rows and columns, binarize ----
def test_dropped_rows_and_columns(small):
    d = small
    rw, cs = d["rw"].copy(), d["cs"].copy()
    rw[[0, 17, 299]] = 0.0
    cs[[3, 4, 199]] = 0.0
    q0 = np.ascontiguousarray(d["q0"][:, :10])
    s, U, V = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, rw, cs, 10, 2, q0)
    assert not U[[3, 4, 199]].any() and not V[[0, 17, 299]].any() and np.all(np.abs(U).sum(axis=1)[[0, 1, 2, 5]] > 0)
    _probe_check((s, U, V), R.sparse_lsi(d["ip"], d["ix"], d["da"], 200, rw, cs, 10, 2, q0), 200, 300)
    # the matrix without them
    A = sp.csr_matrix((d["da"], d["ix"], d["ip"]), shape=(300, 200))
    kr, kc = np.flatnonzero(rw > 0), np.flatnonzero(cs > 0)
    ip2, ix2, da2 = R.csr_of(A[kr][:, kc])
    want = R.sparse_lsi(ip2, ix2, da2, len(kc), rw[kr], cs[kc], 10, 2, np.ascontiguousarray(q0[kr]))
    _probe_check((s, U[kc], V[kr]), want, len(kc), len(kr))
    _orthonormal(U, V)


def test_binarize_is_counts_of_one(small):
    d = small
    q0 = np.ascontiguousarray(d["q0"][:, :9])
    for transform in ("log", "linear"):
        a = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 9, 1, q0, transform=transform, binarize=True)
        b = _ctx().sparse_lsi(d["ip"], d["ix"], np.ones_like(d["da"]), 200, d["rw"], d["cs"], 9, 1, q0, transform=transform)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        _probe_check(a, R.sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 9, 1, q0, transform=transform, binarize=True), 200, 300)
        c = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 9, 1, q0, transform=transform)
        assert np.abs(c[0] - a[0]).max() > 1e-3 * a[0][0]      # the counts do matter
    # scale reaches the log transform
    a = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 9, 1, q0, scale=10.0)
    _probe_check(a, R.sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 9, 1, q0, scale=10.0), 200, 300)


# ---- lost rank ----
def test_lost_rank_is_reported_and_the_context_lives(exact):
    rng = np.random.default_rng(41)
    A = rng.integers(1, 4, (60, 3)).dot(rng.integers(1, 4, (3, 40)))
    ip, ix, da = R.csr_of(A)
    assert np.linalg.matrix_rank(A) == 3
    with pytest.raises(ValueError, match="^rank$"):
        _ctx().sparse_lsi(ip, ix, da, 40, np.ones(60), np.ones(40), 5, 2, rng.standard_normal((60, 5)), transform="linear")
    with pytest.raises(ValueError, match="^rank$"):
        R.sparse_lsi(ip, ix, da, 40, np.ones(60), np.ones(40), 5, 2, rng.standard_normal((60, 5)), transform="linear")
    s, U, V = _ctx().sparse_lsi(ip, ix, da, 40, np.ones(60), np.ones(40), 3, 2, rng.standard_normal((60, 3)), transform="linear")
    assert np.abs(s - np.linalg.svd(A.astype(np.float64), compute_uv=False)[:3]).max() <= TOL * s[0]
    e = exact
    s, U, V = _ctx().sparse_lsi(e["ip"], e["ix"], e["da"], 300, e["rw"], e["cs"], 6, 1, e["q0"], transform="linear")
    assert np.abs(s - e["s"][:6]).max() <= TOL * e["s"][0]


# ---- operand checks ----
def _raw(ip, ix, da, n, rw, cs, r, n_iter, q0, scale=1e4, transform=1, binarize=0, m=None, out=True, status=True):
    """natac_sparse_lsi called directly -> (return code, status)"""
    from nucleoatac_amd import _lib as L
    lib = L.load()
    m = len(ip) - 1 if m is None else m
    rr = max(1, min(r, 64))
    s, U, V = np.zeros(rr), np.zeros((max(n, 1), rr)), np.zeros((max(m, 1), rr))
    st = C.c_int32(-7)
    rc = lib.natac_sparse_lsi(_ctx()._h, m, n, _vp(ip), _vp(ix), _vp(da), _vp(rw), _vp(cs), scale, transform, binarize, r, n_iter, _vp(q0),
                              _vp(s) if out else None, _vp(U) if out else None, _vp(V) if out else None, C.byref(st) if status else None, None)
    return rc, st.value


def test_operand_checks():
    from nucleoatac_amd import _lib as L
    rng = np.random.default_rng(51)
    A = sp.random(30, 20, density=0.4, random_state=3, format="csr")
    A.data[:] = 2
    ip, ix, da = R.csr_of(A)
    rw, cs, q0 = np.ones(30), np.ones(20), rng.standard_normal((30, 4))
    good = (ip, ix, da, 20, rw, cs, 4, 1, q0)
    assert _raw(*good) == (0, 0)

    def bad(what, *args, **kw):
        rc, st = _raw(*args, **kw)
        assert rc == -1 and st == -7, what                   # NATAC_E_ARG, nothing written
        assert len(L.load().natac_last_error()) > 0
        assert _raw(*good) == (0, 0), what                   # and a correct call still works

    def with_(i, v):
        a = list(good)
        a[i] = v
        return a
    big_q0 = rng.standard_normal((30, 64))
    x = ip.copy(); x[6] = x[5] - 1
    bad("row_ptr not monotone", *with_(0, x))
    x = ip.copy(); x[0] = -1
    bad("row_ptr[0] negative", *with_(0, x))
    x = ix.copy(); x[3] = 20
    bad("column == n", *with_(1, x))
    x = ix.copy(); x[3] = -1
    bad("column negative", *with_(1, x))
    k = int(np.flatnonzero(np.diff(ip) >= 2)[0])
    x = ix.copy(); x[ip[k] + 1] = x[ip[k]]
    bad("columns equal in a row", *with_(1, x))
    x = ix.copy(); x[ip[k]], x[ip[k] + 1] = ix[ip[k] + 1], ix[ip[k]]
    bad("columns descending in a row", *with_(1, x))
    x = da.copy(); x[7] = 0
    bad("count 0", *with_(2, x))
    x = da.copy(); x[7] = -3
    bad("count negative", *with_(2, x))
    for r in (0, -1, 65, 21, 31):                            # out of range; more than the 20 live columns; more than the 30 live rows
        bad("r = %d" % r, ip, ix, da, 20, rw, cs, r, 1, big_q0)
    z = rw.copy(); z[:27] = 0
    bad("r more than the live rows", *with_(4, z))
    z = cs.copy(); z[:17] = 0
    bad("r more than the live columns", *with_(5, z))
    bad("n_iter 0", *with_(7, 0))
    bad("n_iter negative", *with_(7, -2))
    for v in (-1.0, np.nan, np.inf):
        z = rw.copy(); z[2] = v
        bad("row_weight %r" % v, *with_(4, z))
        z = cs.copy(); z[2] = v
        bad("col_scale %r" % v, *with_(5, z))
        bad("scale %r" % v, *good, scale=v)
    for v in (np.nan, -np.inf):
        z = q0.copy(); z[29, 3] = v
        bad("q0 %r" % v, *with_(8, z))
    bad("transform 2", *good, transform=2)
    for i in (0, 1, 2, 4, 5, 8):
        bad("null operand %d" % i, *with_(i, None), m=30)
    bad("null outputs", *good, out=False)
    rc, st = _raw(*good, status=False)
    assert rc == -1 and _raw(*good) == (0, 0)


def test_empty_inputs_both_ways():
    rng = np.random.default_rng(61)
    one = np.zeros(1, np.int64)
    # no windows, no cells: r cannot be at most the number of live rows and columns
    assert _raw(one, None, None, 5, np.zeros(0), np.ones(5), 1, 1, np.zeros((0, 1)), m=0)[0] == -1
    assert _raw(np.zeros(4, np.int64), None, None, 0, np.ones(3), np.zeros(0), 1, 1, np.ones((3, 1)))[0] == -1
    with pytest.raises(Exception):
        _ctx().sparse_lsi(one, [], [], 5, [], np.ones(5), 1, 1, np.zeros((0, 1)))
    # windows and cells, and no entry: no direction at all
    assert _raw(np.zeros(4, np.int64), None, None, 5, np.ones(3), np.ones(5), 2, 1, rng.standard_normal((3, 2))) == (0, 1)
    with pytest.raises(ValueError, match="^rank$"):
        _ctx().sparse_lsi(np.zeros(4, np.int64), [], [], 5, np.ones(3), np.ones(5), 2, 1, rng.standard_normal((3, 2)))
    # one entry is one direction
    s, U, V = _ctx().sparse_lsi([0, 0, 1, 1], [2], [3], 5, np.ones(3), np.ones(5), 1, 1, np.ones((3, 1)), transform="linear")
    assert abs(s[0] - 3.0) <= TOL * 3 and np.allclose(U[:, 0], [0, 0, 1, 0, 0], atol=TOL, rtol=0) and np.allclose(V[:, 0], [0, 1, 0], atol=TOL, rtol=0)
