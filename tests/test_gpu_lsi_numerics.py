"""natac_sparse_lsi (csrc/natac_lsi.hpp; Context.sparse_lsi) where tests/test_gpu_lsi.py does not go: matrices whose SVD is known in closed
form, with graded and repeated singular values up to the rank rule's boundary; operands scaled by powers of two up to and past the range
of fp64; the second trip of every grid-stride loop and every residue of the row lengths; and ill-conditioned start blocks.

Tolerances are those of tests/test_gpu_lsi.py (its docstring derives them): TOL = 1e-10 relative to sigma[0] for singular values, products
and orthonormality, VEC_TOL = 1e-8 for unit vectors after the sign rule.  Nothing here is wider.  Where a scaling by 2^k is exact in every
operation of the algorithm the comparison is byte for byte.

Every call that returns also satisfies the residual identity |X V - U diag(sigma)| <= TOL * sigma[0], X from lsi_ref.weighted_matrix: by
construction U sigma = X Q W = X V whatever n_iter is, so this checks the cell-order product and the multiply arm of lsi_rows_small row by
row without the restatement."""
import numpy as np
import pytest

import lsi_ref as R
from test_gpu_lsi import SHORT_MAX, TOL, VEC_TOL, WAVE_MAX, _ctx, _orthonormal, _probe_check, _signs_fixed

pytestmark = pytest.mark.gpu


def _residual(got, ip, ix, da, n, rw, cs, **kw):
    s, U, V = got
    X = R.weighted_matrix(ip, ix, da, n, rw, cs, **kw)
    res = np.abs(X.dot(V) - U * s).max()
    print("residual / sigma[0]:", res / s[0])
    assert res <= TOL * s[0]


# ---- A. closed-form SVD: disjoint all-ones blocks of 9 windows x 4 cells, sigma_k = 6 s_k, U = 1/2, V = 1/3 ----
BW, BC = 9, 4


def _blocks(r, log2_ratio, extra=()):
    """r blocks with s_k = 2^(-g k), sigma[0] / sigma[r - 1] = 2^log2_ratio, and further blocks of the values `extra`"""
    s = 2.0 ** (-(float(log2_ratio) * np.arange(r)) / max(r - 1, 1))
    s = np.concatenate([s, np.asarray(extra, np.float64)])
    ip, ix, da = R.block_counts(len(s), BW, BC)
    rw, sigma, U, V = R.block_truth(s, BW, BC)
    q0 = np.random.default_rng(100 + r).standard_normal((len(rw), r))
    return dict(ip=ip, ix=ix, da=da, n=BC * len(s), rw=rw, cs=np.ones(BC * len(s)), q0=q0, sigma=sigma, U=U, V=V)


def _lsi(b, r, n_iter, f=None):
    f = f or _ctx().sparse_lsi
    return f(b["ip"], b["ix"], b["da"], b["n"], b["rw"], b["cs"], r, n_iter, b["q0"], transform="linear")


def _graded_checks(got, b):
    """the assertions of a graded case against the closed form; -> the largest error of a sigma_k relative to sigma_k itself"""
    s, U, V = got
    r = len(s)
    rel = np.abs(s - b["sigma"][:r]) / b["sigma"][:r]
    print("sigma error / sigma[0]: %.3g  largest sigma_k error / sigma_k: %.3g (k = %d)  U: %.3g  V: %.3g" % (
        np.abs(s - b["sigma"][:r]).max() / b["sigma"][0], rel.max(), int(np.argmax(rel)), np.abs(U - b["U"][:, :r]).max(),
        np.abs(V - b["V"][:, :r]).max()))
    assert np.abs(s - b["sigma"][:r]).max() <= TOL * b["sigma"][0]
    assert np.abs(U - b["U"][:, :r]).max() <= VEC_TOL and np.abs(V - b["V"][:, :r]).max() <= VEC_TOL
    _orthonormal(U, V)
    _signs_fixed(U)
    _residual(got, b["ip"], b["ix"], b["da"], b["n"], b["rw"], b["cs"], transform="linear")
    return rel.max()


@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("r", [6, 20, 64])
def test_blocks_all_sigma_equal(r, n_iter):
    """every basis of the row space is a set of singular vectors: sigma and the projectors are compared, the vectors are not"""
    b = _blocks(r, 0)
    s, U, V = got = _lsi(b, r, n_iter)
    print("sigma:", np.abs(s - 6.0).max() / 6.0, " U U^T:", np.abs(U.dot(U.T) - b["U"].dot(b["U"].T)).max(),
          " V V^T:", np.abs(V.dot(V.T) - b["V"].dot(b["V"].T)).max())
    assert np.abs(s - 6.0).max() <= TOL * 6.0
    assert np.abs(U.dot(U.T) - b["U"].dot(b["U"].T)).max() <= TOL and np.abs(V.dot(V.T) - b["V"].dot(b["V"].T)).max() <= TOL
    _orthonormal(U, V)
    _residual(got, b["ip"], b["ix"], b["da"], b["n"], b["rw"], b["cs"], transform="linear")


@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("log2_ratio", [10, 20])
@pytest.mark.parametrize("r", [6, 20, 64])
def test_blocks_graded(r, log2_ratio, n_iter):
    """rank exactly r: any n_iter gives the exact subspace, every difference from the closed form is rounding"""
    b = _blocks(r, log2_ratio)
    _graded_checks(_lsi(b, r, n_iter), b)


@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("r", [6, 20, 64])
def test_blocks_past_the_rank_rule(r, n_iter):
    """sigma[0] / sigma[r - 1] = 2^32: the Gram matrix's condition is 2^64, above 1 / (r eps) for every r"""
    b = _blocks(r, 32)
    with pytest.raises(ValueError, match="^rank$"):
        _lsi(b, r, n_iter)
    with pytest.raises(ValueError, match="^rank$"):
        _lsi(b, r, n_iter, R.sparse_lsi)


@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("log2_ratio", [24, 26, 28])
@pytest.mark.parametrize("r", [6, 20, 64])
def test_blocks_in_the_boundary_band(r, log2_ratio, n_iter):
    """between the ratio the restatement still takes for every r (2^20) and the one it refuses for every r (2^32): the call reports lost
    rank or it is as accurate as at 2^20 -- there is no third outcome.  Which of the two may differ from the restatement's."""
    b = _blocks(r, log2_ratio)
    try:
        got = _lsi(b, r, n_iter)
    except ValueError as e:
        assert str(e) == "rank"
        print("reported: rank")
        return
    _graded_checks(got, b)


def test_blocks_with_a_truncated_tail():
    """20 of 23 blocks wanted: truncation is real, the restatement is the reference at the tiers of test_parity_on_planted_matrix"""
    b = _blocks(20, 10, extra=2.0 ** -np.arange(12, 15))
    s_all = np.sort(b["sigma"])[::-1]
    assert np.array_equal(s_all, b["sigma"])
    want, got = _lsi(b, 20, 6, R.sparse_lsi), _lsi(b, 20, 6)
    qual = R.qualifying(s_all, 20)
    assert len(qual) >= 10
    print("sigma:", np.abs(got[0] - want[0]).max() / want[0][0], " U:", np.abs(got[1][:, qual] - want[1][:, qual]).max(),
          " V:", np.abs(got[2][:, qual] - want[2][:, qual]).max())
    assert np.abs(got[0] - want[0]).max() <= TOL * want[0][0]
    assert np.abs(got[1][:, qual] - want[1][:, qual]).max() <= VEC_TOL and np.abs(got[2][:, qual] - want[2][:, qual]).max() <= VEC_TOL
    _orthonormal(got[1], got[2])
    _signs_fixed(got[1])
    _probe_check(got, want, b["n"], len(b["rw"]))
    _residual(got, b["ip"], b["ix"], b["da"], b["n"], b["rw"], b["cs"], transform="linear")


# ---- B. magnitude: the 300 x 200 matrix of test_gpu_lsi.py's `small`, r = 12, n_iter = 2 ----
@pytest.fixture(scope="module")
def small():
    import scipy.sparse as sp
    rng = np.random.default_rng(31)
    A = sp.random(300, 200, density=0.2, random_state=7, format="csr")
    A.data = rng.integers(1, 6, len(A.data)).astype(np.float64)
    ip, ix, da = R.csr_of(A)
    tot, rw, cs = R.weights(ip, ix, da, 200)
    d = dict(ip=ip, ix=ix, da=da, rw=rw, cs=cs, q0=np.ascontiguousarray(rng.standard_normal((300, 64))[:, :12]))
    d["linear"] = _ctx().sparse_lsi(ip, ix, da, 200, rw, cs, 12, 2, d["q0"], transform="linear")
    d["log"] = _ctx().sparse_lsi(ip, ix, da, 200, rw, cs, 12, 2, d["q0"])
    for t in ("linear", "log"):
        _probe_check(d[t], R.sparse_lsi(ip, ix, da, 200, rw, cs, 12, 2, d["q0"], transform=t), 200, 300)
        _residual(d[t], ip, ix, da, 200, rw, cs, transform=t)
    return d


def _same_bytes(got, base, k=0):
    """sigma == base sigma * 2^k exactly, U and V the base's bytes"""
    assert np.all(np.isfinite(got[0])) and np.array_equal(got[0], np.ldexp(base[0], k))
    assert got[1].tobytes() == base[1].tobytes() and got[2].tobytes() == base[2].tobytes()


@pytest.mark.parametrize("k", [1, -1, 40, -40, 200, -200, 300, 480, -300, -480])
def test_linear_weights_scaled_by_a_power_of_two(small, k):
    """Every operation of the algorithm is +, x, fma, / or sqrt on operands that carry a common power of two (the products 2^k, their
    Gram matrices 2^2k, the Cholesky factors 2^k) and every threshold is relative: sigma scales, U and V keep their bytes."""
    d = small
    rw = np.ldexp(d["rw"], k)
    got = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, rw, d["cs"], 12, 2, d["q0"], transform="linear")
    _same_bytes(got, d["linear"], k)
    _residual(got, d["ip"], d["ix"], d["da"], 200, rw, d["cs"], transform="linear")


@pytest.mark.parametrize("k", [40, -40, 300, -300])
def test_log_scale_moved_into_col_scale(small, k):
    """t * scale is the same double, so the weighted entries are"""
    d = small
    cs, scale = np.ldexp(d["cs"], k), float(np.ldexp(1e4, -k))
    got = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], cs, 12, 2, d["q0"], scale=scale)
    _same_bytes(got, d["log"])
    _residual(got, d["ip"], d["ix"], d["da"], 200, d["rw"], cs, scale=scale)


@pytest.mark.parametrize("k", [40, -40, 300, -300])
def test_start_block_scaled_by_a_power_of_two(small, k):
    """orth(q0) is the same block: its Gram matrix carries 2^2k, its factor 2^k, and the solve divides that out"""
    d = small
    got = _ctx().sparse_lsi(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 12, 2, np.ldexp(d["q0"], k))
    _same_bytes(got, d["log"])
    _residual(got, d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"])


def _reports_range_or_is_right(f, args, kw, base, k):
    try:
        got = f(*args, **kw)
    except ValueError as e:
        assert str(e) == "range"
        print("reported: range")
        return
    assert all(np.all(np.isfinite(x)) for x in got)
    _probe_check(got, (np.ldexp(base[0], k), base[1], base[2]), 200, 300)
    _orthonormal(got[1], got[2])


@pytest.mark.parametrize("k", [520, -530, -560])
def test_linear_weights_beyond_the_range(small, k):
    """2^520: the Gram matrices overflow.  2^-530: their entries lie among the denormals and the pivots lose bits while staying above the
    relative floor.  2^-560: they vanish.  The call says "range" or it is right; so does the restatement."""
    d = small
    args = (d["ip"], d["ix"], d["da"], 200, np.ldexp(d["rw"], k), d["cs"], 12, 2, d["q0"])
    _reports_range_or_is_right(_ctx().sparse_lsi, args, dict(transform="linear"), d["linear"], k)
    _reports_range_or_is_right(R.sparse_lsi, args, dict(transform="linear"), d["linear"], k)
    _same_bytes(_ctx().sparse_lsi(*args[:4], d["rw"], *args[5:], transform="linear"), d["linear"])      # the context lives


@pytest.mark.parametrize("k", [600, -600])
def test_start_block_beyond_the_range(small, k):
    d = small
    args = (d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], 12, 2, np.ldexp(d["q0"], k))
    _reports_range_or_is_right(_ctx().sparse_lsi, args, {}, d["log"], 0)
    _reports_range_or_is_right(R.sparse_lsi, args, {}, d["log"], 0)


def test_status_2_is_range_and_the_outputs_are_zero(small):
    import ctypes as C
    from test_gpu_lsi import _vp
    from nucleoatac_amd import _lib as L
    d = small
    rw = np.ldexp(d["rw"], 520)
    s, U, V = np.ones(12), np.ones((200, 12)), np.ones((300, 12))
    st = C.c_int32(-7)
    rc = L.load().natac_sparse_lsi(_ctx()._h, 300, 200, _vp(d["ip"]), _vp(d["ix"]), _vp(d["da"]), _vp(rw), _vp(d["cs"]), 1e4, 0, 0, 12, 2,
                                   _vp(d["q0"]), _vp(s), _vp(U), _vp(V), C.byref(st), None)
    assert (rc, st.value) == (0, 2) and not s.any() and not U.any() and not V.any()


# ---- C. launch geometry: n_iter = 1 against the restatement ----
def _geometry_check(ip, ix, da, n, rw, cs, r, seed):
    m = len(ip) - 1
    q0 = np.random.default_rng(seed).standard_normal((m, r))
    want = R.sparse_lsi(ip, ix, da, n, rw, cs, r, 1, q0)
    got = _ctx().sparse_lsi(ip, ix, da, n, rw, cs, r, 1, q0)
    _probe_check(got, want, n, m)
    _orthonormal(got[1], got[2])
    _residual(got, ip, ix, da, n, rw, cs)
    return got


RESIDUES = sorted(set(range(SHORT_MAX + 1, SHORT_MAX + 17)) | set(range(WAVE_MAX - 15, WAVE_MAX + 65)) | {3 * WAVE_MAX + 5})


@pytest.fixture(scope="module")
def residues():
    """test_gpu_lsi.py's ladder with other lengths: sixteen consecutive ones from the wave arm's first, its last sixteen, the block arm's
    first sixty-four and one of three passes of the block -- every tail 0 to 3 of lsi_row_part's unrolled loop in every lane group, for 4, 2
    and 1 groups per wave and 4 waves per block; rows in block 1, columns in block 2, and a random block for rank"""
    import scipy.sparse as sp
    rng = np.random.default_rng(22)
    W = max(RESIDUES)
    rows, cols = [], []
    for i, L in enumerate(RESIDUES):
        rows.append(np.full(L, i))
        cols.append(np.sort(rng.choice(W, L, replace=False)))
    r0, c0 = len(RESIDUES), W
    for j, L in enumerate(RESIDUES):
        rows.append(r0 + np.sort(rng.choice(W, L, replace=False)))
        cols.append(np.full(L, c0 + j))
    r1, c1 = r0 + W, c0 + len(RESIDUES)
    F = sp.random(300, 300, density=0.05, random_state=5, format="coo")
    rows, cols = np.concatenate(rows + [r1 + F.row]), np.concatenate(cols + [c1 + F.col])
    m, n = r1 + 300, c1 + 300
    ip, ix, da = R.csr_of(sp.csr_matrix((rng.integers(1, 5, len(rows)), (rows, cols)), shape=(m, n)))
    assert np.diff(ip)[:r0].tolist() == RESIDUES and np.bincount(ix, minlength=n)[c0:c1].tolist() == RESIDUES
    return dict(ip=ip, ix=ix, da=da, m=m, n=n, rw=rng.uniform(0.5, 2.0, m), cs=rng.uniform(0.5, 2.0, n))


@pytest.mark.parametrize("r", [5, 24, 40])                   # 4, 2 and 1 lane groups per wave
def test_row_length_residues(residues, r):
    d = residues
    _geometry_check(d["ip"], d["ix"], d["da"], d["n"], d["rw"], d["cs"], r, r)


def test_short_arm_second_trip():
    """r = 40: one lane group per wave, 8192 blocks of 4 waves take 32,768 rows a trip.  135,000 windows of 2 cells, 34,000 cells of about
    8 windows: more short rows than that in both orientations.  m r = 5.4 M is more than 16384 * 256 elements, so lsi_mask_rows strides
    too, and the dropped windows lie on both sides of that line."""
    m, n, r = 135000, 34000, 40
    w = np.arange(m)
    ix = np.sort(np.stack([w % n, (7 * w + 3) % n], axis=1), axis=1)
    assert np.all(ix[:, 0] < ix[:, 1])
    ip, ix = np.arange(m + 1, dtype=np.int64) * 2, ix.ravel().astype(np.int32)
    rng = np.random.default_rng(23)
    da = rng.integers(1, 5, 2 * m).astype(np.int32)
    col_len = np.bincount(ix, minlength=n)
    assert m > 32768 and n > 32768 and col_len.max() <= SHORT_MAX and col_len.min() >= 1
    rw, cs = rng.uniform(0.5, 2.0, m), rng.uniform(0.5, 2.0, n)
    dropped = [5, 70000, 16384 * 256 // r + 1, 120000, m - 1]
    rw[dropped] = 0.0
    got = _geometry_check(ip, ix, da, n, rw, cs, r, 40)
    assert not got[2][dropped].any() and np.all(np.abs(got[2][[4, 6, m - 2]]).sum(axis=1) > 0)


def test_wave_arm_and_element_kernels_second_trip():
    """33,000 rows and columns of exactly 128 entries: more wave rows than the 32,768 of a trip (8192 blocks of 4 waves) on both sides, and
    4,224,000 entries, more than the 16384 * 256 that lsi_weight and lsi_transpose take a trip"""
    n, r = 33000, 8
    ip, ix, da = R.circulant_counts(n, 128, 24)
    assert SHORT_MAX < 128 <= WAVE_MAX and n > 32768 and len(ix) > 16384 * 256 and np.all(np.bincount(ix, minlength=n) == 128)
    rng = np.random.default_rng(25)
    _geometry_check(ip, ix, da, n, rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n), r, 8)


def test_block_arm_second_trip():
    """4,200 rows and columns of 4,100 entries: more block rows than the 4,096 blocks of a trip on both sides, each longer than a wave's
    share; the loop reuses the four waves' LDS words between its two barriers"""
    n, r = 4200, 8
    ip, ix, da = R.circulant_counts(n, 4100, 26)
    assert 4100 > WAVE_MAX and n > 4096 and np.all(np.bincount(ix, minlength=n) == 4100)
    rng = np.random.default_rng(27)
    _geometry_check(ip, ix, da, n, rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n), r, 9)


# ---- D. the start block ----
def _start(small, q0, f):
    d = small
    return f(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"], q0.shape[1], 2, q0)


def test_start_block_of_condition_1e6(small):
    d = small
    q0 = d["q0"].copy()
    q0[:, 1] = q0[:, 0] + 2.0 ** -20 * np.random.default_rng(71).standard_normal(300)
    assert 1e5 < np.linalg.cond(q0) < 1e8
    want, got = _start(d, q0, R.sparse_lsi), _start(d, q0, _ctx().sparse_lsi)
    _probe_check(got, want, 200, 300)
    _orthonormal(got[1], got[2])
    _signs_fixed(got[1])
    s_all = np.linalg.svd(R.weighted_matrix(d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"]).toarray(), compute_uv=False)
    qual = [j for j in R.qualifying(s_all, 12) if j < 3]
    assert qual and np.abs(got[1][:, qual] - want[1][:, qual]).max() <= VEC_TOL and np.abs(got[2][:, qual] - want[2][:, qual]).max() <= VEC_TOL
    _residual(got, d["ip"], d["ix"], d["da"], 200, d["rw"], d["cs"])


def test_start_block_without_rank(small):
    d = small
    twin = d["q0"].copy()
    twin[:, 7] = twin[:, 2]
    rw = d["rw"].copy()
    rw[[3, 150, 299]] = 0.0
    dead = np.zeros((300, 3))
    dead[[3, 150, 299]] = np.random.default_rng(72).standard_normal((3, 3))
    for f in (_ctx().sparse_lsi, R.sparse_lsi):
        with pytest.raises(ValueError, match="^rank$"):
            _start(d, twin, f)
        with pytest.raises(ValueError, match="^rank$"):
            f(d["ip"], d["ix"], d["da"], 200, rw, d["cs"], 3, 2, dead)
    _same_bytes(_start(d, d["q0"], _ctx().sparse_lsi), d["log"])
