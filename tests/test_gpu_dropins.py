"""The single-region drop-ins (csrc/natac_dropins.hpp; kernels at the end of csrc/natac_kernels.hpp) at their edges and past their grid caps.

Integer-valued outputs (fragment matrix, insertions, stranded insertions, size histograms) are compared for equality with the oracle or
a NumPy count.  Floating outputs are compared with the exact value of tests/dropins_ref.py under a bound derived from the kernel's
operation count (U = 2^-52; the derivations are in dropins_ref's docstrings), and each case prints its largest error / bound.

Sizes are the smallest that reach each arm: the fragment kernels' grid is capped at 4096 blocks of 256, natac_i32_to_f64's too,
natac_cov_closed's at 1024 blocks of 256, natac_cov_literal's at 4096 one-row blocks; natac_size_hist keeps its histogram in LDS up to
8192 bins and goes to global atomics above."""
import ctypes as C

import numpy as np
import pytest

import dropins_ref as R

pytestmark = pytest.mark.gpu

CAP = 4096 * 256                # threads of a capped fragment / conversion grid
SENTINEL = -7.0
CUTOFF = 2.705543454095404      # chi2.ppf(0.9, 1)


@pytest.fixture(scope="module")
def ctx():
    from nucleoatac_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _lib():
    from nucleoatac_amd import _lib as L
    return L.load()


def report(what, err, bound):
    """print largest error / bound, then assert every error is inside its bound"""
    err, bound = np.atleast_1d(err), np.atleast_1d(bound)
    ratio = np.max(err / np.where(bound > 0, bound, 1), initial=0)
    print("%s: largest error / bound %.3g" % (what, ratio))
    assert np.all(err <= bound), what
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. past the grid caps
# ---------------------------------------------------------------------------------------------------------------------------------
def np_fragment_mat(l, n, start, end, lower, upper):
    n = n.astype(np.int64)
    row, col = n - lower, (n - 1) // 2 + l - start
    ok = (row >= 0) & (row < upper - lower) & (col >= 0) & (col < end - start)
    return np.bincount(row[ok] * (end - start) + col[ok], minlength=(upper - lower) * (end - start)).reshape(upper - lower, end - start).astype(np.float64)


def np_stranded(l, n, start, end, lower, upper):
    n = n.astype(np.int64)
    keep = (n >= lower) & (n < upper)
    lp, rp = l[keep] - start, l[keep] + n[keep] - 1 - start
    npos = end - start
    return (np.bincount(lp[(lp >= 0) & (lp < npos)], minlength=npos).astype(np.float64),
            np.bincount(rp[(rp >= 0) & (rp < npos)], minlength=npos).astype(np.float64))


def test_fragment_kernels_past_the_grid_cap(ctx):
    """CAP + 257 fragments: the grid-stride loops of the three count kernels take a second trip, for the first 257 threads only"""
    rng = np.random.default_rng(11)
    nf, start, end, lower, upper = CAP + 257, 1000, 3917, 30, 250
    l = rng.integers(start - 300, end + 300, nf).astype(np.int64)
    n = rng.integers(-5, 400, nf).astype(np.int32)                 # both sides of [lower, upper)
    ref_mat = np_fragment_mat(l, n, start, end, lower, upper)
    plus, minus = np_stranded(l, n, start, end, lower, upper)
    # the fragments of the second trip show in every reference: a loop that stops after one trip cannot pass
    assert np.any(ref_mat != np_fragment_mat(l[:CAP], n[:CAP], start, end, lower, upper))
    p1, m1 = np_stranded(l[:CAP], n[:CAP], start, end, lower, upper)
    assert np.any(plus != p1) and np.any(minus != m1)
    assert np.array_equal(ctx.make_fragment_mat(l, n, start, end, lower, upper), ref_mat)
    assert np.array_equal(ctx.get_insertions(l, n, start, end, lower, upper), plus + minus)
    gp, gm = ctx.get_stranded_insertions(l, n, start, end, lower, upper)
    assert np.array_equal(gp, plus) and np.array_equal(gm, minus)


def test_count_conversion_past_the_grid_cap(ctx):
    """a region of CAP + 257 bases (insertions) and of CAP / 2 + 129 (stranded: two arrays converted as one of CAP + 258): the second
    trip of natac_i32_to_f64 writes the last bases, which hold counts"""
    rng = np.random.default_rng(12)
    lower, upper = 0, 300
    for npos, stranded in ((CAP + 257, False), (CAP // 2 + 129, True)):
        start = 5000
        end = start + npos
        l = np.concatenate([rng.integers(start - 100, end + 100, 3000), rng.integers(end - 400, end, 600)]).astype(np.int64)
        n = rng.integers(0, 350, len(l)).astype(np.int32)
        plus, minus = np_stranded(l, n, start, end, lower, upper)
        assert minus[-129:].sum() > 0 and plus[-129:].sum() > 0          # counts in the bases only the second trip converts
        if stranded:
            gp, gm = ctx.get_stranded_insertions(l, n, start, end, lower, upper)
            assert np.array_equal(gp, plus) and np.array_equal(gm, minus)
        else:
            assert np.array_equal(ctx.get_insertions(l, n, start, end, lower, upper), plus + minus)


@pytest.mark.parametrize("literal,n", [(False, 1024 * 256 + 300), (True, 4100)])
def test_calculate_cov_past_the_grid_cap(ctx, literal, n):
    """closed form past 1024 blocks x 256 threads, literal pair sum past 4096 one-row blocks.  One dropped element is orders of magnitude
    outside the bound (asserted on the exact sums), and the value is well conditioned, so the bound means something."""
    rng = np.random.default_rng(13 + n)
    p = rng.random(n) ** 3
    p /= p.sum()
    v = rng.uniform(-1.0, 1.0, n)
    r = 37
    exact, bound, cond = R.calculate_cov(p, v, r, literal)
    assert cond < 100, cond
    # the elements past the cap carry far more than the bound: the exact value without the last 100 is outside it
    short = R.calculate_cov(p[:-100], v[:-100], r, literal)[0]
    assert abs(float(short - exact)) > 1000 * bound
    got = ctx.calculate_cov(p, v, r, literal=literal)
    report("calculate_cov %s n=%d" % ("literal" if literal else "closed", n), R.errors([got], [exact]), bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. size-histogram arms
# ---------------------------------------------------------------------------------------------------------------------------------
def np_size_hist(l, n, cs, ce, lower, upper):
    """the search-count restatement: a fragment counts once per chunk that holds its centre"""
    n = n.astype(np.int64)
    c = l + (n - 1) // 2
    ok = (n >= lower) & (n < upper)
    cnt = np.searchsorted(np.sort(cs), c, "right") - np.searchsorted(np.sort(np.maximum(ce, cs)), c, "right")
    return np.bincount(n[ok] - lower, weights=cnt[ok].astype(np.float64), minlength=upper - lower)[:upper - lower]


@pytest.mark.parametrize("upper", [8192, 8193, 20000, 1 << 20])
def test_size_hist_lds_and_global_arms(ctx, upper):
    """8192 bins: the last LDS histogram; 8193, 20000 and the widest accepted range: global atomics.  Sizes reach the last bin."""
    rng = np.random.default_rng(upper)
    nf = 30000
    l = np.sort(rng.integers(0, 400000, nf)).astype(np.int64)
    n = rng.integers(-3, upper + 5, nf).astype(np.int32)
    n[[5, 2047, 2048, nf - 1]] = upper - 1
    n[[6, nf - 2]] = upper
    span = 400000 + upper // 2                                       # where the centres l + (n - 1) // 2 fall
    cs = rng.integers(0, span, 40).astype(np.int64)
    ce = cs + rng.integers(0, span // 4, 40)
    cs[0], ce[0] = l[5] + (upper - 2) // 2 - 10, l[5] + (upper - 2) // 2 + 10      # a chunk around a centre of the largest size
    ref = np_size_hist(l, n, cs, ce, 0, upper)
    assert ref[-1] > 0 and ref.sum() > nf // 2
    assert np.array_equal(ctx.fragment_sizes(l, n, cs, ce, 0, upper), ref)


def test_size_hist_refuses_more_than_2_20_bins(ctx):
    from nucleoatac_amd import _lib as L
    with pytest.raises(L.NatacError, match="size range too wide"):
        ctx.fragment_sizes(np.array([10], np.int64), np.array([5], np.int32), [0], [100], 0, (1 << 20) + 1)
    with pytest.raises(L.NatacError, match="size range too wide"):
        ctx.fragment_sizes(np.array([10], np.int64), np.array([5], np.int32), [0], [100], -1, 1 << 20)


def test_size_hist_counts_negative_sizes_under_a_negative_lower(ctx):
    """lower = -6: a size in [-6, 0) passes the filter and is counted into bin size + 6, as the reference does.  (The kernel's mark
    for "not countable" was -1 and the test `< 0`, which dropped them; the mark is now INT_MIN.)"""
    from oracle import natac_oracle as O
    rng = np.random.default_rng(21)
    nf, lower, upper = 5000, -6, 40                                   # three segments of 2048
    l = np.sort(rng.integers(0, 3000, nf)).astype(np.int64)
    n = rng.integers(-10, 50, nf).astype(np.int32)
    cs = np.array([100, 900, 1000, 2500], np.int64)
    ce = np.array([1200, 1500, 1000, 2900], np.int64)
    ref = O.fragment_sizes_from_chunks(l, n.astype(np.int64), cs, ce, lower, upper)
    assert ref[:6].min() > 0                                           # every negative bin holds something
    assert np.array_equal(ctx.fragment_sizes(l, n, cs, ce, lower, upper), ref)
    # a segment whose only countable fragments are negative sizes: they alone set the segment's centre range
    n2 = np.where(n < 0, n, 45).astype(np.int32)
    ref2 = O.fragment_sizes_from_chunks(l, n2.astype(np.int64), cs, ce, lower, upper)
    assert ref2[6:].sum() == 0 and ref2[:6].sum() > 0
    assert np.array_equal(ctx.fragment_sizes(l, n2, cs, ce, lower, upper), ref2)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. count-kernel edges, by construction
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_fragments(start, end, lower, upper):
    """every size of interest with its left end, and then its right end l + n - 1, on start - 1, start, end - 1 and end"""
    l, n = [], []
    for s in (-3, 0, 1, 2, lower - 1, lower, upper - 1, upper):
        for b in (start - 1, start, end - 1, end):
            l += [b, b - s + 1]
            n += [s, s]
    return np.array(l, np.int64), np.array(n, np.int32)


@pytest.mark.parametrize("start,lower,shift", [(100, 4, 0), (-20, 4, 0), (100, -5, 0), (-20, -5, 0), (100, 4, 1 << 40), (100, -5, 1 << 40),
                                                (100, 4, -(1 << 40)), (-20, -5, -(1 << 40))])
def test_count_kernel_edges_match_the_oracle(ctx, start, lower, shift):
    from oracle import natac_oracle as O
    end, upper = start + 37, 12
    l, n = edge_fragments(start, end, lower, upper)
    l, start, end = l + shift, start + shift, end + shift
    n64 = n.astype(np.int64)
    ref = O.make_fragment_mat(l, n64, start, end, lower, upper)
    ins = O.get_insertions(l, n64, start, end, lower, upper)
    plus, minus = O.get_stranded_insertions(l, n64, start, end, lower, upper)
    assert ref.sum() > 0 and plus[0] > 0 and plus[-1] > 0 and minus[0] > 0 and minus[-1] > 0     # both ends of the region are hit
    assert np.array_equal(ctx.make_fragment_mat(l, n, start, end, lower, upper), ref)
    assert np.array_equal(ctx.get_insertions(l, n, start, end, lower, upper), ins)
    gp, gm = ctx.get_stranded_insertions(l, n, start, end, lower, upper)
    assert np.array_equal(gp, plus) and np.array_equal(gm, minus)


def test_insert_sizes_zero_and_one_by_hand(ctx):
    """region [10, 20), sizes [0, 3).  A size-0 fragment at 14 has its right end at 13 and its centre at 14 + floor(-1 / 2) = 13; a size-1
    fragment at 17 has both ends and its centre on 17; a size-3 fragment is filtered."""
    l, n = np.array([14, 17, 12], np.int64), np.array([0, 1, 3], np.int32)
    mat = np.zeros((3, 10))
    mat[0, 3] = 1
    mat[1, 7] = 1
    ins, plus, minus = np.zeros(10), np.zeros(10), np.zeros(10)
    ins[[3, 4]] = 1
    ins[7] = 2
    plus[[4, 7]] = 1
    minus[[3, 7]] = 1
    assert np.array_equal(ctx.make_fragment_mat(l, n, 10, 20, 0, 3), mat)
    assert np.array_equal(ctx.get_insertions(l, n, 10, 20, 0, 3), ins)
    gp, gm = ctx.get_stranded_insertions(l, n, 10, 20, 0, 3)
    assert np.array_equal(gp, plus) and np.array_equal(gm, minus)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. smooth
# ---------------------------------------------------------------------------------------------------------------------------------
def c_smooth(ctx, x, w, mode, norm):
    x, w = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(w, np.float64)
    out = np.full(len(x) - len(w) + 1 if mode == "valid" else len(x), SENTINEL)
    rc = _lib().natac_smooth(ctx._h, _vp(x), len(x), _vp(w), len(w), 0 if mode == "valid" else 1, 1 if norm else 0, _vp(out))
    return rc, out


@pytest.fixture(scope="module")
def asym():
    """a 500-value signal with a NaN stretch longer than the 61-tap window and a few single NaNs; an asymmetric positive window"""
    rng = np.random.default_rng(31)
    x = rng.normal(0, 3, 500)
    x[200:290] = np.nan
    x[[3, 57, 58, 400, 499]] = np.nan
    w = rng.random(61) + 0.05
    w[:20] *= 8.0
    return x, w


@pytest.mark.parametrize("mode", ["valid", "same"])
@pytest.mark.parametrize("norm", [True, False])
def test_smooth_orientation_with_an_asymmetric_window(ctx, asym, mode, norm):
    """the window handed to natac_smooth itself: np.convolve(w, x) orientation.  The same sums with the window reversed are far outside
    the bound, so a flipped tap index cannot pass."""
    x, w = asym
    exact, bound = R.smooth(x, w, mode, norm)
    flipped, _ = R.smooth(x, w[::-1].copy(), mode, norm)
    fin = [t for t, e in enumerate(exact) if not isinstance(e, float)]
    apart = max(abs(float(exact[t] - flipped[t])) for t in fin)
    assert apart > 1.0 and apart > 1e6 * bound.max(), apart
    assert sum(isinstance(e, float) for e in exact) >= (20 if norm else 0)       # all-NaN windows: NaN with norm
    rc, got = c_smooth(ctx, x, w, mode, norm)
    assert rc == 0
    report("smooth asymmetric %s norm=%d" % (mode, norm), R.errors(got, exact), bound)
    if not norm:                                                                # an all-NaN window sums nothing: 0.0
        m0 = 61 - 1 if mode == "valid" else 30
        hollow = [t for t in range(len(got)) if t + m0 - 60 >= 200 and t + m0 < 290]
        assert len(hollow) >= 20 and np.all(got[hollow] == 0.0)


@pytest.mark.parametrize("n,wl,window", [(9, 1, "flat"), (7, 7, "flat"), (7, 7, "gaussian"), (61, 61, "gaussian"), (300, 11, "flat"), (300, 11, "gaussian")])
def test_smooth_window_edges_through_the_wrapper(ctx, n, wl, window):
    """window_len 1, n == window_len, and 'same' at both ends of the signal (taps outside the signal are skipped), with a NaN near each
    end and an all-NaN window in the long signal; both modes, both norm values; NaN positions exactly as the formula gives them"""
    from oracle import natac_oracle as O
    rng = np.random.default_rng(100 * n + wl)
    x = rng.normal(1, 2, n)
    x[[1, n - 2]] = np.nan
    if n == 300:
        x[100:125] = np.nan
    w = np.ones(wl) if window == "flat" else O.gaussian_window(wl, (wl - 1) / 6.0 if wl > 1 else 1.0)
    for mode in ("valid", "same"):
        for norm in (True, False):
            exact, bound = R.smooth(x, w, mode, norm)
            got = ctx.smooth(x, wl, window=window, sd=None if wl > 1 else 1.0, mode=mode, norm=norm)
            assert got.shape == (n - wl + 1 if mode == "valid" else n,)
            if n == 300:
                assert (sum(isinstance(e, float) for e in exact) > 0) == norm
            report("smooth n=%d M=%d %s %s norm=%d" % (n, wl, window, mode, norm), R.errors(got, exact), bound)


def test_smooth_refusals(ctx):
    from nucleoatac_amd import _lib as L
    x = np.arange(10.0)
    rc, out = c_smooth(ctx, x, np.ones(4), "same", True)
    assert rc == -1 and _lib().natac_last_error() == b"window length must be odd (got 4)" and np.all(out == SENTINEL)
    rc, out = c_smooth(ctx, x[:3], np.ones(5), "same", True)
    assert rc == -1 and _lib().natac_last_error() == b"signal (3) shorter than the window (5)" and np.all(out == SENTINEL)
    with pytest.raises(L.NatacError, match="shorter than the window"):
        ctx.smooth(x[:4], 5, mode="same")
    with pytest.raises(L.NatacError, match="shorter than the window"):
        ctx.smooth(x[:4], 5, mode="valid")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. make_bias_mat
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bias_mat_first_rows_and_the_smallest_covering_track(ctx):
    """rows 0..3: i = 0 reads b[g + 1] + b[g], i = 1 the single cell b[g], i = 2 b[g] + b[g + 1], i = 3 b[g - 1] + b[g + 1].  The smallest
    track that covers every read is therefore [start - (upper - 2) // 2, end + (upper - 1) // 2) = [start - 1, end + 1); one value less on
    either side is refused.  A NaN, a +inf and a -inf in the track land in exactly the cells that read them."""
    from nucleoatac_amd import _lib as L
    rng = np.random.default_rng(41)
    start, end, lower, upper = 5000, 5077, 0, 4
    ts = start - (upper - 2) // 2
    b = rng.normal(0, 0.8, (end + (upper - 1) // 2) - ts)
    b[10], b[30], b[50] = np.nan, np.inf, -np.inf
    b[0], b[-1] = 1.5, -2.5
    exact, rel = R.make_bias_mat(b, ts, start, end, lower, upper)
    kinds = [e for e in exact if isinstance(e, float)]
    assert sum(np.isnan(k) for k in kinds) == 7 and sum(k == np.inf for k in kinds) == 7 and sum(k == 0.0 for k in kinds) == 7
    got = ctx.make_bias_mat(b, ts, start, end, lower, upper)
    assert got.shape == (4, 77)
    bound = np.array([r * float(e) if not isinstance(e, float) else 0.0 for r, e in zip(rel, exact)])
    report("make_bias_mat rows 0..3", R.errors(got, exact), bound)
    # the same values from a longer track (a wider margin on both sides) and from another track_start
    wide = np.concatenate([[9.0, 9.0], b, [9.0, 9.0, 9.0]])
    assert np.array_equal(ctx.make_bias_mat(wide, ts - 2, start, end, lower, upper), got, equal_nan=True)
    for short, t0 in ((b[1:], ts + 1), (b[:-1], ts)):
        with pytest.raises(L.NatacError, match="bias track does not cover"):
            ctx.make_bias_mat(short, t0, start, end, lower, upper)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. pwm_bias
# ---------------------------------------------------------------------------------------------------------------------------------
def _pwm(rng, nrow, K):
    pwm = rng.random((nrow, K)) + 0.01
    return pwm / pwm.sum(axis=0)


PWM_CASES = {
    # name: (nucleotides, K, sequence length, alphabet of the sequence, zero cell)
    "single output": ("ACGT", 21, 21, "ACGT", None),
    "three rows": ("ACG", 11, 300, "ACGT", None),
    "five rows": ("ACGTN", 11, 300, "ACGTN", None),
    "rows T G C A": ("TGCA", 21, 300, "ACGT", None),
    "foreign letter": ("ACGT", 21, 300, "ACGTRYN", None),
    "lower case": ("ACGT", 21, 300, "ACGTacgt", None),
    "zero cell": ("ACGT", 21, 300, "ACGT", (2, 7)),
}


@pytest.mark.parametrize("name", list(PWM_CASES))
def test_pwm_bias_rows_letters_and_a_zero_cell(ctx, name):
    from oracle import natac_oracle as O
    nucs, K, n, alphabet, zero = PWM_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    pwm = _pwm(rng, len(nucs), K)
    if zero:
        pwm[zero] = 0.0
    seq = "".join(rng.choice(list(alphabet), size=n))
    with np.errstate(divide="ignore"):
        logp = np.log(pwm)
        got = ctx.pwm_bias(seq, pwm, list(nucs))
    exact, bound = R.pwm_bias(seq.encode(), logp, nucs.encode())
    assert got.shape == (n - K + 1,)
    report("pwm_bias %s" % name, R.errors(got, exact), bound)
    if name == "lower case":                      # raw bytes: a lower-case letter is no row, it adds 0 as in the oracle
        up = R.pwm_bias(seq.upper().encode(), logp, nucs.encode())[0]
        assert max(abs(float(a - b)) for a, b in zip(up, exact)) > 1.0
        np.testing.assert_allclose(got, O.compute_bias_pwm(seq, pwm, list(nucs)), rtol=1e-12, atol=1e-12)
    if zero:                                      # exactly the windows that put the zero cell's letter on its column
        r, k = zero
        hit = np.array([seq[x + k] == nucs[r] for x in range(n - K + 1)])
        assert 0 < hit.sum() < len(hit) and np.array_equal(got == -np.inf, hit) and np.all(np.isfinite(got[~hit]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. correlate_valid
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R_,W,extra", [(5, 21, 0), (1, 21, 40), (7, 1, 40), (1, 1, 0), (149, 121, 257)])
def test_correlate_valid_shapes_and_a_nan(ctx, R_, W, extra):
    """ncol == W (one output), one row, a one-column template, and 258 outputs (two workgroups).  A NaN in one cell of sub makes exactly
    the outputs whose window holds it NaN."""
    rng = np.random.default_rng(1000 * R_ + W)
    vm = rng.normal(0, 1, (R_, W))
    sub = rng.normal(0, 1, (R_, W + extra))
    exact, bound = R.correlate_valid(sub, vm)
    got = ctx.correlate_valid(sub, vm)
    assert got.shape == (extra + 1,)
    report("correlate_valid R=%d W=%d ncol=%d" % (R_, W, W + extra), R.errors(got, exact), bound)
    col = (W + extra) // 2
    sub[R_ // 2, col] = np.nan
    reads = np.array([g <= col < g + W for g in range(extra + 1)])
    assert reads.sum() == min(W, extra + 1, col + 1, W + extra - col)
    exact = [float("nan") if hit else e for hit, e in zip(reads, exact)]      # the other outputs read what they read before
    got = ctx.correlate_valid(sub, vm)
    assert np.array_equal(np.isnan(got), reads)
    report("correlate_valid R=%d W=%d ncol=%d with a NaN" % (R_, W, W + extra), R.errors(got, exact), bound)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. calculate_occupancy
# ---------------------------------------------------------------------------------------------------------------------------------
def occ_model(kind):
    from nucleoatac_amd.synth import synth_occ_distributions
    nucp, nfrp = synth_occ_distributions(251)
    if kind == "128 alphas":
        return nucp, nfrp, np.linspace(0, 1, 128)
    if kind == "one alpha":
        return nucp, nfrp, np.array([0.5])
    nfrp = nfrp.copy()
    nfrp[170:] = 0.0
    return nucp, nfrp / nfrp.sum(), np.linspace(0, 1, 101)


def occ_windows(rng):
    dense = rng.integers(0, 4, 251).astype(np.float64) * (rng.random(251) < 0.3)
    one = np.zeros(251)
    one[140] = 1.0
    return {"dense": dense, "one fragment": one, "all zero": np.zeros(251)}


@pytest.mark.parametrize("kind", ["128 alphas", "one alpha", "model zeros"])
def test_calculate_occupancy_model_grids(kind):
    """128 alphas fill the kernel's ll[128]; one alpha; 101 alphas over a model with zeros.  Each with a dense window, a one-fragment
    window and an empty one.  Every case is first shown, on mpmath log-likelihoods, to be decided by a margin of 1e-9: the argmax
    and every likelihood-ratio comparison, so that the triple cannot depend on the order of an fp64 sum."""
    from nucleoatac_amd.device import Context
    from oracle import natac_oracle as O
    nucp, nfrp, alphas = occ_model(kind)
    rng = np.random.default_rng(len(kind))
    bias = np.exp(rng.normal(0, 1, 251))
    with Context(0) as c:
        c.set_occ_model(nucp, nfrp, alphas=alphas, cutoff=CUTOFF, step=5, flank=60)
        for name, ins in occ_windows(rng).items():
            ll, scale = R.occupancy_logliks(ins, bias, nucp, nfrp, alphas)
            assert R.occupancy_is_decided(ll, scale, CUTOFF), (kind, name)
            ref = O.calculate_occupancy(ins, bias, nucp, nfrp, alphas, CUTOFF)
            if name == "all zero":
                # every likelihood is an exact 0, except at an alpha whose mixture is 0 at some size (0 * log 0: -inf).  The first of the
                # tied maxima wins, and every tied alpha passes the ratio test.  Only alpha = 0 over a model with nfr zeros is shut out.
                first = alphas[1] if kind == "model zeros" else alphas[0]
                assert tuple(ref) == (first, first, alphas[-1])
            got = c.calculate_occupancy(ins, bias)
            print("calculate_occupancy %s / %s: %r" % (kind, name, got))
            assert tuple(got) == tuple(float(x) for x in ref), (kind, name, got, ref)


def test_calculate_occupancy_refuses_other_lengths():
    """the C entry reads the model's `upper` values of each operand: the wrapper refuses any other length before a native call"""
    from nucleoatac_amd.device import Context
    nucp, nfrp, alphas = occ_model("128 alphas")
    with Context(0) as c:
        c.set_occ_model(nucp, nfrp, alphas=alphas, cutoff=CUTOFF)
        calls = []
        real = c._lib
        c._lib = type("NoNative", (), {"__getattr__": lambda self, k: calls.append(k) or getattr(real, k)})()
        try:
            for ni, nb in ((250, 251), (251, 250), (252, 251), (251, 252), (0, 0), (502, 502)):
                with pytest.raises(ValueError, match="251 values"):
                    c.calculate_occupancy(np.ones(ni), np.ones(nb))
            with pytest.raises(ValueError, match="251 values"):
                c.calculate_occupancy(np.ones((1, 251)), np.ones(251))
            assert calls == []
            c.calculate_occupancy(np.ones(251), np.ones(251))
            assert "natac_calculate_occupancy" in calls
        finally:
            c._lib = real


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. refusals of a negative size
# ---------------------------------------------------------------------------------------------------------------------------------
def test_negative_sizes_are_refused_before_any_device_work(ctx):
    """n_frags < 0 in the three fragment calls and nb < 0 in natac_make_bias_mat: NATAC_E_ARG "negative size", outputs as they were"""
    lib, h = _lib(), ctx._h
    l, n, b = np.array([12], np.int64), np.array([3], np.int32), np.zeros(40)
    for nf in (-1, -(1 << 40)):
        mat = np.full(5 * 10 + 2, SENTINEL)
        assert lib.natac_make_fragment_mat(h, nf, _vp(l), _vp(n), 10, 20, 0, 5, _vp(mat)) == -1
        assert lib.natac_last_error() == b"negative size" and np.all(mat == SENTINEL)
        out = np.full(12, SENTINEL)
        assert lib.natac_get_insertions(h, nf, _vp(l), _vp(n), 10, 20, 0, 5, _vp(out)) == -1
        assert lib.natac_last_error() == b"negative size" and np.all(out == SENTINEL)
        plus, minus = np.full(12, SENTINEL), np.full(12, SENTINEL)
        assert lib.natac_get_stranded_insertions(h, nf, _vp(l), _vp(n), 10, 20, 0, 5, _vp(plus), _vp(minus)) == -1
        assert lib.natac_last_error() == b"negative size" and np.all(plus == SENTINEL) and np.all(minus == SENTINEL)
        mat = np.full(5 * 10 + 2, SENTINEL)
        assert lib.natac_make_bias_mat(h, _vp(b), nf, 0, 10, 20, 0, 5, _vp(mat)) == -1
        assert lib.natac_last_error() == b"negative size" and np.all(mat == SENTINEL)
    # the accepting side of the same calls: no fragments gives zeros, and the context still works
    assert lib.natac_get_insertions(h, 0, _vp(l), _vp(n), 10, 20, 0, 5, _vp(out)) == 0 and np.all(out[:10] == 0.0) and np.all(out[10:] == SENTINEL)
    assert np.array_equal(ctx.get_insertions(l, n, 10, 20, 0, 5), np.array([0, 0, 1, 0, 1, 0, 0, 0, 0, 0], np.float64))
