"""Exact restatements of the single-region drop-ins' floating outputs (csrc/natac_dropins.hpp), for tests/test_gpu_dropins.py.

Every value is computed from the same fp64 inputs the device gets, without a rounding: a double is an integer times a power of two, so
a sum of products of doubles is an integer dot product over a common scale (Python integers, exact at any length), which mpmath then
holds at 256 bits for the one division, exp or log that follows.  A function returns the exact values as mpmath numbers (or the float
NaN / +-inf where the formula gives one) and the magnitude its error bound is stated in; `errors` measures a device result against
them in mpmath, so the reference's own rounding never enters."""
import mpmath as mp
import numpy as np

mp.mp.prec = 256
U = 2.0 ** -52


def scaled(x):
    """(object array of Python integers, k) with x == integers / 2^k exactly; x finite"""
    x = np.asarray(x, np.float64)
    assert np.all(np.isfinite(x))
    m, e = np.frexp(x.ravel())
    mant = (m * 2.0 ** 53).astype(np.int64)                       # exact: |m| < 1 has 53 bits
    sh = 53 - e.astype(np.int64)
    k = int(sh[mant != 0].max()) if np.any(mant != 0) else 0
    out = np.array([(mi << (k - s)) if mi else 0 for mi, s in zip(mant.tolist(), sh.tolist())], dtype=object)
    return out.reshape(x.shape), k


def unscale(i, k):
    return mp.mpf(int(i)) / mp.mpf(2) ** k


def errors(got, exact):
    """|got - exact| per element, the difference taken in mpmath; positions where either is not finite are compared outright"""
    got = np.asarray(got, np.float64).ravel()
    assert len(got) == len(exact), (len(got), len(exact))
    err = np.zeros(len(got))
    for t, (g, e) in enumerate(zip(got.tolist(), exact)):
        if isinstance(e, float) and not np.isfinite(e):
            assert (np.isnan(g) and np.isnan(e)) or g == e, "output %d is %r, the formula gives %r" % (t, g, e)
        else:
            assert np.isfinite(g), "output %d is %r, the formula gives %s" % (t, g, mp.nstr(e, 17))
            err[t] = float(abs(mp.mpf(g) - e))
    return err


def smooth(x, w, mode, norm):
    """utils.smooth in np.convolve(w, x) orientation: full[m] = sum_k w[k] x[m - k] over the taps inside x that are not NaN;
    'valid' takes m = t + M-1, 'same' m = t + (M-1)//2.  norm: divided by the sum of the weights that met a value (none: NaN).
    Returns (exact, bound): (M + 1) U A without norm and (2M + 4) U A / den with it, A = sum |w[k] x[m - k]|."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, M = len(x), len(w)
    ok = ~np.isnan(x)
    xi, kx = scaled(np.where(ok, x, 0.0))
    wi, kw = scaled(w)
    wa = np.array([abs(int(v)) for v in wi], dtype=object)
    xa = np.array([abs(int(v)) for v in xi], dtype=object)
    nout = n - M + 1 if mode == "valid" else n
    exact, bound = [], np.zeros(nout)
    for t in range(nout):
        m = t + (M - 1 if mode == "valid" else (M - 1) // 2)
        ks = [k for k in range(M) if 0 <= m - k < n and ok[m - k]]
        idx = [m - k for k in ks]
        num = unscale(sum(wi[k] * xi[i] for k, i in zip(ks, idx)), kx + kw)
        A = unscale(sum(wa[k] * xa[i] for k, i in zip(ks, idx)), kx + kw)
        if not norm:
            exact.append(num)
            bound[t] = float((M + 1) * U * A)
            continue
        den = unscale(sum(wi[k] for k in ks), kw)
        if den == 0:
            exact.append(float("nan"))
        else:
            exact.append(num / den)
            bound[t] = float((2 * M + 4) * U * A / abs(den))
    return exact, bound


def pwm_bias(seq, logp, nucs):
    """out[x] = sum_k logp[row(seq[x + k]), k] over the letters that are a row of the PWM (bytes compared as they are).  A -inf cell under
    the window gives -inf.  Returns (exact, bound) with bound = (T + 1) U sum |term|, T the number of terms of that output."""
    seq = np.frombuffer(bytes(seq), dtype=np.uint8)
    logp = np.asarray(logp, np.float64)
    nrow, K = logp.shape
    assert len(nucs) == nrow and not np.any(np.isnan(logp)) and not np.any(logp == np.inf)
    li, kl = scaled(np.where(np.isfinite(logp), logp, 0.0))
    exact, bound = [], np.zeros(len(seq) - K + 1)
    for x in range(len(seq) - K + 1):
        cells = [(r, k) for k in range(K) for r in range(nrow) if seq[x + k] == nucs[r]]
        if any(logp[c] == -np.inf for c in cells):
            exact.append(-float("inf"))
            continue
        exact.append(unscale(sum(li[c] for c in cells), kl))
        bound[x] = float((len(cells) + 1) * U * unscale(sum(abs(li[c]) for c in cells), kl))
    return exact, bound


def correlate_valid(sub, vm):
    """out[g] = sum_r sum_c sub[r, g + c] vm[r, c]; a NaN of sub makes the outputs that read it NaN.  bound = (R W + 1) U sum |term|."""
    sub, vm = np.asarray(sub, np.float64), np.asarray(vm, np.float64)
    R, W = vm.shape
    nan = np.isnan(sub)
    si, ks = scaled(np.where(nan, 0.0, sub))
    vi, kv = scaled(vm)
    sa, va = np.abs(si), np.abs(vi)
    nout = sub.shape[1] - W + 1
    exact, bound = [], np.zeros(nout)
    for g in range(nout):
        if nan[:, g:g + W].any():
            exact.append(float("nan"))
            continue
        exact.append(unscale((si[:, g:g + W] * vi).sum(), ks + kv))
        bound[g] = float((R * W + 1) * U * unscale((sa[:, g:g + W] * va).sum(), ks + kv))
    return exact, bound


def make_bias_mat(b, track_start, start, end, lower, upper):
    """mat[i - lower, x] = exp(b[g - (i-1)//2] + b[g + i//2]), g = start + x - track_start, and exp(b[g]) in the i == 1 row.  Returns
    (exact, relbound) flattened row-major; a NaN, +inf or -inf of the track gives NaN, inf and 0.0 (as floats in `exact`).  relbound =
    (4 + |b_l + b_r|) U: 4 ulp for the device exp, the rest for the rounded sum in its argument (an error d of the argument is a relative
    error d of the exponential); 4 U in the i == 1 row, which adds nothing."""
    b = np.asarray(b, np.float64)
    exact, rel = [], []
    for i in range(lower, upper):
        for x in range(end - start):
            g = start + x - track_start
            jl, jr = g - (i - 1) // 2, g + i // 2
            assert 0 <= jl < len(b) and 0 <= jr < len(b), "the track does not cover row %d column %d" % (i, x)
            with np.errstate(invalid="ignore"):
                s = float(b[jl]) if jl == jr else float(b[jl] + b[jr])
            if not np.isfinite(s):
                exact.append(float("nan") if np.isnan(s) else (float("inf") if s > 0 else 0.0))
                rel.append(0.0)
            elif jl == jr:
                exact.append(mp.exp(mp.mpf(float(b[jl]))))
                rel.append(4 * U)
            else:
                a = mp.mpf(float(b[jl])) + mp.mpf(float(b[jr]))
                exact.append(mp.exp(a))
                rel.append((4 + abs(float(a))) * U)
    return exact, np.array(rel)


def cov_sums(p, v):
    """exact S1 = sum p v^2, S2 = sum p v, Q = sum p^2 v^2 and their absolute-value versions A1 = sum |p v^2|, A2 = sum |p v|"""
    pi, kp = scaled(p)
    vi, kv = scaled(v)
    pv = pi * vi
    S1, S2 = unscale((pv * vi).sum(), kp + 2 * kv), unscale(pv.sum(), kp + kv)
    Q = unscale((pv * pv).sum(), 2 * kp + 2 * kv)
    A1, A2 = unscale((np.abs(pv) * np.abs(vi)).sum(), kp + 2 * kv), unscale(np.abs(pv).sum(), kp + kv)
    return S1, S2, Q, A1, A2


def calculate_cov(p, v, r, literal):
    """calculateCov: r (S1 - S2^2) exactly -- the literal pair sum, sum_i p_i (1 - p_i) v_i^2 - 2 sum_{i<j} p_i p_j v_i v_j, is the same
    number.  Returns (exact, bound, condition): closed (2n + 6) 2U r (A1 + A2^2); literal (n (n+1) / 2 + 6) 2U r sum |term| over the
    diagonal and upper-triangle terms, which for 0 <= p <= 1 is (S1' - Q) + (A2^2 - Q) with S1' = A1; condition = (A1 + A2^2) / |S1 - S2^2|."""
    p, v = np.asarray(p, np.float64), np.asarray(v, np.float64)
    assert np.all(p >= 0) and np.all(p <= 1)
    n = len(p)
    S1, S2, Q, A1, A2 = cov_sums(p, v)
    exact = r * (S1 - S2 * S2)
    if literal:
        bound = (n * (n + 1) // 2 + 6) * 2 * U * r * ((A1 - Q) + (A2 * A2 - Q))
    else:
        bound = (2 * n + 6) * 2 * U * r * (A1 + A2 * A2)
    return exact, float(bound), float((A1 + A2 * A2) / abs(S1 - S2 * S2))


def occupancy_logliks(inserts, bias, nuc_probs, nfr_probs, alphas):
    """calculateOccupancy's log-likelihoods in mpmath: ll[a] = sum_j inserts[j] log(alpha pn[j] + (1 - alpha) pf[j]), pn and pf the model
    times the bias, normalised.  A mixture that is 0 at any size makes the sum NaN or -inf, which the reference turns into -inf, whatever
    inserts holds there.  Returns (ll, scale): scale = the largest sum_j |inserts[j] log(...)|, the magnitude a rounding of the fp64
    evaluations is relative to (0 when inserts is all zero: every finite ll is then an exact 0 in any arithmetic)."""
    f = lambda a: [mp.mpf(float(x)) for x in np.asarray(a, np.float64)]      # noqa: E731
    ins, b, nu, nf = f(inserts), f(bias), f(nuc_probs), f(nfr_probs)
    pn, pf = [x * y for x, y in zip(nu, b)], [x * y for x, y in zip(nf, b)]
    sn, sf = mp.fsum(pn), mp.fsum(pf)
    pn, pf = [x / sn for x in pn], [x / sf for x in pf]
    ll, scale = [], mp.mpf(0)
    for al in f(alphas):
        mix = [al * x + (1 - al) * y for x, y in zip(pn, pf)]
        if any(m == 0 for m in mix):
            ll.append(-mp.inf)
            continue
        terms = [i * mp.log(m) for i, m in zip(ins, mix) if i != 0]
        ll.append(mp.fsum(terms))
        scale = max(scale, mp.fsum(abs(t) for t in terms))
    return ll, scale


def occupancy_is_decided(ll, scale, cutoff, margin=1e-9):
    """True when the argmax and every 2 (max - ll) < cutoff decision sit at least `margin` (relative to the likelihoods' magnitude, and to
    the cutoff) away from their thresholds, so fp64 evaluations in any order take the same decisions.  With scale == 0 ties are exact."""
    mx = max(ll)
    if mx == -mp.inf:
        return False
    im = ll.index(mx)
    for k, v in enumerate(ll):
        if v == -mp.inf:
            continue
        if scale > 0 and k != im and mx - v < margin * scale:
            return False
        if abs(2 * (mx - v) - cutoff) < margin * max(scale, mp.mpf(cutoff)):
            return False
    return True
