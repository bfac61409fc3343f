"""A high-precision restatement of one occupancy grid point (tests only; plain Python / numpy, no GPU).

calculateOccupancy (nucleoatac/Occupancy.py:104-120), as oracle.natac_oracle.calculate_occupancy restates it in fp64, evaluated in
np.longdouble where that is the x87 80-bit format (64-bit significand) and in mpmath at 100 bits elsewhere.  It keeps the reference's
rule `0 * log 0 = NaN -> -inf` (Occupancy.py:112-114): an alpha for which SOME insert size has mixture probability 0 -- alpha = 0 with a
zero nfr_prob, 1 - alpha = 0 with a zero nuc_prob -- has log-likelihood -inf for every window, with or without a fragment of that size.

Besides the three alpha indices a grid point gets a DECISION MARGIN, the smaller of
  * the gap between the best and the second-best finite log-likelihood, and
  * min_a |2 (llmax - ll_a) - cutoff| over the finite a,
and counts as DECIDED when the margin exceeds DECIDED_REL * (1 + |llmax|).  The fp64 sum of at most 251 logarithms is good to about
251 * 2^-53 |ll| ~ 3e-14 |ll|, the product-domain kernels to about (fragments * 2^-53); 1e-10 is more than three orders of magnitude
above both, so a decided point has one right answer in any sane arithmetic and an implementation may be held to it bit for bit."""
import numpy as np

DECIDED_REL = 1e-10
USE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63


def _logliks_longdouble(ins, bias, nuc_probs, nfr_probs, alphas):
    ld = np.longdouble
    b = bias.astype(ld)
    pn = nuc_probs.astype(ld) * b
    pn = pn / pn.sum()
    pf = nfr_probs.astype(ld) * b
    pf = pf / pf.sum()
    al = alphas.astype(ld)
    be = (1 - alphas).astype(ld)                      # 1 - alpha as the reference forms it (fp64): its zero is the reference's zero
    mix = al[:, None] * pn[None, :] + be[:, None] * pf[None, :]
    dead = (mix == 0).any(axis=1)
    use = ins > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        ll = np.log(mix[:, use]) @ ins[use].astype(ld)
    ll[dead | np.isnan(ll)] = -np.inf
    return ll


def _logliks_mpmath(ins, bias, nuc_probs, nfr_probs, alphas):
    import mpmath
    with mpmath.workprec(100):
        mpf = mpmath.mpf
        b = [mpf(x) for x in bias]
        pn = [mpf(float(p)) * x for p, x in zip(nuc_probs, b)]
        pf = [mpf(float(p)) * x for p, x in zip(nfr_probs, b)]
        sn, sf = mpmath.fsum(pn), mpmath.fsum(pf)
        pn = [p / sn for p in pn]
        pf = [p / sf for p in pf]
        use = [j for j in range(len(ins)) if ins[j] > 0]
        out = []
        for a in alphas:
            al, be = mpf(float(a)), mpf(float(1 - a))
            mix = [al * p + be * q for p, q in zip(pn, pf)]
            if any(m == 0 for m in mix):
                out.append(-mpmath.inf)
            else:
                out.append(mpmath.fsum(mpmath.log(mix[j]) * mpf(float(ins[j])) for j in use))
        return out


def grid_point(ins, bias, nuc_probs, nfr_probs, alphas, cutoff):
    """(imax, ilo, ihi, margin, llmax) of one window: `ins` / `bias` are its per-insert-size fragment counts and bias sums.  The indices
    are those of calculateOccupancy's occ / lower / upper in `alphas`; margin and llmax are Python floats."""
    fn = _logliks_longdouble if USE_LONGDOUBLE else _logliks_mpmath
    ll = fn(np.asarray(ins), np.asarray(bias), np.asarray(nuc_probs, dtype=np.float64), np.asarray(nfr_probs, dtype=np.float64),
            np.asarray(alphas, dtype=np.float64))
    finite = [a for a in range(len(ll)) if ll[a] != -np.inf]
    if not finite:
        raise ValueError("every log-likelihood is -inf (the reference raises, Occupancy.py:118)")
    llmax = max(ll[a] for a in finite)
    imax = next(a for a in finite if ll[a] == llmax)
    ratios = {a: 2 * (llmax - ll[a]) for a in finite}
    inside = [a for a in finite if ratios[a] < cutoff]
    second = [llmax - ll[a] for a in finite if a != imax]
    gap = float(min(second)) if second else float("inf")
    edge = float(min(abs(ratios[a] - cutoff) for a in finite))
    return imax, min(inside), max(inside), min(gap, edge), float(llmax)


def chunk_reference(mat, b0, nuc_probs, nfr_probs, alphas, cutoff, L, step, flank):
    """every grid point of one chunk.  mat / b0: the fragment and bias matrices of oracle.natac_oracle.occ_chunk_tracks (insert sizes x
    bases from start - flank on).  Returns a dict of arrays over the chunk's grid points i = halfstep, halfstep + step, ... < L:
    idx int[nk, 3] (imax, ilo, ihi; -1 where the window holds no fragment: NaN in the reference), margin, llmax and decided."""
    halfstep = (step - 1) // 2
    pts = range(halfstep, L, step)
    nk = len(pts)
    idx = np.full((nk, 3), -1, dtype=np.int64)
    margin = np.full(nk, np.nan)
    llmax = np.full(nk, np.nan)
    W = 2 * flank + 1
    hp = np.longdouble if USE_LONGDOUBLE else np.float64      # mpmath: the 121-term sums of positive fp64 values are formed below
    for k, i in enumerate(pts):
        ins = mat[:, i:i + W].sum(axis=1)
        if ins.sum() > 0:
            if USE_LONGDOUBLE:
                bias = b0[:, i:i + W].astype(hp).sum(axis=1)
            else:
                import mpmath
                with mpmath.workprec(100):
                    bias = np.array([mpmath.fsum(map(float, row)) for row in b0[:, i:i + W]], dtype=object)
            a, lo, hi, margin[k], llmax[k] = grid_point(ins, bias, nuc_probs, nfr_probs, alphas, cutoff)
            idx[k] = (a, lo, hi)
    decided = margin > DECIDED_REL * (1 + np.abs(llmax))       # False at the NaN points
    return dict(idx=idx, margin=margin, llmax=llmax, decided=decided, live=idx[:, 0] >= 0)


def tile_fragments(lpos, ilen, tile, step, flank, upper):
    """natac_occ_tile_ranges restated: (t0, t1, n_valid) of tile `tile` (64 consecutive grid points) of a chunk whose fragments
    lpos / ilen are sorted by centre.  [t0, t1) are the fragments with a centre in [gfirst - flank, gfirst + 63 step + flank],
    gfirst = halfstep + 64 tile step; valid ones have 0 <= ilen < upper.  More than 512 valid fragments: natac_occ_decide reads the
    tile's fragments from global memory instead of staging them."""
    lpos, ilen = np.asarray(lpos, dtype=np.int64), np.asarray(ilen, dtype=np.int64)
    centre = lpos + (ilen - 1) // 2
    assert np.all(np.diff(centre) >= 0), "fragments must be sorted by centre"
    gfirst = (step - 1) // 2 + 64 * tile * step
    t0 = int(np.searchsorted(centre, gfirst - flank, "left"))
    t1 = int(np.searchsorted(centre, gfirst + 63 * step + flank + 1, "left"))
    n = ilen[t0:t1]
    return t0, t1, int(np.count_nonzero((n >= 0) & (n < upper)))
