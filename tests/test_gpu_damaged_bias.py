"""The data-selected arms of the nucleosome stage -- the ones a candidate takes only when its bias window holds a non-finite, zero or very
small exp(bias) -- against the oracle: lr / var / z of every candidate kernel, the second launch site (run_peaks), the per-base tracks
with the NaN-aware smoothing, and the window-probability route (run_candidates_cov).

natac_candidates_paired and natac_candidates4 run the exact zero-cell test (lr = NaN where a model cell is 0) only in waves whose window
minimum of exp(bias) is not above 2^-500 (`esmall`); natac_candidates always runs it.  The reference's rule: a zero model cell anywhere in
the window gives lr = NaN (log(0) * 0) while var and z stay finite; a NaN in the window makes all three NaN.

One batch per V-plot geometry, one chunk per kind of damage.  Every chunk has the same fragments and the same base bias, normal(0, 0.7),
and one edit at base `a` (or two, `a` and `a + d`).  With w = W // 2, A = (upper - 2) >> 1, Bh = (upper - 1) >> 1 an insert size i pairs the
bases x - (i-1)//2 and x + i//2, so two damaged bases at distance d form the single cell i = d + 1, x = a + (i-1)//2:

    control     none                                           all finite
    tiny-1      b[a] = -400                                    all finite; esmall is true and no cell is zero
    tiny-2-in   b[a] = b[a+d] = -400, d + 1 = lower,           lr NaN exactly for |p - x| <= w (W positions); var, z finite
                (lower + upper) // 2 (150 for 105..251), upper - 1
    tiny-2-out  the same with d + 1 = upper and lower - 1      all finite: the cell lies outside the V-plot
    zero        b[a] = -inf                                    lr NaN exactly for a - w - Bh <= p <= a + w + A; var, z, bg, norm finite
    nan         b[a] = nan                                     lr, var, z, bg, norm NaN on that span; smoothed on 60 bases fewer
    nan-ends    NaN in both bias flanks                        norm NaN over the first 90 and the last 85 bases of the chunk
    range       b[a-20:a+20] += 25                             all finite

Fragments sit on the damaged cells (several with an end at `a`, one on each tiny-2-in cell), so the reference's per-fragment terms really
carry the logarithm of a 1e-174 or zero probability.  |b| <= 700 and no -inf next to large positive values: the oracle's exp(b1 + b2) and
the device's exp(b1) * exp(b2) then agree to rounding.  No template or size-distribution zeros, so the documented -inf / NaN deviation
 cannot occur and no candidate is left out of any comparison.

test_oracle_gives_the_table needs no GPU: it holds the oracle half of this file to the table above."""
import functools
import os

import numpy as np
import pytest

from helpers import _assert_stat, _assert_stats, _reference_stats, assert_track, cancel_scale
from nucleoatac_amd import _lib as L
from nucleoatac_amd.packing import PackedChunks
from nucleoatac_amd.synth import synth_centres, synth_size_distribution, synth_sizes
from test_gpu_vplot_arms import BL, BR, PEAKS, _vmat

gpu = pytest.mark.gpu

A_BASE = 400           # the damaged base: near the middle of the chunk, 16 or more bases from the border of its two background tiles
TINY = -400.0          # exp(-400) = 1.9e-174 < 2^-500 = 3.1e-151; a product of two such values underflows to 0, one of them times
                       # exp(normal(0, 0.7)) does not
NAN_HEAD, NAN_TAIL = 90, 85    # bases of norm the nan-ends chunk loses at its two ends: more than w + 10 (candidates see them) and more
                               # than the smoothing's half width of 30 (smoothed loses its first 60 and last 55 bases too)
SMOOTH_SD = 10
ESMALL = 2.0 ** -500   # the kernels' threshold: no product of two window values can underflow to 0 above it
TRACKS = (L.T_BACKGROUND, L.T_NORM, L.T_SMOOTH)

# lower, upper, w, the candidate kernel launch_candidates picks, validation switches to run on top of it
GEOMETRIES = [
    pytest.param(105, 251, 60, id="105-251-w60"),      # natac_candidates_paired<true>; NATAC_CAND_OLD / _FULL: natac_candidates4<true> / <false>
    pytest.param(110, 250, 60, id="110-250-w60"),      # natac_candidates_paired<false>
    pytest.param(105, 250, 63, id="105-250-w63"),      # natac_candidates4<true>: odd row count, the R % 4 tail rows go through row_generic
    pytest.param(40, 140, 64, id="40-140-w64"),        # natac_candidates
]
SWITCHES = {(105, 251, 60): ("NATAC_CAND_OLD", "NATAC_CAND_FULL")}
# the longest chunk of about 900 bases whose FFT background tiling has extended tiles (natac_bg_tiling: two extended tiles of
# 512 - W + 1 + 32 bases); the GPU tests check it with ctx.bg_tiling
CHUNK_LEN = {121: 848, 127: 836, 129: 832}


def _half(up):
    return (up - 2) >> 1, (up - 1) >> 1


def _kinds(lo, up, w, Lc):
    """[(name, edit(bias of the chunk, index of base 0), damaged bases, cell centre x or None)]"""
    A, Bh = _half(up)
    a = A_BASE
    kinds = [("control", {}, None), ("tiny-1", {a: TINY}, None)]
    for name, i in (("tiny-2-in-lower", lo), ("tiny-2-in-mid", (lo + up) // 2), ("tiny-2-in-last", up - 1)):
        kinds.append((name, {a: TINY, a + i - 1: TINY}, a + (i - 1) // 2))
    for name, i in (("tiny-2-out-upper", up), ("tiny-2-out-below", lo - 1)):
        kinds.append((name, {a: TINY, a + i - 1: TINY}, None))
    kinds.append(("zero", {a: -np.inf}, None))
    kinds.append(("nan", {a: np.nan}, None))
    # norm[p] is NaN for a - w - Bh <= p <= a + w + A: the first NAN_HEAD bases for a = NAN_HEAD - 1 - w - A, the last NAN_TAIL for the mirror
    kinds.append(("nan-ends", {NAN_HEAD - 1 - w - A: np.nan, Lc - NAN_TAIL + w + Bh: np.nan}, None))
    kinds.append(("range", {j: 25.0 for j in range(a - 20, a + 20)}, None))
    return kinds


class Case:
    """the batch of one geometry, its candidates and what the oracle gives for them (no GPU)"""

    def __init__(self, lo, up, w):
        from oracle import natac_oracle as O
        self.lo, self.up, self.w, self.W = lo, up, w, 2 * w + 1
        self.vm = _vmat(lo, up, w, False)
        self.sizes = synth_size_distribution(max(up, 251))[:up]
        self.Lc = Lc = CHUNK_LEN[self.W]
        A, Bh = _half(up)
        assert BL >= w + A + 2 and BR >= w + Bh + 2 and BL >= self.W + Bh     # every candidate window and the oracle's matrices stay in the flanks
        self.kinds = _kinds(lo, up, w, Lc)
        self.names = [k[0] for k in self.kinds]
        nc = len(self.kinds)
        rng = np.random.default_rng(lo * 7 + up + w)
        # the same fragments in every chunk, three per base: every insert size of the V-plot and beyond, half of them nucleosome-like;
        # phased centres from -150 to Lc + 100 (the peak search then finds a candidate every 90 bases or so)
        nf = 3 * Lc
        n = np.where(rng.random(nf) < 0.5, synth_sizes(rng, nf), rng.integers(1, up + 20, size=nf))
        c = synth_centres(rng, nf, Lc + 250, period=90, band=3, enrich=8.0) - 150
        l = c - (n - 1) // 2
        a = A_BASE
        mid = (lo + up) // 2
        # planted: ends at `a` (left ends and right ends; tiny-1), and one fragment on the cell of each tiny-2-in chunk
        pl = [a, a, a, a - (lo + 10) + 1, a - (up - 10) + 1, a, a, a]
        pn = [lo + 10, mid + 7, up - 10, lo + 10, up - 10, lo, mid, up - 1]
        l, n = np.concatenate((l, pl)), np.concatenate((n, pn))
        o = np.argsort(l + (n - 1) // 2, kind="stable")
        self.l, self.n = l[o].astype(np.int64), n[o].astype(np.int64)
        assert len(self.l) >= 2 * Lc
        base = rng.normal(0, 0.7, size=Lc + BL + BR)
        bias = np.tile(base, nc)
        nb = Lc + BL + BR
        self.damaged = []
        for k, (name, edit, x) in enumerate(self.kinds):
            for j, v in edit.items():
                assert -BL <= j < Lc + BR
                if name == "range":
                    bias[k * nb + BL + j] += v
                else:
                    bias[k * nb + BL + j] = v
            self.damaged.append(sorted(edit))
        fin = bias[np.isfinite(bias)]
        assert np.abs(fin).max() <= 700
        self.pk = PackedChunks(np.arange(nc) * 20000, [Lc] * nc, np.arange(nc + 1) * len(self.l), np.tile(self.l, nc), np.tile(self.n, nc),
                               np.arange(nc + 1) * nb, bias, bias_left=BL, bias_right=BR)
        # candidates: every position within w + upper // 2 + 20 of a damaged base, every 7th elsewhere, the first and the last
        first, last = w + 10, Lc - w - 11
        assert first - w - A < 0 and last + w + Bh >= Lc                           # their windows reach into both bias flanks
        cc, cp = [], []
        for k in range(nc):
            take = np.zeros(Lc, bool)
            take[first:last + 1:7] = True
            take[[first, last]] = True
            for j in self.damaged[k]:
                take[max(first, j - (w + up // 2 + 20)):max(first, min(last, j + (w + up // 2 + 20)) + 1)] = True
            take[:first] = False
            take[last + 1:] = False
            pos = np.flatnonzero(take)
            cc += [k] * len(pos)
            cp += list(pos)
        if len(cc) % 4 == 0:                                                       # the last wave has a tail
            cc.append(0)
            cp.append(first + 1)
        self.cc, self.cp = np.array(cc, np.int32), np.array(cp, np.int32)
        assert len(self.cc) % 4 != 0 and len(self.cc) % 16 != 0
        # ---- the oracle
        self.nts = []
        with np.errstate(all="ignore"):
            for k in range(nc):
                self.nts.append(O.nuc_chunk_tracks(self.l, self.n, 0, Lc, self.pk.chunk_bias(k), -BL, self.vm, lo, up, self.sizes,
                                                   smooth_sd=SMOOTH_SD))
            self.ref, self.scales = self.reference(self.cc, self.cp)
        # minimum of exp(bias) over each candidate's window [p - w - A, p + w + Bh] (what the per-wave kernels test against 2^-500)
        e = np.exp(bias)
        self.emin = np.array([np.nanmin(e[k * nb + BL + p - w - A:k * nb + BL + p + w + Bh + 1]) for k, p in zip(cc, cp)])
        self.enan = np.array([np.isnan(e[k * nb + BL + p - w - A:k * nb + BL + p + w + Bh + 1]).any() for k, p in zip(cc, cp)])

    def reference(self, cc, cp):
        """_reference_stats, with the floor of z on the range chunk following the floor of var.  There one cell of e^50 can hold all but
        1e-7 of a window's probability, var = r (sum p v^2 - (sum p v)^2) cancels to 1e-10 and less, and the oracle's own fp64 closed form
        is off by up to 2e-8 of it (against the same sums in long double).  var keeps its floor of TIGHT_ATOL; but z = norm / sqrt(var)
        cannot be held tighter than its operand: an error dv of var moves z by |z| dv / (2 var).  dv is taken relative to the largest
        term r p v^2 of the oracle's window sum (cancel_scale's idea; below 1, the scale var itself is compared with), so z's scale
        grows by |z| / (2 var) * r max(p v^2) -- all of it from the oracle's operands, nothing from the device."""
        from oracle import natac_oracle as O
        ref, (lr_scale, var_scale, z_scale) = _reference_stats(self.nts, self.vm, self.lo, self.up, cc, cp)
        k = self.names.index("range")
        nt = self.nts[k]
        v2 = np.ravel(self.vm) ** 2
        z_scale = z_scale.copy()
        for j in np.flatnonzero(np.asarray(cc) == k):
            p, var, z = int(cp[j]), ref[1][j], ref[2][j]
            if var > 0 and np.isfinite(z):
                pr = O.signal_distribution_probs(nt["bmat"], nt["b_start"], self.lo, self.up, self.w, p)
                term = int(nt["nuc_cov"][p]) * float(np.max(pr * v2))
                assert term <= 1.0
                z_scale[j] += abs(z) / (2 * var) * term
        return ref, (lr_scale, var_scale, z_scale)

    def of(self, name):
        """mask of the candidates of the chunk `name`"""
        return self.cc == self.names.index(name)

    def in_span(self, name):
        """mask of the candidates of chunk `name` whose bias window holds a damaged base"""
        A, Bh = _half(self.up)
        m = np.zeros(len(self.cc), bool)
        for j in self.damaged[self.names.index(name)]:
            m |= self.of(name) & (self.cp - self.w - A <= j) & (j <= self.cp + self.w + Bh)
        return m

    def cov_sample(self):
        """8 candidates per kind for the window-probability route: inside the damaged span where there is one"""
        idx = []
        for name in self.names:
            m = self.in_span(name) if self.damaged[self.names.index(name)] else self.of(name)
            j = np.flatnonzero(m)
            idx += list(j[np.linspace(0, len(j) - 1, 8).astype(int)])
        return np.array(idx)


@functools.lru_cache(maxsize=None)
def case(lo, up, w):
    return Case(lo, up, w)


def check_oracle_table(cs):
    """the table of the module docstring, from the oracle alone (no GPU): spans come from the geometry's own w, A, Bh"""
    lo, up, w, W, Lc = cs.lo, cs.up, cs.w, cs.W, cs.Lc
    A, Bh = _half(up)
    a = A_BASE
    lr, var, z = cs.ref
    fin = lambda x, m: bool(np.isfinite(x[m]).all())
    found = {}
    for k, (name, edit, x) in enumerate(cs.kinds):
        m = cs.of(name)
        nt = cs.nts[k]
        pos = cs.cp[m]
        nan_lr = pos[np.isnan(lr[m])]
        found[name] = dict(lr=len(nan_lr), var=int(np.isnan(var[m]).sum()), z=int(np.isnan(z[m]).sum()),
                           bg=int(np.isnan(nt["bg"]).sum()), smoothed=int(np.isnan(nt["smoothed"]).sum()))
        assert not np.isinf(lr[m]).any() and not np.isinf(z[m]).any(), name
        if name in ("control", "tiny-1", "tiny-2-out-upper", "tiny-2-out-below", "range"):
            assert fin(lr, m) and fin(var, m) and fin(z, m), name
            assert all(np.isfinite(nt[t]).all() for t in ("bg", "norm", "smoothed")), name
        elif name.startswith("tiny-2-in"):
            assert np.array_equal(nan_lr, np.arange(x - w, x + w + 1)), name     # W positions centred on the cell, all of them candidates
            assert fin(var, m) and fin(z, m), name
            assert all(np.isfinite(nt[t]).all() for t in ("bg", "norm", "smoothed")), name
        elif name == "zero":
            assert np.array_equal(nan_lr, np.arange(a - w - Bh, a + w + A + 1)), name
            assert fin(var, m) and fin(z, m), name
            assert all(np.isfinite(nt[t]).all() for t in ("bg", "norm", "smoothed")), name
        elif name == "nan":
            span = np.arange(a - w - Bh, a + w + A + 1)
            for s in (lr, var, z):
                assert np.array_equal(pos[np.isnan(s[m])], span), name
            for t in ("bg", "norm"):
                assert np.array_equal(np.flatnonzero(np.isnan(nt[t])), span), name
            # smoothed is NaN only where all 6 sd + 1 bases under the Gaussian are: 6 sd bases fewer
            assert np.array_equal(np.flatnonzero(np.isnan(nt["smoothed"])), span[3 * SMOOTH_SD:len(span) - 3 * SMOOTH_SD]), name
        elif name == "nan-ends":
            want = np.concatenate((np.arange(NAN_HEAD), np.arange(Lc - NAN_TAIL, Lc)))
            assert np.array_equal(np.flatnonzero(np.isnan(nt["norm"])), want)
            want = np.concatenate((np.arange(NAN_HEAD - 3 * SMOOTH_SD), np.arange(Lc - NAN_TAIL + 3 * SMOOTH_SD, Lc)))
            assert np.array_equal(np.flatnonzero(np.isnan(nt["smoothed"])), want)
            for s in (lr, var, z):
                assert np.array_equal(np.isnan(s[m]), (pos < NAN_HEAD) | (pos >= Lc - NAN_TAIL))
            assert np.isnan(lr[m]).sum() >= 15
    # the arm under test is taken by construction: 2^-500 separates the tiny-* windows from the control's
    for name in cs.names:
        if name.startswith("tiny"):
            s = cs.in_span(name)
            assert s.sum() >= W and (cs.emin[s] < ESMALL).all() and (cs.emin[s] > 0).all(), name
    assert (cs.emin[cs.of("control")] > ESMALL).all() and (cs.emin[cs.of("range")] > ESMALL).all()
    assert (cs.emin[cs.in_span("zero")] == 0).all() and cs.enan[cs.in_span("nan")].all()
    # the planted fragments are inside the NaN windows' fragment lists: more than 64 fragments per window (the paired kernel's tail loop)
    cen = cs.l + (cs.n - 1) // 2
    inwin = [int(((cen >= p - w) & (cen <= p + w)).sum()) for p in cs.cp[cs.of("control")]]
    assert min(inwin) > 64
    return found


@pytest.mark.parametrize("lo,up,w", GEOMETRIES)
def test_oracle_gives_the_table(lo, up, w):
    found = check_oracle_table(case(lo, up, w))
    if (lo, up, w) == (105, 251, 60):      # the figures of the issue, for a = 400
        for name in ("control", "tiny-1", "tiny-2-out-upper", "tiny-2-out-below", "range"):
            assert found[name] == dict(lr=0, var=0, z=0, bg=0, smoothed=0), name
        for name in ("tiny-2-in-lower", "tiny-2-in-mid", "tiny-2-in-last"):
            assert found[name] == dict(lr=121, var=0, z=0, bg=0, smoothed=0), name
        assert found["zero"] == dict(lr=370, var=0, z=0, bg=0, smoothed=0)
        assert found["nan"] == dict(lr=370, var=370, z=370, bg=370, smoothed=310)


# ---- the device ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def device(lo, up, w):
    """everything the device computes for one geometry, once: tracks, candidates through the default arm and the validation switches,
    the peak search with its statistics, and the window-probability route"""
    from nucleoatac_amd.device import Context
    cs = case(lo, up, w)
    out = {}
    with Context(0) as c:
        c.set_vmat(cs.vm, lo, up)
        c.set_sizes(cs.sizes)
        out["tiling"] = c.bg_tiling(cs.Lc)
        b = c.upload(cs.pk)
        b.run_nuc(SMOOTH_SD)
        out["tracks"] = {t: b.split(b.track(t)) for t in TRACKS}
        out["default"] = b.run_candidates(cs.cc, cs.cp)
        for switch in SWITCHES.get((lo, up, w), ()):                 # read at every launch
            os.environ[switch] = "1"
            try:
                out[switch] = b.run_candidates(cs.cc, cs.cp)
            finally:
                os.environ.pop(switch, None)
        pc, pp, lr, var, z = b.run_peaks(**PEAKS)
        out["peaks"] = (pc, pp, (lr, var, z), b.run_candidates(pc, pp))
        s = cs.cov_sample()
        out["cov"] = {mode: b.run_candidates_cov(cs.cc[s], cs.cp[s], mode) for mode in ("closed", "literal")}
        b.free()
    return out


@gpu
@pytest.mark.parametrize("lo,up,w", GEOMETRIES)
def test_candidates_of_every_kind_match_the_oracle(lo, up, w):
    """lr / var / z of the default arm (and of the validation switches' arms) at every candidate of every kind: NaN and infinity patterns
    exactly, finite values in the tight tier with the scales _reference_stats derives from the oracle's operands (Case.reference: and the
    floor of z on the range chunk following the floor of var)"""
    cs, dev = case(lo, up, w), device(lo, up, w)
    check_oracle_table(cs)
    nt, ex = dev["tiling"]
    assert 2 <= nt <= 3 and ex >= 1                                  # FFT background, extended tiles
    tvx = 512 - cs.W + 1 + 32
    assert ex == nt and all(abs(A_BASE - t * tvx) >= 16 for t in range(nt + 1))      # `a` is on no tile border
    arms = ["default"] + list(SWITCHES.get((lo, up, w), ()))
    for arm in arms:
        for name in cs.names:                                        # per kind: a failure names the kind
            m = cs.of(name)
            _assert_stats([g[m] for g in dev[arm]], [r[m] for r in cs.ref], [s[m] for s in cs.scales], "%s %s" % (arm, name))
        _assert_stats(dev[arm], cs.ref, cs.scales, arm)


@gpu
@pytest.mark.parametrize("lo,up,w", GEOMETRIES)
def test_peak_search_launch_site(lo, up, w):
    """natac_run_peaks launches the candidate kernel itself: its list is call_peaks of the device's own norm + smoothed (NaNs filled with
    the chunk's minimum), its statistics are natac_run_candidates' at the same positions bit for bit, and they match the oracle"""
    from oracle import natac_oracle as O
    cs, dev = case(lo, up, w), device(lo, up, w)
    pc, pp, stats, again = dev["peaks"]
    tr = dev["tracks"]
    for k, name in enumerate(cs.names):
        hp = np.asarray(O.call_peaks((tr[L.T_NORM][k] + tr[L.T_SMOOTH][k]).copy(), **PEAKS), np.int64)
        assert np.array_equal(pp[pc == k], hp), "peaks of the %s chunk" % name
    assert len(pc) >= 5 * len(cs.names)
    for g, a in zip(stats, again):
        assert np.array_equal(g, a, equal_nan=True)
    with np.errstate(all="ignore"):
        ref, scales = cs.reference(pc, pp)
    _assert_stats(stats, ref, scales, "run_peaks")
    A, Bh = _half(up)
    k = cs.names.index("zero")
    inz = (pc == k) & (pp >= A_BASE - w - Bh) & (pp <= A_BASE + w + A)
    assert inz.sum() >= 2 and np.isnan(stats[0][inz]).all() and np.isfinite(stats[1][inz]).all()     # peaks inside the zero chunk's span


@gpu
@pytest.mark.parametrize("lo,up,w", GEOMETRIES)
def test_tracks_of_every_kind_match_the_oracle(lo, up, w):
    cs, dev = case(lo, up, w), device(lo, up, w)
    tr = dev["tracks"]
    for k, name in enumerate(cs.names):
        nt = cs.nts[k]
        sc = cancel_scale(nt["raw"], nt["bg"])
        assert_track(tr[L.T_BACKGROUND][k], nt["bg"], "bg " + name)          # assert_track: NaN patterns equal exactly, then the tight tier
        assert_track(tr[L.T_NORM][k], nt["norm"], "norm " + name, scale=sc)
        assert_track(tr[L.T_SMOOTH][k], nt["smoothed"], "smoothed " + name, scale=sc)
    k = cs.names.index("nan")
    n_bg, n_sm = int(np.isnan(tr[L.T_BACKGROUND][k]).sum()), int(np.isnan(tr[L.T_SMOOTH][k]).sum())
    assert 0 < n_sm == n_bg - 6 * SMOOTH_SD
    k = cs.names.index("nan-ends")
    norm, sm = tr[L.T_NORM][k], tr[L.T_SMOOTH][k]
    assert np.isnan(norm[:NAN_HEAD]).all() and np.isnan(norm[-NAN_TAIL:]).all() and np.isfinite(norm[NAN_HEAD:-NAN_TAIL]).all()
    # the renormalised `same` smoothing at both ends, NaNs under the window: finite as soon as one base under the Gaussian is
    assert np.isnan(sm[0]) and np.isnan(sm[-1]) and np.isfinite(sm[NAN_HEAD - 3 * SMOOTH_SD:cs.Lc - NAN_TAIL + 3 * SMOOTH_SD]).all()


@gpu
@pytest.mark.parametrize("lo,up,w", GEOMETRIES)
def test_window_probability_route(lo, up, w):
    """run_candidates_cov (natac_cand_window_probs, then the closed form and the .pyx's literal pair sum in fp64) at 8 candidates per
    kind, against calculate_cov_closed of the oracle's window probabilities"""
    from oracle import natac_oracle as O
    cs, dev = case(lo, up, w), device(lo, up, w)
    s = cs.cov_sample()
    assert len(s) == 8 * len(cs.names)
    ref = np.empty(len(s))
    with np.errstate(all="ignore"):
        for j, (k, p) in enumerate(zip(cs.cc[s], cs.cp[s])):
            nt = cs.nts[k]
            pr = O.signal_distribution_probs(nt["bmat"], nt["b_start"], lo, up, w, int(p))
            ref[j] = O.calculate_cov_closed(pr, np.ravel(cs.vm), nt["nuc_cov"][p])
    assert np.array_equal(ref, cs.ref[1][s], equal_nan=True)             # the same numbers z_score returned
    assert np.isnan(ref[cs.cc[s] == cs.names.index("nan")]).all() and np.isfinite(ref[cs.cc[s] == cs.names.index("zero")]).all()
    assert (ref[np.isfinite(ref)] > 0).sum() >= 8 * (len(cs.names) - 2)
    for mode in ("closed", "literal"):
        _assert_stat(dev["cov"][mode], ref, "run_candidates_cov %s" % mode, 1.0)
