"""GPU: the multinomial-variance sweep (natac_run_candidates_cov: natac_cand_window_probs, natac_cov_literal_many,
natac_cov_closed_many<double> / <float>, natac_gather_f64) off the default V-plot, against the oracle's chain nuc_chunk_tracks -> bmat ->
signal_distribution_probs -> calculate_cov_literal / calculate_cov_closed (tests/scale_workers.py::cov_literal_worker).

Geometries: the four V-plots of test_generic_vmat_geometry (even / odd lower bound, odd row count, a size-1 row whose cell is ONE exp(bias)
factor) and a tiny one, rows 1..5 x 11 columns (lower 1, upper 6, w 5): 55 cells -- fewer than a workgroup has lanes, R odd, R * W no
multiple of 256 -- with a size distribution that gives the size-1 row real weight.  Each with and without a bias track, on 8 ragged
chunks of 300..900 bases (one without fragments), hand-made candidates (positions 0, 1, L - 1, interior ones, repeats) and, for the tiny
V-plot, every position of five chunks: 2,691 candidates, two passes of the 2,048-candidate slab loop, the second one short.

Tolerances are the config-5 test's, relative to the variance r (S1 - S2^2), S1 = sum p v^2, S2 = sum p v: they hold while the
cancellation is mild, so every asserted candidate also asserts the condition number (S1 + S2^2) / (S1 - S2^2) <= 10 (largest met: 9.9)."""
import functools

import numpy as np
import pytest

from helpers import golden
from nucleoatac_amd import _lib as L
from nucleoatac_amd.packing import PackedChunks
from nucleoatac_amd.synth import synth_size_distribution

pytestmark = pytest.mark.gpu

TINY = (1, 6, 5)
GEOMS = [(110, 240, 50), (111, 240, 50), (107, 250, 60), (1, 60, 20), TINY]
LENS = [300, 517, 900, 641, 333, 768, 455, 899]
EMPTY = 6                         # the chunk without fragments
PEAK_KW = dict(min_signal=0, sep=21, boundary=40, order=10)
COND_MAX = 10.0
RTOL_LITERAL, RTOL_CLOSED = 1e-10, 1e-9


def _model(vlo, vup, w):
    """V-plot and sizes: built as test_generic_vmat_geometry builds them; the tiny one with a wide spread of template values and a
    size distribution that is positive at size 1"""
    if (vlo, vup, w) == TINY:
        rng = np.random.default_rng(11)
        vm = rng.random((vup - vlo, 2 * w + 1)) ** 2 * 0.01 + 1e-4
        sizes = rng.random(vup) * 0.5 + 0.1
        return vm, sizes / sizes.sum()
    if vlo >= 105:
        vm = np.ascontiguousarray(golden("params_example")["vmat"][vlo - 105:vup - 105, 60 - w:60 + w + 1])
    else:
        vm = np.random.default_rng(3).random((vup - vlo, 2 * w + 1)) * 0.01 + 1e-4
    return vm, synth_size_distribution(251)[:vup]


def _fragments(rng, lens, vlo, vup, empty=EMPTY):
    """at most 300 fragments per chunk, half of them with a size inside the V-plot, centres from 150 bases before to 150 after"""
    fr = []
    for k, Lc in enumerate(lens):
        nf = 0 if k == empty else int(rng.integers(150, 301))
        n = np.where(rng.random(nf) < 0.5, rng.integers(vlo, vup, size=nf), rng.integers(1, 330, size=nf))
        c = np.sort(rng.integers(-150, Lc + 150, size=nf))
        fr.append(((c - (n - 1) // 2).astype(np.int64), n.astype(np.int64)))
    return fr


def _pack(lens, fr, bias, bias_left, bias_right):
    off = np.concatenate(([0], np.cumsum([len(x[0]) for x in fr])))
    nb = [Lc + bias_left + bias_right for Lc in lens]
    return PackedChunks(np.arange(len(lens)) * 20000, lens, off, np.concatenate([x[0] for x in fr]), np.concatenate([x[1] for x in fr]),
                        None if bias is None else np.concatenate(([0], np.cumsum(nb))), bias, bias_left=bias_left, bias_right=bias_right)


def _stats(pr, v, r):
    """(oracle literal, oracle closed, S1, S2, condition number) of one candidate"""
    from oracle import natac_oracle as O
    S1, S2 = float(np.sum(pr * v * v)), float(np.sum(pr * v))
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = (S1 + S2 * S2) / (S1 - S2 * S2)
    return O.calculate_cov_literal(pr, v, r), O.calculate_cov_closed(pr, v, r), S1, S2, cond


@functools.lru_cache(maxsize=None)
def _case(vlo, vup, w, with_bias):
    """the batch of one geometry, its hand-made candidates and the oracle's values at them: computed once, shared, never changed"""
    from oracle import natac_oracle as O
    vm, sizes = _model(vlo, vup, w)
    rng = np.random.default_rng([vlo, vup, w])            # one set of fragments per geometry, with and without bias
    fr = _fragments(rng, LENS, vlo, vup)
    bias = rng.normal(0, 0.7, size=sum(Lc + 246 + 247 for Lc in LENS)) if with_bias else None
    pk = _pack(LENS, fr, bias, 246, 247)
    nts = [O.nuc_chunk_tracks(l, n, 0, Lc, pk.chunk_bias(k), -246, vm, vlo, vup, sizes, smooth_sd=7)
           for k, ((l, n), Lc) in enumerate(zip(fr, LENS))]
    cc, cp = [], []
    if (vlo, vup, w) == TINY:                              # every position of five chunks: 2,691 > 2,048, two slab passes
        for k in range(5):
            cc += [k] * LENS[k]
            cp += list(range(LENS[k]))
    else:                                                  # 0, L - 1 and the oracle's first peak (or the middle) of every chunk, 1 of two
        for k, Lc in enumerate(LENS):
            hp = O.call_peaks((nts[k]["norm"] + nts[k]["smoothed"]).copy(), **PEAK_KW)
            pos = [0, Lc - 1, int(hp[0]) if len(hp) else Lc // 2] + ([1] if k in (0, 3) else [])
            cc += [k] * len(pos)
            cp += pos
    cc += cc[2:6]                                          # repeated entries
    cp += cp[2:6]
    assert (vlo, vup, w) == TINY or len(cc) <= 40          # the literal pair sum is O(N^2) per candidate, on both sides
    v = np.ravel(vm)
    r = np.array([nts[k]["nuc_cov"][p] for k, p in zip(cc, cp)])
    once = {}                                              # the oracle once per distinct candidate with reads; the others assert 0.0
    for k, p, rk in zip(cc, cp, r):
        if int(rk) > 0 and (k, p) not in once:
            once[(k, p)] = _stats(O.signal_distribution_probs(nts[k]["bmat"], nts[k]["b_start"], vlo, vup, w, p), v, rk)
    ref = np.array([once.get((k, p), (0.0, 0.0, 0.0, 0.0, 0.0)) for k, p in zip(cc, cp)]).reshape(-1, 5)
    for a in (ref, r):
        a.setflags(write=False)
    return dict(vm=vm, sizes=sizes, pk=pk, nts=nts, cc=np.array(cc, np.int32), cp=np.array(cp, np.int32), ref=ref, r=r)


def _rel_ok(got, want, rtol):
    return np.abs(got - want) <= rtol * np.abs(want)


def _assert_fp32(f32, clo, ref, r, N):
    """|fp32 - closed fp64| <= (N + 8) 2^-24 r (S1 + 2 S2^2): S1 and S2 are sums of N non-negative terms, so in any order each is off
    by at most (N - 1) units of 2^-24 relative, plus three input / product roundings per term and the final S2^2 and subtraction;
    and the fp32 result must not be the fp64 one (a dispatch mix-up between the two templates)"""
    bound = (N + 8) * 2.0 ** -24 * np.abs(r) * (ref[:, 2] + 2 * ref[:, 3] ** 2)
    err = np.abs(f32 - ref[:, 1])
    frac = float(np.max(err / bound))
    print("fp32: largest error / bound = %.3g" % frac)
    assert np.all(err <= bound), frac
    assert np.any(f32 != clo)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("vlo,vup,w", GEOMS)
def test_cov_sweep_geometry(vlo, vup, w, with_bias):
    from nucleoatac_amd.device import Context
    case = _case(vlo, vup, w, with_bias)
    cc, cp, ref, r = case["cc"], case["cp"], case["ref"], case["r"]
    with Context(0) as c:
        c.set_vmat(case["vm"], vlo, vup)
        c.set_sizes(case["sizes"])
        b = c.upload(case["pk"])
        b.run_nuc(7)
        pc, pp, _, pvar, _ = b.run_peaks(**PEAK_KW)
        lit = b.run_candidates_cov(cc, cp, "literal")
        clo = b.run_candidates_cov(cc, cp, "closed")
        f32 = b.run_candidates_cov(cc, cp, "fp32")
        b.free()
    reads = r.astype(np.int64) > 0
    assert reads.sum() >= 12 and (~reads).sum() >= 3           # the chunk without fragments alone gives 3 without reads
    assert reads[np.isin(cp, (0, 1))].any() and reads[cp == np.array(LENS)[cc] - 1].any()      # chunk edges among the asserted ones
    # coverage 0: exactly 0.0 in all three modes
    for got in (lit, clo, f32):
        assert np.array_equal(got[~reads], np.zeros((~reads).sum()))
    ref, r, lit, clo, f32, kc, kp = ref[reads], r[reads], lit[reads], clo[reads], f32[reads], cc[reads], cp[reads]
    cond = float(ref[:, 4].max())
    print("condition number: largest %.3g over %d candidates" % (cond, len(r)))
    assert cond <= COND_MAX
    assert np.all(_rel_ok(lit, ref[:, 0], RTOL_LITERAL)), float(np.max(np.abs(lit - ref[:, 0]) / ref[:, 0]))
    assert np.all(_rel_ok(clo, ref[:, 1], RTOL_CLOSED)), float(np.max(np.abs(clo - ref[:, 1]) / ref[:, 1]))
    # natac_run_peaks' own var is the closed form: compared where a candidate of the list is one of its peaks
    peak_var = {(int(k), int(p)): x for k, p, x in zip(pc, pp, pvar)}
    mine = np.array([peak_var.get((int(k), int(p)), np.nan) for k, p in zip(kc, kp)])
    hit = ~np.isnan(mine)
    assert hit.sum() >= 5
    assert np.all(_rel_ok(mine[hit], clo[hit], RTOL_CLOSED))
    _assert_fp32(f32, clo, ref, r, case["vm"].size)


@functools.lru_cache(maxsize=None)
def _short_margin_case():
    from oracle import natac_oracle as O
    vlo, vup, w = 110, 240, 50
    BL, BR = 40, 25
    assert BL < w + (vup - 2) // 2 and BR < w + (vup - 1) // 2
    vm, sizes = _model(vlo, vup, w)
    lens = [300, 30, 420]
    rng = np.random.default_rng(5)
    fr = _fragments(rng, lens, vlo, vup, empty=-1)
    bias = rng.normal(0, 0.7, size=sum(Lc + BL + BR for Lc in lens))
    pk = _pack(lens, fr, bias, BL, BR)
    # edge candidates: up to 84 % of the window's cells are 0.  The very last positions (0, L - 1: 90 % and more) leave so few cells that the
    # condition number passes 10 (12 .. 26); the candidates below stay at 9.9 or less on both sides of both long chunks
    cc = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2], np.int32)
    cp = np.array([20, 25, 35, 60, 150, 240, 265, 275, 0, 15, 29, 35, 210, 385, 395], np.int32)
    cov = 5.0
    v = np.ravel(vm)
    nts = []
    for k, Lc in enumerate(lens):
        padded = np.concatenate((np.full(246 - BL, -np.inf), pk.chunk_bias(k), np.full(247 - BR, -np.inf)))
        nts.append(O.nuc_chunk_tracks(fr[k][0], fr[k][1], 0, Lc, padded, -246, vm, vlo, vup, sizes, smooth_sd=7))
    ref = []
    for k, p in zip(cc, cp):
        with np.errstate(invalid="ignore", divide="ignore"):
            pr = O.signal_distribution_probs(nts[k]["bmat"], nts[k]["b_start"], vlo, vup, w, int(p))
        ref.append(_stats(pr, v, cov) + (float(np.mean(pr == 0)),))
    ref = np.array(ref)
    ref.setflags(write=False)
    return vm, sizes, pk, cc, cp, cov, ref


def test_cov_sweep_bias_margins_shorter_than_the_window():
    """the `j < 0 || j >= nb` arm of the exp(bias) window: the entry point needs only NUC_COV, so a batch that never ran natac_run_nuc
    may carry bias margins (40 left, 25 right) far shorter than w + (vup - 2) // 2 = w + (vup - 1) // 2 = 169.  exp(bias) counts as 0
    outside the track -- the oracle on the same track padded with -inf.  Chunk 1 (30 bases, 95 bias entries) is shorter than the 109
    bases between the two insertion points of the smallest size: every cell of every window is 0, sB = 0, NaN on both sides."""
    from nucleoatac_amd.device import Context
    vlo, vup, w = 110, 240, 50
    vm, sizes, pk, cc, cp, cov, ref = _short_margin_case()
    with Context(0) as c:
        c.set_vmat(vm, vlo, vup)
        c.set_sizes(sizes)
        b = c.upload(pk)
        b.set_track(L.T_NUC_COV, np.full(pk.total_bp, cov))        # natac_run_nuc never runs
        lit = b.run_candidates_cov(cc, cp, "literal")
        clo = b.run_candidates_cov(cc, cp, "closed")
        f32 = b.run_candidates_cov(cc, cp, "fp32")
        b.free()
    dead = cc == 1
    assert np.isnan(ref[dead, :2]).all() and not np.isnan(ref[~dead, :2]).any()
    assert (ref[~dead, 5] > 0.2).sum() >= 6 and (ref[~dead, 5] == 0).any()    # windows that are partly outside, and one that is not
    for got in (lit, clo, f32):
        assert np.array_equal(np.isnan(got), dead)
    ref, lit, clo, f32 = ref[~dead], lit[~dead], clo[~dead], f32[~dead]
    print("condition number: largest %.3g" % ref[:, 4].max())
    assert ref[:, 4].max() <= COND_MAX
    assert np.all(_rel_ok(lit, ref[:, 0], RTOL_LITERAL))
    assert np.all(_rel_ok(clo, ref[:, 1], RTOL_CLOSED))
    _assert_fp32(f32, clo, ref, np.full(len(ref), cov), vm.size)


def test_cov_sweep_read_count_of_any_coverage_value():
    """r = int(nuc_cov[pos]) on the host for what natac_batch_set_track can put there: fractions truncate towards zero (0.99 -> 0,
    7.9 -> 7, -0.5 -> 0 and var = 0.0, -1.5 -> -1), 1e6 stays, NaN gives NaN and 3e9 saturates at INT_MAX (natac.h) -- in the sweep and
    in the var of natac_run_candidates, which converts the same value on the device"""
    from nucleoatac_amd.device import Context
    from oracle import natac_oracle as O
    vlo, vup, w = TINY
    case = _case(vlo, vup, w, True)
    vals = np.array([0.99, 1.0, 7.9, -0.5, -1.5, 1e6, np.nan, 3e9])
    want_r = np.array([0, 1, 7, 0, -1, 10 ** 6, 0, 2 ** 31 - 1], np.float64)
    k, p0 = 2, 400
    cc, cp = np.full(len(vals), k, np.int32), (p0 + 3 * np.arange(len(vals))).astype(np.int32)
    nt = case["nts"][k]
    v = np.ravel(case["vm"])
    unit = np.array([_stats(O.signal_distribution_probs(nt["bmat"], nt["b_start"], vlo, vup, w, int(p)), v, 1) for p in cp])
    assert unit[:, 4].max() <= COND_MAX
    with Context(0) as c:
        c.set_vmat(case["vm"], vlo, vup)
        c.set_sizes(case["sizes"])
        b = c.upload(case["pk"])
        b.run_nuc(7)
        track = b.track(L.T_NUC_COV)
        track[case["pk"].out_off[k] + cp] = vals
        b.set_track(L.T_NUC_COV, track)
        got = {m: b.run_candidates_cov(cc, cp, m) for m in ("literal", "closed", "fp32")}
        _, var, _ = b.run_candidates(cc, cp)
        b.free()
    nan = np.isnan(vals)
    zero = want_r == 0
    zero[nan] = False
    for name, res, col, rtol in (("literal", got["literal"], 0, RTOL_LITERAL), ("closed", got["closed"], 1, RTOL_CLOSED),
                                 ("run_candidates", var, 1, RTOL_CLOSED)):
        assert np.isnan(res[nan]).all() and not np.isnan(res[~nan]).any(), name
        assert np.array_equal(res[zero], np.zeros(zero.sum())), name
        m = ~nan & ~zero
        want = want_r[m] * unit[m, col]                  # the oracle's value for int(r): r times its value for r = 1
        assert np.all(_rel_ok(res[m], want, rtol)), (name, res[m], want)
    assert np.isnan(got["fp32"][nan]).all() and np.array_equal(got["fp32"][zero], np.zeros(zero.sum()))
    m = ~nan & ~zero
    ref = unit[m].copy()
    ref[:, 1] *= want_r[m]
    _assert_fp32(got["fp32"][m], got["closed"][m], ref, want_r[m], v.size)


def test_cov_sweep_argument_errors():
    from nucleoatac_amd.device import Context
    vlo, vup, w = TINY
    case = _case(vlo, vup, w, True)
    with Context(0) as c:
        c.set_vmat(case["vm"], vlo, vup)
        c.set_sizes(case["sizes"])
        b = c.upload(case["pk"])
        b.set_track(L.T_NUC_COV, np.ones(case["pk"].total_bp))
        for k, p in ((len(LENS), 0), (-1, 0), (0, LENS[0]), (0, -1), (4, LENS[4])):
            for mode in ("closed", "literal", "fp32"):
                with pytest.raises(L.NatacError):
                    b.run_candidates_cov([0, k], [5, p], mode)
        with pytest.raises(ValueError):
            b.run_candidates_cov([0, 1], [5], "closed")
        for mode in ("closed", "literal", "fp32"):
            out = b.run_candidates_cov(np.zeros(0, np.int32), np.zeros(0, np.int32), mode)
            assert out.shape == (0,) and out.dtype == np.float64
        assert b.run_candidates_cov([0], [LENS[0] - 1], "closed").shape == (1,)     # the batch is still usable
        b.free()
