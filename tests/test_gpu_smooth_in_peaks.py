"""GPU: T_SMOOTH formed inside the peak search (natac_peaks_chunk_reg<NJ, 256, true>) == T_SMOOTH formed by natac_run_nuc's own
smoothing kernel, bit for bit, with everything downstream of it (candidate lists, lr / var / z).

natac_run_nuc leaves T_SMOOTH pending when its window is 61 bases (smooth_sd 10) and no chunk is longer than 4,096 bases; natac_run_peaks
then forms it from the chunk it holds -- unless another reader asked for the track first, or the search takes an arm the fused kernel
does not cover (masks in registers), in which case natac_smooth_same4 runs as before.  NATAC_SMOOTH_FUSED=0, read when a context is
created, keeps the two-kernel path: every scenario below runs on one context of each kind and the results are compared with
np.array_equal (NaN positions included).  The profile's smooth_nuc launch count tells which path a scenario took.

NaNs reach the fused kernel the way they do in a run: through the bias track (a NaN there makes the background, and so NORM, NaN on
370 bases around it).  natac_batch_set_track(T_NORM) is a READER of a pending T_SMOOTH (the track keeps the values of the NORM it was
run with), so NaNs planted that way test that rule and the search on a NaN-riddled NORM next to a clean SMOOTH."""
import os

import numpy as np
import pytest

from helpers import assert_track, golden, packed_from_golden
from nucleoatac_amd import _lib as L
from nucleoatac_amd.packing import PackedChunks

gpu = pytest.mark.gpu       # every test but the CPU check of the plan

# 61 = the window, the shortest chunk natac_run_nuc takes; the edges of NJ = 1, 4, 16; 2120 (NJ = 9, the flagship's)
LENS = [61, 62, 255, 256, 257, 1023, 1024, 1025, 2120, 4095, 4096]
DENSITY = [0.5, 0.0, 0.4, 0.4, 0.4, 0.4, 0.4, 0.4, 0.4, 0.4, 0.4]     # chunk 1: no fragments, NORM is exactly 0 on all of it
BL, BR = 246, 247                       # the default bias halo
BENCH = dict(min_signal=0, sep=25, boundary=60, order=12)
ARMS = [("bench", BENCH), ("order2", dict(min_signal=0, sep=25, boundary=60, order=2)),      # no two-phase list
        ("order150", dict(min_signal=0, sep=25, boundary=60, order=150))]                   # masks in registers at 4,096 bases: unfused
# NaNs of the bias track, (chunk, base): NORM is NaN on about [base - 185, base + 184]
BIAS_NAN = [(8, 1000),              # a run of 370 in the middle of 2,120 bases
            (5, 100), (5, 930),     # runs touching base 0 and base L - 1 of 1,023 bases
            (2, 127),               # all 255 bases
            (9, 210), (9, 3890)]    # runs that stop about 25 / 20 bases short of the ends of 4,095 bases: NaN within 30 bases of both


def _batch(lens, density, seed, bias_nan=()):
    rng = np.random.default_rng(seed)
    fr = []
    for Lc, d in zip(lens, density):
        nf = int(d * (Lc + 300))
        n = rng.integers(30, 330, size=nf)
        c = np.sort(rng.integers(-150, Lc + 150, size=nf))
        fr.append(((c - (n - 1) // 2).astype(np.int64), n.astype(np.int64)))
    off = np.concatenate(([0], np.cumsum([len(x[0]) for x in fr])))
    nb = [Lc + BL + BR for Lc in lens]
    boff = np.concatenate(([0], np.cumsum(nb)))
    bias = rng.normal(0, 0.7, size=sum(nb))
    for k, p in bias_nan:
        bias[boff[k] + BL + p] = np.nan
    return PackedChunks(np.arange(len(lens)) * 20000, lens, off, np.concatenate([x[0] for x in fr]), np.concatenate([x[1] for x in fr]),
                        boff, bias)


def _context(fused):
    from nucleoatac_amd.device import Context
    old = os.environ.pop("NATAC_SMOOTH_FUSED", None)
    if not fused:
        os.environ["NATAC_SMOOTH_FUSED"] = "0"
    try:
        c = Context(0)                  # natac_ctx_create reads the switch
    finally:
        os.environ.pop("NATAC_SMOOTH_FUSED", None)
        if old is not None:
            os.environ["NATAC_SMOOTH_FUSED"] = old
    par = golden("params_example")
    c.set_vmat(par["vmat"], int(par["vlower"]), int(par["vupper"]))
    c.set_sizes(par["sizes"])
    c.profile_enable(True)
    return c


def _smooth_launches(ctx, fn):
    """what fn() returns and the number of smoothing-kernel launches (natac_smooth_same4 / natac_smooth_same) it made"""
    ctx.profile_reset()
    out = fn()
    return out, ctx.profile()["smooth_nuc"][1]


def _planted_norm(norm, lens):
    """NORM of the ragged batch with NaNs, negative values and exact zeros planted, every kind in a chunk of its own"""
    x = norm.copy()
    o = np.concatenate(([0], np.cumsum(lens)))
    x[o[8] + 700] = np.nan                                  # a single base
    x[o[8] + 1200:o[8] + 1300] = np.nan                     # a run longer than the window
    x[o[6]:o[6] + 40] = np.nan                              # a run touching base 0
    x[o[7] - 75:o[7]] = np.nan                              # a run touching base L - 1 (of chunk 6)
    x[o[3]:o[4]] = np.nan                                   # a chunk that is all NaN
    x[o[10] + 12:o[10] + 20] = np.nan                       # NaN within 30 bases of both ends
    x[o[11] - 29:o[11] - 3] = np.nan
    x[o[9] + 100:o[9] + 200] = -np.abs(x[o[9] + 100:o[9] + 200]) - 0.25      # negative values
    x[o[9] + 300:o[9] + 400] = 0.0                          # exact zeros, both signs
    x[o[9] + 350:o[9] + 360] = -0.0
    return x


def _scenarios(ctx):
    """every scenario on one context: {name: array} and {name: smoothing launches}"""
    res, launches = {}, {}

    def keep(name, arrays):
        for i, a in enumerate(arrays):
            res["%s/%d" % (name, i)] = np.asarray(a)

    pk = _batch(LENS, DENSITY, seed=1, bias_nan=BIAS_NAN)
    b = ctx.upload(pk)
    # ---- every arm of the search on a fresh pass: release_outputs, natac_run_nuc, natac_run_peaks, then the tracks
    for name, kw in ARMS:
        def one_pass():
            b.release_outputs()
            b.run_nuc(10)
            pks = b.run_peaks(**kw)
            return list(pks) + [b.track(L.T_SMOOTH), b.track(L.T_NORM), b.status()]
        out, launches[name] = _smooth_launches(ctx, one_pass)
        keep(name, out)
    # ---- the track read before the search == the track the search leaves; a second search gives the same
    def read_first():
        b.release_outputs()
        b.run_nuc(10)
        before = b.track(L.T_SMOOTH)
        first = b.run_peaks(**BENCH)
        return [before] + list(first)
    out, launches["read_first"] = _smooth_launches(ctx, read_first)
    keep("read_first", out)

    def twice():
        b.release_outputs()
        b.run_nuc(10)
        first = b.run_peaks(**BENCH)
        mid = b.track(L.T_SMOOTH)
        second = b.run_peaks(**BENCH)
        return list(first) + [mid] + list(second) + [b.track(L.T_SMOOTH)]
    out, launches["twice"] = _smooth_launches(ctx, twice)
    keep("twice", out)
    # ---- NORM replaced while SMOOTH is pending: SMOOTH keeps the values of the run's NORM, the search reads the new NORM next to it
    def planted():
        b.release_outputs()
        b.run_nuc(10)
        b.set_track(L.T_NORM, _planted_norm(b.track(L.T_NORM), LENS))
        pks = b.run_peaks(**BENCH)
        return list(pks) + [b.track(L.T_SMOOTH), b.track(L.T_NORM)]
    out, launches["planted"] = _smooth_launches(ctx, planted)
    keep("planted", out)
    # ---- another batch of the context changes the model generation and the context's window while this one's SMOOTH is pending
    par = golden("params_example")
    other = ctx.upload(_batch([500, 300], [0.4, 0.4], seed=2))

    def window_kept(reader):
        def run():
            b.release_outputs()
            b.run_nuc(10)
            ctx.set_vmat(par["vmat"], int(par["vlower"]), int(par["vupper"]))
            ctx.set_sizes(par["sizes"])
            other.run_nuc(4)                        # a 25-base window in the context's slot
            if reader == "search":
                pks = b.run_peaks(**BENCH)
                return list(pks) + [b.track(L.T_SMOOTH)]
            return [b.track(L.T_SMOOTH), other.track(L.T_SMOOTH)]
        return run
    for reader in ("search", "download"):
        out, launches["window_" + reader] = _smooth_launches(ctx, window_kept(reader))
        keep("window_" + reader, out)
    other.free()
    b.free()
    # ---- one chunk of 4,097 bases: the 1,024-thread variant, not fused
    b = ctx.upload(_batch([4097], [0.4], seed=3, bias_nan=[(0, 2000)]))

    def long_chunk():
        b.run_nuc(10)
        pks = b.run_peaks(**BENCH)
        return list(pks) + [b.track(L.T_SMOOTH)]
    out, launches["4097"] = _smooth_launches(ctx, long_chunk)
    keep("4097", out)
    b.free()
    return res, launches


def test_plan_forms_smooth_where_the_model_says():
    """CPU: the library's plan (natac_peaks_plan, natac_peaks.hpp) forms SMOOTH in the search exactly where the model of
    test_gpu_peak_arms says the 256-thread kernel runs with its masks in LDS -- for every length of LENS (and 4,097) as a batch's
    longest chunk under every search of ARMS; natac_run_nuc leaves the track pending (order 1 can fuse) exactly up to 4,096 bases"""
    from nucleoatac_amd.device import peaks_plan
    from test_gpu_peak_arms import peak_arm
    for maxL in LENS + [4097]:
        for name, kw in ARMS:
            want = maxL <= 4096 and peak_arm(maxL, kw["order"]).mask != "registers"
            assert peaks_plan(maxL, kw["order"])["forms_smooth"] == want, (maxL, name)
    assert [peaks_plan(4096, kw["order"])["forms_smooth"] for _, kw in ARMS] == [True, True, False]      # bench, order2, order150
    assert all(peaks_plan(maxL, 1)["forms_smooth"] == (maxL <= 4096) for maxL in range(1, 5000))


@pytest.fixture(scope="module")
def both():
    out = {}
    for fused in (True, False):
        c = _context(fused)
        try:
            out[fused] = _scenarios(c)
        finally:
            c.close()
    return out


@gpu
def test_fused_equals_two_kernels(both):
    """every array of every scenario: chunk lengths 61 .. 4,096 in one ragged batch and 4,097 alone, NaN runs from the bias track, the
    bench's search parameters, order 2 and order 150, reads before and after the search, planted NORM, a foreign window"""
    (fu, _), (sp, _) = both[True], both[False]
    assert fu.keys() == sp.keys() and len(fu) > 60
    for name in fu:
        assert fu[name].dtype == sp[name].dtype and np.array_equal(fu[name], sp[name], equal_nan=fu[name].dtype.kind == "f"), name


@gpu
def test_which_path_ran(both):
    """smoothing-kernel launches per scenario: the fused context runs none where the search forms the track, one where another
    reader comes first or the search's arm is not covered (the other batch of window_* adds its own)"""
    assert both[False][1] == {"bench": 1, "order2": 1, "order150": 1, "read_first": 1, "twice": 1, "planted": 1, "window_search": 2,
                              "window_download": 2, "4097": 1}
    assert both[True][1] == {"bench": 0, "order2": 0, "order150": 1, "read_first": 1, "twice": 0, "planted": 1, "window_search": 1,
                             "window_download": 2, "4097": 1}


@gpu
def test_scenarios_hold_what_they_claim(both):
    """the NaN runs, zeros and candidates the comparison above relies on are there, and the state rules hold on the fused context"""
    fu = both[True][0]
    o = np.concatenate(([0], np.cumsum(LENS)))
    cc, cp, lr, var, z, sm, norm = [fu["bench/%d" % i] for i in range(7)]
    nan = np.isnan(norm)
    assert nan[o[2]:o[3]].all() and np.isnan(sm[o[2]:o[3]]).all()                        # the all-NaN chunk
    assert nan[o[5]] and nan[o[6] - 1] and not nan[o[5] + 400:o[5] + 700].any()          # runs touching both ends
    n9 = nan[o[9]:o[10]]
    assert not n9[0] and n9[:30].any() and not n9[-1] and n9[-30:].any()                 # NaN within 30 bases of both ends, not at them
    run8 = np.flatnonzero(nan[o[8]:o[9]])
    assert len(run8) > 61 and run8[0] > 61 and run8[-1] < LENS[8] - 62                   # longer than the window, inside the chunk
    assert np.isnan(sm[o[8]:o[9]]).sum() == len(run8) - 60                               # NaN only where the whole window is
    assert (norm[o[1]:o[2]] == 0).all() and (sm[o[1]:o[2]] == 0).all()                   # exact zeros
    assert (norm[~nan] < 0).sum() > 1000 and (sm[~np.isnan(sm)] >= 0).all()              # negative values are clamped
    assert len(cc) > 100 and np.isfinite(lr).any()
    assert not fu["bench/7"].any()
    # read before the search == after it; searched twice: the same lists and the same track
    assert np.array_equal(fu["read_first/0"], sm, equal_nan=True)
    for i in range(5):
        assert np.array_equal(fu["read_first/%d" % (i + 1)], fu["bench/%d" % i], equal_nan=True)
        assert np.array_equal(fu["twice/%d" % i], fu["twice/%d" % (i + 6)], equal_nan=True)
    assert np.array_equal(fu["twice/5"], fu["twice/11"], equal_nan=True) and np.array_equal(fu["twice/5"], sm, equal_nan=True)
    # a planted NORM leaves SMOOTH what the run's NORM made it
    assert np.array_equal(fu["planted/5"], sm, equal_nan=True) and np.isnan(fu["planted/6"][o[3]:o[4]]).all()
    # formed under another batch's window and model generation: still this batch's window
    assert np.array_equal(fu["window_search/5"], sm, equal_nan=True) and np.array_equal(fu["window_download/0"], sm, equal_nan=True)
    for i in range(2):      # the lists; the statistics take another arm after a model change (no background factors of that generation)
        assert np.array_equal(fu["window_search/%d" % i], fu["bench/%d" % i])
    assert len(fu["4097/0"]) > 10 and np.isnan(fu["4097/5"]).sum() > 250


@gpu
def test_fused_track_and_candidates_against_the_oracle():
    """the chunks_basic golden on a fused context: T_SMOOTH (formed by the search) against the oracle's smoothed track in the default
    tier of assert_track, the candidates == the oracle's call_peaks of norm + smoothed, and they hold the reference's own"""
    from oracle import natac_oracle as O
    g = golden("chunks_basic")
    par = golden("params_example")
    pk = packed_from_golden(g, True)
    ctx = _context(True)
    try:
        b = ctx.upload(pk)
        def default_pass():
            b.run_nuc(10)
            return b.run_peaks(**BENCH)[:2]
        (cc, cp), n_smooth = _smooth_launches(ctx, default_pass)
        assert n_smooth == 0
        norm, sm = b.split(b.track(L.T_NORM)), b.split(b.track(L.T_SMOOTH))
        for k in range(pk.n_chunks):
            l, n = pk.chunk_frags(k)
            nt = O.nuc_chunk_tracks(l.astype(np.int64), n.astype(np.int64), 0, int(pk.chunk_len[k]), pk.chunk_bias(k), -pk.bias_left,
                                    par["vmat"], int(par["vlower"]), int(par["vupper"]), par["sizes"])
            assert_track(sm[k], nt["smoothed"], "smoothed")
            assert_track(sm[k], g["c%d_smoothed" % k], "smoothed (golden)")
            want = np.asarray(O.call_peaks((norm[k] + sm[k]).copy(), **BENCH), np.int32)
            assert np.array_equal(cp[cc == k], want)
            assert set(g["c%d_cands" % k][:, 0].astype(np.int32)) <= set(want)
        b.free()
    finally:
        ctx.close()
