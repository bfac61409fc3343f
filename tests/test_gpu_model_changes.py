"""GPU: model changes on a context that has run, and stages run again on a batch that lives through them (natac.h, rules A and B
above natac_set_vmat; DESIGN.md "State keyed on the model").

Every other parity test makes a fresh Context, sets one model, uploads a fresh batch, runs it and frees it.  The drivers do not:
get_context() is one context per process, `nucleoatac run` installs the occupancy model and then the V-plot and sizes on it, and
nuc_batch / occ_batch install their parameters before every batch.  Between those calls the context keeps tables derived from the
model (size weights, template spectra, log(V / s), windows, block weights, q4 / rho) and the batch keeps tables derived from the model's
geometry (background tiles, fragment ranges, grids, block-sum tables, heavy-tile lists) plus what its outputs were formed with.

test_rerun_after_model_change_equals_a_fresh_run (rule A) walks one context and one batch through models that differ from their
predecessor in one keyed quantity each and compares every output, bit for bit, with a fresh context and batch given the same model
and the same calls.  The fresh run's own parity with the oracle is test_gpu_vplot_arms.py (V-plot arms) and
test_gpu_generic_params.py (occupancy arms, smoothing widths); here the last visit of the first model is anchored to the oracle once
more, so that "fresh" is not the only reference.

test_consumers_after_a_model_change_do_not_mix_models (rule B) changes the model between a stage and the calls that read its outputs
next to the context's model.  Every group begins with a change that keeps the geometry, so that array sizes, steps and bounds are the
run's whatever the library does; the geometry-changing cases come after it and are reached only if it passed."""
import numpy as np
import pytest

from helpers import assert_track, cancel_scale, expand_grid, golden
from nucleoatac_amd import _lib as L
from nucleoatac_amd.packing import PackedChunks
from nucleoatac_amd.synth import synth_occ_distributions, synth_size_distribution, synth_sizes

pytestmark = pytest.mark.gpu

# chunk lengths for the golden V-plot's FFT tiles (392 plain / 424 extended outputs): only extended tiles (2120: 5, 848: 2), extended
# and plain (1203: 1 + 2, 4100: 6 + 4), one tile (393).  One chunk without fragments; one with 5 per base, so that a tile of 64 grid
# points (320 bases + the window) holds more fragments than the 512 natac_occ_decide stages in LDS.
LENS = [2120, 848, 1203, 393, 4100]
DENSITY = [0.3, 0.0, 5.0, 0.3, 0.3]
LENS_Y = [848, 2500, 393]
DENSITY_Y = [0.4, 0.3, 1.0]
NUC_TRACKS = (L.T_NUC_COV, L.T_NFR_COV, L.T_RAW, L.T_BACKGROUND, L.T_NORM, L.T_SMOOTH)
OCC_TRACKS = (L.T_OCC, L.T_OCC_LOWER, L.T_OCC_UPPER, L.T_OCC_COV, L.T_OCC_PREFILL)
GRIDS = (L.G_OCC, L.G_LOWER, L.G_UPPER)
PEAKS = dict(min_signal=0, sep=25, boundary=20, order=10)


def _batch(lens, density, seed):
    """ragged chunks with fragments of every size up to 330 (half of them nucleosome-like), centres from 150 bases left of the chunk
    to 150 right of it; bias normal(0, 0.7) over the default 246 / 247 halo"""
    rng = np.random.default_rng(seed)
    fr = []
    for Lc, d in zip(lens, density):
        nf = int(d * (Lc + 300))
        n = np.where(rng.random(nf) < 0.5, np.asarray(synth_sizes(rng, nf), dtype=np.int64), rng.integers(1, 330, size=nf))
        c = np.sort(rng.integers(-150, Lc + 150, size=nf))
        fr.append(((c - (n - 1) // 2).astype(np.int64), n.astype(np.int64)))
    off = np.concatenate(([0], np.cumsum([len(x[0]) for x in fr])))
    nb = [Lc + 246 + 247 for Lc in lens]
    bias = rng.normal(0, 0.7, size=sum(nb))
    pk = PackedChunks(np.arange(len(lens)) * 20000, lens, off, np.concatenate([x[0] for x in fr]), np.concatenate([x[1] for x in fr]),
                      np.concatenate(([0], np.cumsum(nb))), bias)
    return pk, fr


def _edge_positions(lens):
    """fixed candidate positions: both ends of every chunk, one window in from them, the middle"""
    ec, ep = [], []
    for k, Lc in enumerate(lens):
        pos = sorted({0, 1, 60, Lc // 2, Lc - 61, Lc - 1})
        ec += [k] * len(pos)
        ep += pos
    return np.array(ec, np.int32), np.array(ep, np.int32)


def _vplots():
    g = np.ascontiguousarray(golden("params_example")["vmat"])          # rows 105..251, w = 60
    rng = np.random.default_rng(11)

    def rnd(lo, up, w):
        return dict(mat=rng.random((up - lo, 2 * w + 1)) * 0.01 + 1e-4, lo=lo, up=up)
    return dict(golden=dict(mat=g, lo=105, up=251),
                values=dict(mat=g * rng.uniform(0.5, 1.5, size=g.shape), lo=105, up=251),   # the same geometry, other values
                even=rnd(104, 250, 60),                                      # even first size: natac_candidates_paired<false>
                w40=dict(mat=np.ascontiguousarray(g[:, 20:101]), lo=105, up=251),   # TV, ranges256_w and the background tiles change
                short=rnd(61, 121, 60),                                      # fewer rows ...
                w100=rnd(105, 251, 100),                                     # ... more again; W = 201 > 192: no FFT, column-loop candidates
                single=rnd(1, 147, 60))                                      # lower < 2: the generic background


def _occ_models():
    nucp, nfrp = synth_occ_distributions(251)

    def om(step, flank, upper=251, n_alpha=101, zero_nfr=False, zero_both=False):
        a, f = nucp[:upper].copy(), nfrp[:upper].copy()
        if zero_nfr:
            f[170:] = 0.0
        if zero_both:                           # a window that holds such a fragment has no likelihood: status bit 0 (Occupancy.py:118)
            a[140:161] = f[140:161] = 0.0
        return dict(nucp=a / a.sum(), nfrp=f / f.sum(), alphas=np.linspace(0, 1, n_alpha), step=step, flank=flank)
    return dict(default=om(5, 60),              # the V-plot's window and size range: natac_run_nuc writes OCC_COV
                f61=om(5, 61),                  # the same Q, another remainder; OCC_COV from the fragments
                s3=om(3, 60),                   # another grid
                s9=om(9, 44, upper=200, n_alpha=65),
                s11=om(11, 60),                 # the general kernel; OCC_PREFILL written, not pending
                a112=om(5, 60, n_alpha=112),    # natac_occ_mle<5, 60, 0, 1>
                zf=om(5, 60, zero_nfr=True), both=om(5, 60, zero_both=True), f40=om(5, 40),
                f45=om(5, 45), f75=om(5, 75), a65=om(5, 60, n_alpha=65))


def _install(ctx, m, prev=None):
    """set the model `m` on the context; with `prev` (the model the context holds), only the setters whose argument changed"""
    if prev is None or m["v"] is not prev["v"]:
        ctx.set_vmat(m["v"]["mat"], m["v"]["lo"], m["v"]["up"])
    if prev is None or m["sizes"] is not prev["sizes"]:
        ctx.set_sizes(m["sizes"])
    if prev is None or m["occ"] is not prev["occ"]:
        o = m["occ"]
        ctx.set_occ_model(o["nucp"], o["nfrp"], alphas=o["alphas"], step=o["step"], flank=o["flank"])


def _run(b, m, calls):
    for s in calls:
        if s == "nuc":
            b.run_nuc(m["sd"])
        else:
            b.run_occ()


def _read(b, calls, cand):
    """every output of the stages in `calls`, in one fixed order"""
    out = {}
    if "nuc" in calls:
        for t in NUC_TRACKS:
            out["track %d" % t] = b.track(t)
        for name, a in zip(("cc", "cp", "lr", "var", "z"), b.run_peaks(**PEAKS)):
            out["peaks " + name] = a
        for name, a in zip(("lr", "var", "z"), b.run_candidates(*cand)):
            out["candidates " + name] = a
    if "occ" in calls:
        for g in GRIDS:
            out["grid %d" % g] = b.grid(g)
        for t in OCC_TRACKS:
            out["track %d" % t] = b.track(t)
        for name, a in zip(("cc", "cp", "occ", "lower", "upper", "reads", "keep", "nuc_dist"), b.run_occ_peaks(min_occ=0.1, sep=120)):
            out["occ_peaks " + name] = a
    out["status"] = b.status()
    return out


def _fresh(m, calls, pk, cand):
    """`calls` on a new Context and a new batch"""
    from nucleoatac_amd.device import Context
    with Context(0) as c:
        _install(c, m)
        b = c.upload(pk)
        _run(b, m, calls)
        out = _read(b, calls, cand)
        b.free()
    return out


def _same(a, b, what):
    """float64 arrays as uint64 views with equal NaN positions, integers exactly"""
    assert sorted(a) == sorted(b), what
    for k in sorted(a):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        if x.dtype == np.float64:
            nan = np.isnan(x)
            assert np.array_equal(nan, np.isnan(y)), "%s: %s: NaN positions differ" % (what, k)
            diff = (x.view(np.uint64) != y.view(np.uint64)) & ~nan
            assert not diff.any(), "%s: %s: %d of %d values differ, max |d| = %g" % (
                what, k, int(diff.sum()), x.size, float(np.max(np.abs(x[diff] - y[diff]))))
        else:
            assert np.array_equal(x, y), "%s: %s differs" % (what, k)


def _code(call):
    with pytest.raises(L.NatacError) as e:
        call()
    return e.value.code


def test_rerun_after_model_change_equals_a_fresh_run():
    from nucleoatac_amd.device import Context
    from oracle import natac_oracle as O
    V, OM = _vplots(), _occ_models()
    sizes = synth_size_distribution(251)
    sizes2 = sizes * np.linspace(0.3, 3.0, 251)            # positive wherever `sizes` is; the rows' weights change by up to 10x
    sizes2 /= sizes2.sum()
    first = dict(v=V["golden"], sizes=sizes, sd=10, occ=OM["default"])
    NO, ON, N, O1 = ("nuc", "occ"), ("occ", "nuc"), ("nuc",), ("occ",)
    # (what changes, calls on X, run Y too, release X's outputs first)
    walk = [(dict(), NO, False, False),
            (dict(v=V["values"]), NO, False, False),
            (dict(sizes=sizes2), NO, False, False),
            (dict(v=V["even"]), NO, False, False),
            (dict(v=V["w40"]), NO, True, False),          # Y: uploaded before this change, first run after it
            (dict(v=V["short"]), NO, False, False),
            (dict(v=V["w100"]), NO, True, False),         # Y again, two changes later
            (dict(v=V["single"]), NO, False, False),
            (dict(v=V["golden"], sizes=sizes), NO, True, False),      # the first model again
            (dict(sd=5), N, False, False),                # natac_smooth_same instead of natac_smooth_same4; the window cache
            (dict(sd=12), N, False, False),
            (dict(sd=10), N, True, False),
            (dict(occ=OM["f61"]), NO, False, False),
            (dict(occ=OM["s3"]), O1, True, False),        # occ alone
            (dict(occ=OM["s9"]), ("occ", "occ"), False, False),
            (dict(occ=OM["s11"]), ON, True, False),
            (dict(occ=OM["a112"]), NO, False, True),      # natac_batch_release_outputs between two models
            (dict(occ=OM["both"]), NO, True, False),      # raises status bit 0 on X and Y: the next model's re-run must drop it
            (dict(occ=OM["zf"]), ON, True, False),        # the fast path after occ -> nuc: exp(bias) must be formed, not assumed
            (dict(occ=OM["default"]), NO, True, False)]   # the first model again
    pkx, frx = _batch(LENS, DENSITY, seed=5)
    pky, _ = _batch(LENS_Y, DENSITY_Y, seed=6)
    candx, candy = _edge_positions(LENS), _edge_positions(LENS_Y)
    visits = []
    with Context(0) as c:
        x, y = c.upload(pkx), None
        m = prev = None
        for i, (change, calls, with_y, release) in enumerate(walk):
            if i == 4:
                y = c.upload(pky)
            m = dict(first if m is None else m, **change)
            _install(c, m, prev)
            prev = m
            if i == 0:
                assert [c.bg_tiling(n) for n in LENS] == [(5, 5), (2, 2), (3, 1), (1, 1), (10, 6)]
            if release:
                x.release_outputs()
            what = "step %d (%s)" % (i, ", ".join(sorted(change)) or "first model")
            if with_y:                                    # the two batches' stages interleaved
                for s in calls:
                    _run(x, m, (s,))
                    _run(y, m, (s,))
            else:
                _run(x, m, calls)
            got = _read(x, calls, candx)
            _same(got, _fresh(m, calls, pkx, candx), what + ", X")
            if with_y:
                _same(_read(y, calls, candy), _fresh(m, calls, pky, candy), what + ", Y")
            visits.append(got)
            if m["occ"] is OM["both"]:                    # every chunk with fragments holds some of the sizes 140..160
                assert (got["status"] & 1).any() and got["status"][1] == 0 and not (got["status"] & ~1).any(), what
            else:
                assert not got["status"].any(), what
        last = visits[-1]
        _same(last, visits[0], "the first model's last visit against its first")
        _same({k: v for k, v in visits[8].items() if k in visits[11]}, visits[11], "smooth_sd 10 again")
        # not a vacuous comparison: peaks with statistics in every chunk that has fragments, and occupancy peaks
        assert sorted(set(last["peaks cc"])) == [0, 2, 3, 4] and len(last["occ_peaks cc"]) > 0
        x.free()
        y.free()
    # anchors: the dense chunk and the one-tile chunk of the last visit against the oracle
    g = first["v"]
    o = first["occ"]
    goff = np.concatenate(([0], np.cumsum([len(range(2, n, 5)) for n in LENS])))
    boff = np.concatenate(([0], np.cumsum(LENS)))
    for k in (2, 3):
        l, n = frx[k]
        Lc, sl = LENS[k], slice(int(boff[k]), int(boff[k + 1]))
        nt = O.nuc_chunk_tracks(l, n, 0, Lc, pkx.chunk_bias(k), -246, g["mat"], g["lo"], g["up"], sizes, smooth_sd=10)
        cs = cancel_scale(nt["raw"], nt["bg"])
        assert_track(last["track %d" % L.T_NUC_COV][sl], nt["nuc_cov"], "nuc_cov", exact=True)
        assert_track(last["track %d" % L.T_NFR_COV][sl], nt["nfr_cov"], "nfr_cov", exact=True)
        assert_track(last["track %d" % L.T_RAW][sl], nt["raw"], "raw")
        assert_track(last["track %d" % L.T_BACKGROUND][sl], nt["bg"], "bg")
        assert_track(last["track %d" % L.T_NORM][sl], nt["norm"], "norm", scale=cs)
        assert_track(last["track %d" % L.T_SMOOTH][sl], nt["smoothed"], "smoothed", scale=cs)
        oc = O.occ_chunk_tracks(l, n, 0, Lc, pkx.chunk_bias(k), -246, o["nucp"], o["nfrp"])
        for gi, key in zip(GRIDS, ("occ", "occ_lower", "occ_upper")):
            assert_track(expand_grid(last["grid %d" % gi][int(goff[k]):int(goff[k + 1])], Lc, 5), oc[key], key, exact=True)
        assert_track(last["track %d" % L.T_OCC_PREFILL][sl], oc["smoothed_vals"], "smoothed occ")
        assert_track(last["track %d" % L.T_OCC_LOWER][sl], oc["smoothed_lower"], "smoothed lower")
        assert_track(last["track %d" % L.T_OCC_UPPER][sl], oc["smoothed_upper"], "smoothed upper")
        assert_track(last["track %d" % L.T_OCC_COV][sl], oc["cov"], "occ cov", exact=True)


def test_consumers_after_a_model_change_do_not_mix_models():
    from nucleoatac_amd.device import Context, TrackStore
    from test_gpu_vplot_arms import _assert_stats, _reference_stats
    from oracle import natac_oracle as O
    V, OM = _vplots(), _occ_models()
    sizes = synth_size_distribution(251)
    sizes_b = sizes * np.linspace(0.3, 3.0, 251)           # clearly other size weights, positive wherever `sizes` is
    sizes_b /= sizes_b.sum()
    A = dict(v=V["golden"], sizes=sizes, sd=10, occ=OM["default"])
    B = dict(A, v=V["values"], sizes=sizes_b)
    pkx, frx = _batch(LENS, DENSITY, seed=5)
    pky, _ = _batch(LENS_Y, DENSITY_Y, seed=6)
    cand = _edge_positions(LENS)
    chroms = ["chr1"] * pkx.n_chunks
    with Context(0) as c:
        # ---- candidates: the statistics of the model that is set now, with its own size weights
        _install(c, A)
        x, y = c.upload(pkx), c.upload(pky)
        x.run_nuc(10)
        peaks, stats = x.run_peaks(**PEAKS), x.run_candidates(*cand)
        _install(c, B, A)
        y.run_nuc(10)                                     # the context's size weights are B's now
        _install(c, A, B)
        again_peaks, again_stats = x.run_peaks(**PEAKS), x.run_candidates(*cand)      # no natac_run_nuc in between
        assert np.array_equal(again_peaks[0], peaks[0]) and np.array_equal(again_peaks[1], peaks[1])
        # the window sums now come from the kernel itself (a newer model generation than bnum / bcov): the bound between candidate
        # arms of test_gpu_vplot_arms.py, scales from the oracle
        g = A["v"]
        nts = [O.nuc_chunk_tracks(l, n, 0, Lc, pkx.chunk_bias(k), -246, g["mat"], g["lo"], g["up"], sizes, smooth_sd=10)
               for k, ((l, n), Lc) in enumerate(zip(frx, LENS))]
        allc, allp = np.concatenate((peaks[0], cand[0])), np.concatenate((peaks[1], cand[1]))
        _, scales = _reference_stats(nts, g["mat"], g["lo"], g["up"], allc, allp)
        _assert_stats([np.concatenate((a, b)) for a, b in zip(again_peaks[2:], again_stats)],
                      [np.concatenate((a, b)) for a, b in zip(peaks[2:], stats)], scales, "after B and A again")
        assert sorted(set(peaks[0])) == [0, 2, 3, 4] and np.isfinite(peaks[2]).all()
        # another width: the tracks are w = 60's
        W40 = dict(A, v=V["w40"])
        _install(c, W40, A)
        assert _code(lambda: x.run_candidates(*cand)) == -3
        assert _code(lambda: x.run_peaks(**PEAKS)) == -3
        assert _code(lambda: x.run_candidates_cov(*cand)) == -3
        x.run_nuc(10)
        _same(_read(x, ("nuc",), cand), _fresh(W40, ("nuc",), pkx, cand), "natac_run_nuc after the refusals")
        # the same width and last size, one row less at the top
        _install(c, A, W40)
        x.run_nuc(10)
        LOWER = dict(A, v=dict(mat=np.ascontiguousarray(g["mat"][1:]), lo=106, up=251))
        _install(c, LOWER, A)
        assert _code(lambda: x.run_candidates(*cand)) == -3
        assert _code(lambda: x.run_peaks(**PEAKS)) == -3
        x.run_nuc(10)
        _same(_read(x, ("nuc",), cand), _fresh(LOWER, ("nuc",), pkx, cand), "natac_run_nuc after the refusals (lower)")

        # ---- background: formed on request from what natac_run_nuc left, not from the model
        _install(c, A, LOWER)
        twin = c.upload(pkx)
        x.run_nuc(10)
        twin.run_nuc(10)
        want = twin.track(L.T_BACKGROUND)
        _install(c, dict(A, v=V["values"]), A)
        _same(dict(bg=x.track(L.T_BACKGROUND)), dict(bg=want), "a pending BACKGROUND after natac_set_vmat")
        y.free()

        # ---- occupancy: OCC_PREFILL formed on request, natac_run_occ_peaks
        _install(c, A)
        live = [x] + [c.upload(pkx) for _ in range(3)]
        z = c.upload(pky)
        for b in live + [twin]:
            b.run_occ()
        store = TrackStore()

        def adopted(b):
            seg = store.adopt(b, [L.T_OCC_PREFILL])
            assert seg is not None
            return store.read(c, [seg], [0], [pkx.total_bp], 0)

        def occ_peaks(b):
            return dict(zip("abcdefgh", b.run_occ_peaks(min_occ=0.1, sep=120)))
        want_peaks = occ_peaks(twin)
        want_text = twin.format_track(L.T_OCC_PREFILL, chroms, pkx.chunk_start, compress=False)[0].tobytes()
        want_pre = twin.track(L.T_OCC_PREFILL)
        want_store = adopted(twin)
        F75, A65 = dict(A, occ=OM["f75"]), dict(A, occ=OM["a65"])
        _install(c, F75, A)
        z.run_occ()                                       # the context's smoothing window is flank 75's now (longer, not shorter)
        _install(c, A65, F75)                             # the run's geometry, another alpha grid
        _same(dict(p=live[0].track(L.T_OCC_PREFILL)), dict(p=want_pre), "a pending OCC_PREFILL after natac_set_occ_model")
        _same(occ_peaks(live[1]), want_peaks, "natac_run_occ_peaks after natac_set_occ_model")
        assert live[2].format_track(L.T_OCC_PREFILL, chroms, pkx.chunk_start, compress=False)[0].tobytes() == want_text
        _same(dict(s=adopted(live[3])), dict(s=want_store), "natac_store_adopt after natac_set_occ_model")
        for b in live:
            b.run_occ()                                   # OCC_PREFILL is pending again
        F45 = dict(A, occ=OM["f45"])

        def refused():
            assert _code(lambda: live[0].track(L.T_OCC_PREFILL)) == -3
            assert _code(lambda: live[1].run_occ_peaks(min_occ=0.1, sep=120)) == -3
            assert _code(lambda: live[2].format_track(L.T_OCC_PREFILL, chroms, pkx.chunk_start, compress=False)) == -3
            assert _code(lambda: store.adopt(live[3], [L.T_OCC_PREFILL])) == -3
        _install(c, F45, A65)
        refused()
        fresh65 = _fresh(A65, ("occ",), pkx, cand)
        for gi in GRIDS:                                  # the grids and the formed tracks stay the run's
            _same(dict(g=x.grid(gi)), dict(g=fresh65["grid %d" % gi]), "grid after the refusals")
        _same({k: v for k, v in fresh65.items() if k.startswith("track") and not k.endswith(" %d" % L.T_OCC_PREFILL)},
              {"track %d" % t: x.track(t) for t in OCC_TRACKS[:4]}, "formed tracks stay readable")
        x.run_occ()                                       # the same step: the grid keeps its layout
        _same(_read(x, ("occ",), cand), _fresh(F45, ("occ",), pkx, cand), "natac_run_occ after the refusals (flank 45)")
        x.run_occ()                                       # OCC_PREFILL pending again, under flank 45
        S3 = dict(A, occ=OM["s3"])
        _install(c, S3, F45)                              # only now: a smaller step, the grid holds fewer points than it implies
        refused()
        x.run_occ()
        _same(_read(x, ("occ",), cand), _fresh(S3, ("occ",), pkx, cand), "natac_run_occ after the refusals")
        store.close()

        # ---- OCC_COV: natac_run_nuc writes it on the side only while it is its own
        F61 = dict(A, occ=OM["f61"])
        _install(c, F61, S3)
        x.run_occ()
        cov61 = x.track(L.T_OCC_COV)
        _install(c, A, F61)                               # the V-plot's window and size range
        x.run_nuc(10)
        _same(dict(c=x.track(L.T_OCC_COV)), dict(c=cov61), "OCC_COV of natac_run_occ after natac_run_nuc")
        x.run_occ()
        _same(_read(x, ("nuc", "occ"), cand), _fresh(A, ("nuc", "occ"), pkx, cand), "nuc and occ after all of it")
        # ... and its own only for the window it wrote it for: nuc + occ under w = flank = 60, then both become 40
        u = c.upload(pkx)
        u.run_nuc(10)
        u.run_occ()
        cov60 = u.track(L.T_OCC_COV)
        W40F40 = dict(A, v=V["w40"], occ=OM["f40"])
        _install(c, W40F40, A)
        u.run_nuc(10)
        _same(dict(c=u.track(L.T_OCC_COV)), dict(c=cov60), "OCC_COV of flank 60 after natac_run_nuc under w = 40")
        u.run_occ()
        _same(_read(u, ("nuc", "occ"), cand), _fresh(W40F40, ("nuc", "occ"), pkx, cand), "nuc and occ under w = flank = 40")
        u.free()
        for b in live + [twin, z]:
            b.free()
