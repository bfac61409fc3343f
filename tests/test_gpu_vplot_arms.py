"""GPU: every kernel arm that the V-plot's geometry selects for the nucleosome stage, against the oracle.

The host picks the candidate kernel (launch_candidates) and the background kernel (run_nuc, fft_bg_applicable) from the V-plot's
bounds and width.  With A = (upper - 2) >> 1, Bh = (upper - 1) >> 1 and EW = W + A + Bh:

    lower..upper  w (W)     candidates                      background
    105..251     60 (121)   natac_candidates_paired<true>   FFT
    110..250     60 (121)   natac_candidates_paired<false>  FFT
    105..250     63 (127)   natac_candidates4<true>         FFT        odd row count; the widest template of the per-wave kernels
     40..140     64 (129)   natac_candidates                FFT        wider than 128 columns: the per-wave kernels cannot hold it
     41..141     80 (161)   natac_candidates                FFT
    105..250     80 (161)   natac_candidates                FFT
    105..251     96 (193)   natac_candidates                generic    W > 192
    105..251     96 (193)   natac_candidates                generic    exact zero cells in the template: lr = NaN
    105..251    120 (241)   natac_candidates                generic
    105..400     60 (121)   natac_candidates                FFT        EW too large for the per-wave kernels' LDS

Per case: the per-base tracks of a ragged batch (FFT cases: chunks of only extended tiles, of extended and plain tiles, of plain tiles,
and one shorter than a tile; a sparse chunk where nuc_cov = 0 gives var = 0), lr / var / z of every candidate run_peaks finds and of
positions whose window reaches into the bias flanks, all against the oracle; then the same candidates through the validation switches
NATAC_CAND_OLD / NATAC_CAND_FULL (natac_candidates4<false> for W <= 128) and the background through NATAC_BG_DIRECT, against the
default arm."""
import os

import numpy as np
import pytest

from helpers import _assert_stats, _reference_stats, assert_track, cancel_scale, golden
from nucleoatac_amd import _lib as L
from nucleoatac_amd.packing import PackedChunks
from nucleoatac_amd.synth import synth_centres, synth_size_distribution, synth_sizes

pytestmark = pytest.mark.gpu

BL = BR = 400          # bias flanks: the widest case needs W + A = 365 (w = 120) / 320 (upper = 400) bases on each side
SPARSE_LEN = 700       # fragments only near its left end: nuc_cov = 0 over the rest
TRACKS = (L.T_NUC_COV, L.T_NFR_COV, L.T_RAW, L.T_BACKGROUND, L.T_NORM, L.T_SMOOTH)
PEAKS = dict(min_signal=0, sep=25, boundary=20, order=10)

CASES = [
    pytest.param(105, 251, 60, False, id="105-251-w60"),
    pytest.param(110, 250, 60, False, id="110-250-w60"),
    pytest.param(105, 250, 63, False, id="105-250-w63"),
    pytest.param(40, 140, 64, False, id="40-140-w64"),
    pytest.param(41, 141, 80, False, id="41-141-w80"),
    pytest.param(105, 250, 80, False, id="105-250-w80"),
    pytest.param(105, 251, 96, False, id="105-251-w96"),
    pytest.param(105, 251, 96, True, id="105-251-w96-zero-cells"),
    pytest.param(105, 251, 120, False, id="105-251-w120"),
    pytest.param(105, 400, 60, False, id="105-400-w60"),
]


def _vmat(lo, up, w, zero):
    if lo >= 105 and up <= 251 and w <= 60:
        vm = np.ascontiguousarray(golden("params_example")["vmat"][lo - 105:up - 105, 60 - w:60 + w + 1])
    else:
        rng = np.random.default_rng(lo * 1000 + up + w)
        vm = rng.random((up - lo, 2 * w + 1)) * 0.01 + 1e-4
    if zero:
        R, W = vm.shape
        vm[R // 3, W // 5] = 0.0
        vm[2 * R // 3, W - 3] = 0.0          # a column past 128
    return vm


def _lengths(ctx, W):
    """chunk lengths for the FFT background's tilings (natac_bg_tiling): only extended tiles, extended + plain, only plain (two or more
    tiles each), and one chunk shorter than a tile; fixed lengths for the generic kernel"""
    nt, _ = ctx.bg_tiling(1000)
    if nt == 0:
        return [817, 425, 150]
    found = {}
    for Lc in range(300, 3000):
        nt, ex = ctx.bg_tiling(Lc)
        if nt < 2:
            continue
        kind = "extended" if ex == nt else ("mixed" if ex > 0 else "plain")
        found.setdefault(kind, Lc)
        if len(found) == 3:
            break
    assert sorted(found) == ["extended", "mixed", "plain"], found
    short = 150
    assert short < 512 - W + 1 and ctx.bg_tiling(short) == (1, 0)
    return [found["extended"], found["mixed"], found["plain"], short]


def _batch(lens, up, seed):
    rng = np.random.default_rng(seed)
    fr = []
    for Lc in lens:
        if Lc == SPARSE_LEN:
            n = rng.integers(1, up + 20, size=8)
            c = np.sort(rng.integers(0, 120, size=8))
        else:
            nf = 3 * Lc                 # every insert size of the V-plot and beyond, half of them nucleosome-like; phased centres
            n = np.where(rng.random(nf) < 0.5, synth_sizes(rng, nf), rng.integers(1, up + 20, size=nf))
            c = np.sort(synth_centres(rng, nf, Lc + 300, period=90, band=3, enrich=8.0) - 150)
        fr.append((c - (n - 1) // 2, n))
    off = np.concatenate(([0], np.cumsum([len(x[0]) for x in fr])))
    nb = [Lc + BL + BR for Lc in lens]
    bias = rng.normal(0, 0.7, size=sum(nb))
    pk = PackedChunks(np.arange(len(lens)) * 20000, lens, off, np.concatenate([x[0] for x in fr]), np.concatenate([x[1] for x in fr]),
                      np.concatenate(([0], np.cumsum(nb))), bias, bias_left=BL, bias_right=BR)
    return pk, fr


@pytest.mark.parametrize("lo,up,w,zero", CASES)
def test_vplot_geometry_arms(lo, up, w, zero):
    from nucleoatac_amd.device import Context
    from oracle import natac_oracle as O
    vm = _vmat(lo, up, w, zero)
    W = 2 * w + 1
    sizes = synth_size_distribution(max(up, 251))[:up]
    with Context(0) as c:
        c.set_vmat(vm, lo, up)
        c.set_sizes(sizes)
        lens = _lengths(c, W) + [SPARSE_LEN]
        pk, fr = _batch(lens, up, seed=lo * 7 + up + w)
        b = c.upload(pk)
        b.run_nuc(10)
        tr = {t: b.split(b.track(t)) for t in TRACKS}
        cc, cp, lr, var, z = b.run_peaks(**PEAKS)
        # positions whose window reaches into the bias flanks on either side
        ec, ep = [], []
        for k, Lc in enumerate(lens):
            pos = sorted({p for p in (0, 1, w, Lc - w - 1, Lc - 1) if 0 <= p < Lc})
            ec += [k] * len(pos)
            ep += pos
        ec, ep = np.array(ec, np.int32), np.array(ep, np.int32)
        elr, evar, ez = b.run_candidates(ec, ep)
        allc, allp = np.concatenate((cc, ec)), np.concatenate((cp, ep))
        mine = (np.concatenate((lr, elr)), np.concatenate((var, evar)), np.concatenate((z, ez)))
        # the peak search's statistics are natac_run_candidates' at the same positions, bit for bit
        again = b.run_candidates(cc, cp)
        for g, a in zip((lr, var, z), again):
            assert np.array_equal(g, a, equal_nan=True)
        arms = {}
        for switch in ("NATAC_CAND_OLD", "NATAC_CAND_FULL"):     # read at every launch
            os.environ[switch] = "1"
            try:
                arms[switch] = b.run_candidates(allc, allp)
            finally:
                os.environ.pop(switch, None)
        b.free()
    os.environ["NATAC_BG_DIRECT"] = "1"                          # read when a context is created
    try:
        with Context(0) as c:
            c.set_vmat(vm, lo, up)
            c.set_sizes(sizes)
            b = c.upload(pk)
            b.run_nuc(10)
            direct = {t: b.split(b.track(t)) for t in (L.T_BACKGROUND, L.T_NORM, L.T_SMOOTH)}
            arms["NATAC_BG_DIRECT"] = b.run_candidates(allc, allp)
            b.free()
    finally:
        os.environ.pop("NATAC_BG_DIRECT", None)

    nts = []
    for k, Lc in enumerate(lens):
        l, n = fr[k]
        nt = O.nuc_chunk_tracks(l, n, 0, Lc, pk.chunk_bias(k), -BL, vm, lo, up, sizes, smooth_sd=10)
        nts.append(nt)
        cs = cancel_scale(nt["raw"], nt["bg"])
        assert_track(tr[L.T_NUC_COV][k], nt["nuc_cov"], "nuc_cov", exact=True)
        assert_track(tr[L.T_NFR_COV][k], nt["nfr_cov"], "nfr_cov", exact=True)
        assert_track(tr[L.T_RAW][k], nt["raw"], "raw")
        assert_track(tr[L.T_BACKGROUND][k], nt["bg"], "bg")
        assert_track(tr[L.T_NORM][k], nt["norm"], "norm", scale=cs)
        assert_track(tr[L.T_SMOOTH][k], nt["smoothed"], "smoothed", scale=cs)
        assert_track(direct[L.T_BACKGROUND][k], tr[L.T_BACKGROUND][k], "bg direct")
        assert_track(direct[L.T_NORM][k], tr[L.T_NORM][k], "norm direct", scale=cs)
        assert_track(direct[L.T_SMOOTH][k], tr[L.T_SMOOTH][k], "smoothed direct", scale=cs)
        hp = np.asarray(O.call_peaks((tr[L.T_NORM][k] + tr[L.T_SMOOTH][k]).copy(), **PEAKS), np.int64)
        assert np.array_equal(cp[cc == k], hp), "peaks of chunk %d" % k
    assert len(cc) >= 15
    ref, scales = _reference_stats(nts, vm, lo, up, allc, allp)
    _assert_stats(mine, ref, scales, "oracle")
    assert (ref[1] == 0).any() and (ref[1] > 0).any()          # the sparse chunk's empty windows and ordinary ones
    if zero:
        assert np.isnan(ref[0]).all()                           # every window holds the template's zero cells
    else:
        assert not np.isnan(ref[0]).any()
    for name, got in arms.items():
        _assert_stats(got, mine, scales, name)
