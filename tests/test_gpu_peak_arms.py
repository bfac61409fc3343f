"""Every dispatch arm of the device peak search (peaks_plan / peaks_enqueue, nucleoatac_amd/csrc/natac_peaks.hpp) against the host
restatement of utils.call_peaks, chunk and position exact.

peaks_plan picks the kernel from the LONGEST chunk of the batch (maxL) and `order`: natac_peaks_chunk_reg<NJ, 256> up to 4,096
bases, natac_peaks_chunk_reg<NJ, 1024> up to 16,384 bases while its LDS fits 150 KB, else the segmented natac_peaks_chunk with LDS
or global peak lists.  Inside the register kernel the maxima test keeps the row masks in registers, runs two phases over a survivor
list, or runs the direct test.  peak_arm() below restates that choice; test_cases_cover_every_arm (CPU) checks that the cases reach
every arm and that the restatement is the library's plan (natac_peaks_plan), field by field, for every maxL up to 20,000.  The register kernels keep at most PEAK_MAX maxima per chunk and
flag a chunk with more (status value 2) for the drivers' host fallback: every search here predicts that flag on the host and checks
it chunk by chunk."""
from collections import namedtuple

import numpy as np
import pytest

from helpers import call_peaks_stable, golden
from nucleoatac_amd import _lib as L
from nucleoatac_amd.packing import PackedChunks

PEAK_MAX = 2048          # natac_peaks.hpp: constexpr int PEAK_MAX
LDS_REG_MAX = 150 * 1024

Arm = namedtuple("Arm", "kernel bt nj mask global_lists")


def pk_cap_of(maxL, order):
    """natac_peaks.hpp, peaks_list_cap: min(PEAK_MAX, maxL / (order + 1) + 2) rounded up to a multiple of 8"""
    return (min(PEAK_MAX, maxL // (order + 1) + 2) + 7) & ~7


def peak_arm(maxL, order):
    """the kernel the library launches for a batch whose longest chunk has maxL bases, written out here on its own (natac_peaks.hpp
    states it in peaks_plan: pk_cap, the 13-byte list region, bt / nj, the register variants' LDS against 150 KB, the segmented kernel
    with `maxL / (order + 1) + 2 > pk_cap` for the global lists) and the maxima test inside the register kernel (natac_peaks_chunk_reg:
    the per-wave stride, two phases, and `stride < NJ * 8` for the masks in registers)"""
    pk_cap = pk_cap_of(maxL, order)
    lds_lists = pk_cap * (8 + 4 + 1)
    bt = 256 if maxL <= 4096 else 1024
    nj = (maxL + bt - 1) // bt
    lds_reg = ((bt * nj + 2 * order + 1) & ~1) * 8 + lds_lists
    if bt == 256 or (nj <= 16 and lds_reg <= LDS_REG_MAX):
        stride = (lds_lists // (bt // 64)) & ~7
        if stride < nj * 8:
            mask = "registers"
        elif order > 2 and stride >= nj * 8 + 2 * 128:
            mask = "two_phase"
        else:
            mask = "direct"
        return Arm("reg", bt, nj, mask, False)
    return Arm("seg", 256, None, None, maxL // (order + 1) + 2 > pk_cap)


def overflows(arm, maxL, order, n_maxima):
    """status value 2: a register kernel met more maxima (after the thresholds) than its lists hold"""
    return arm.kernel == "reg" and n_maxima > pk_cap_of(maxL, order)


# (order, boundary, sep, min_signal) of every search; every case length runs all of them.  Order 30 fills the two-phase survivor
# list of the 256-thread kernels at NJ >= 10 on white noise (4,096 bases: 156 entries per wave for ~200 survivors of distances
# 1 and 2, with min_signal -10 letting every one through), so the rows after it take the direct test
PARAMS = [(1, 0, 1, 0.0), (1, 60, 120, 0.1), (2, 0, 2, 0.0), (3, 60, 25, 0.0), (12, 0, 25, 0.5), (12, 60, 3, 0.0),
          (30, 0, 25, -10.0), (150, 60, 120, 0.0), (255, 0, 7, 0.0)]
ORDERS = sorted(set(p[0] for p in PARAMS))
# the longest chunk of a batch sits at an arm's edges: BT * NJ and BT * (NJ - 1) + 1 bases; past 16,384 the segmented kernel
LENGTHS = sorted(set([256 * nj for nj in range(1, 17)] + [256 * (nj - 1) + 1 for nj in range(1, 17)] +
                     [1024 * nj for nj in range(5, 17)] + [1024 * (nj - 1) + 1 for nj in range(5, 17)] + [16385, 20000]))
# run_peaks (norm + smoothed with statistics) on natac_run_nuc output: the upper edge of every instance and the segmented kernel
NUC_LENGTHS = [256 * nj for nj in range(1, 17)] + [1024 * nj for nj in range(5, 17)] + [16385]
NUC_PARAMS = [(12, 60, 25, 0.0), (1, 60, 2, 0.0)]


ARM_ORDERS = (1, 2, 3, 4, 8, 12, 30, 150, 255)


def all_arms():
    """every arm the dispatcher has: the 16 + 12 register instances, each with the mask modes it can take, the segmented kernel
    with LDS and with global lists"""
    arms = set()
    for maxL in range(1, 20001):
        for order in ARM_ORDERS:
            arms.add(peak_arm(maxL, order))
    return arms


def library_arm(maxL, order):
    """(Arm, pk_cap) of the library's own plan (natac_peaks_plan: host only)"""
    from nucleoatac_amd.device import peaks_plan
    p = peaks_plan(maxL, order)
    return Arm(p["kernel"], p["bt"], p["nj"], p["mask"], p["global_lists"]), p["pk_cap"]


def launched_instances():
    """the natac_peaks_chunk_reg<NJ, BT> instances the library's plan launches over the lengths and orders all_arms() walks"""
    plans = (library_arm(maxL, order)[0] for maxL in range(1, 20001) for order in ARM_ORDERS)
    return set((a.bt, a.nj) for a in plans if a.kernel == "reg")


def test_cases_cover_every_arm():
    """CPU: the model is the library's plan in every field (kernel, bt, nj, mask, global lists, pk_cap) for every maxL in 1..20000 and
    every order all_arms() walks, and the cases below reach every instance, every mask mode, both segmented variants and the
    fall-through of NJ = 16 at 1,024 threads to the segmented kernel (lds_reg > 150 KB)"""
    for maxL in range(1, 20001):
        for order in ARM_ORDERS:
            assert library_arm(maxL, order) == (peak_arm(maxL, order), pk_cap_of(maxL, order)), (maxL, order)
    model = set((a.bt, a.nj) for a in all_arms() if a.kernel == "reg")
    assert model == launched_instances()
    assert model == set((256, nj) for nj in range(1, 17)) | set((1024, nj) for nj in range(5, 17))
    reached = set(peak_arm(m, o) for m in LENGTHS for o in ORDERS)
    assert set((a.bt, a.nj) for a in reached if a.kernel == "reg") == model
    assert set(a.mask for a in reached if a.kernel == "reg") == {"registers", "two_phase", "direct"}
    for bt in (256, 1024):
        assert set(a.mask for a in reached if a.kernel == "reg" and a.bt == bt) == {"registers", "two_phase", "direct"}, bt
    assert set(a.global_lists for a in reached if a.kernel == "seg") == {True, False}
    falls = set((m, o) for m in LENGTHS for o in ORDERS if m <= 16384 and peak_arm(m, o).kernel == "seg")
    assert falls and all((m + 1023) // 1024 == 16 for m, _ in falls)
    # every arm the dispatcher has is among those reached
    assert all_arms() <= reached
    # the run_peaks cases reach every instance and both kernels too
    nuc = set(peak_arm(m, o) for m in NUC_LENGTHS for o, _, _, _ in NUC_PARAMS)
    assert set((a.bt, a.nj) for a in nuc if a.kernel == "reg") == model and any(a.kernel == "seg" for a in nuc)


def test_peak_arm_examples():
    """CPU: spot values of the model worked out by hand from peaks_plan"""
    assert peak_arm(4096, 150) == Arm("reg", 256, 16, "registers", False)        # pk_cap 32: 104-byte stride for 128 bytes of masks
    assert peak_arm(4096, 12) == Arm("reg", 256, 16, "two_phase", False)
    assert peak_arm(4096, 1) == Arm("reg", 256, 16, "direct", False)
    assert peak_arm(4097, 1) == Arm("reg", 1024, 5, "direct", False)
    assert peak_arm(15360, 1) == Arm("reg", 1024, 15, "direct", False)          # 122,880 + 26,624 bytes of LDS
    assert peak_arm(15361, 1) == Arm("seg", 256, None, None, True)              # 131,088 + 26,624 > 150 KB
    assert peak_arm(16384, 8) == Arm("seg", 256, None, None, False)             # lists of 1,824: LDS
    assert peak_arm(16384, 12) == Arm("reg", 1024, 16, "two_phase", False)
    assert peak_arm(16385, 12) == Arm("seg", 256, None, None, False)
    assert peak_arm(16385, 1) == Arm("seg", 256, None, None, True)
    assert pk_cap_of(5000, 1) == PEAK_MAX


# ---- GPU ------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def ctx():
    from nucleoatac_amd.device import Context
    par = golden("params_example")
    c = Context(0)
    c.set_vmat(par["vmat"], int(par["vlower"]), int(par["vupper"]))
    c.set_sizes(par["sizes"])
    yield c
    c.close()


def _packed(lens, frags=None):
    """PackedChunks of chunks with the given lengths; `frags`: per chunk (l, n) or None for one short fragment"""
    lp, il, off = [], [], [0]
    for k, Lc in enumerate(lens):
        l, n = frags[k] if frags is not None else (np.zeros(1, np.int64), np.full(1, min(Lc, 50), np.int64))
        lp.append(l)
        il.append(n)
        off.append(off[-1] + len(l))
    return PackedChunks(np.arange(len(lens)) * 100000, lens, off, np.concatenate(lp), np.concatenate(il), None, None)


def surviving_maxima(sig, min_signal=0.0, boundary=0, order=1):
    """number of maxima of utils.call_peaks before reduce_peaks (after the min_signal and boundary tests): what the device lists hold"""
    from scipy import signal
    x = np.array(sig, dtype=np.float64)
    nan = np.isnan(x)
    if nan.all():
        return 0
    x[nan] = np.min(x[~nan])
    n = len(x)
    pk = signal.argrelmax(x * (1 + np.random.RandomState(seed=25).uniform(0, 10 ** -12, n)), order=order)[0]
    pk = pk[x[pk] >= min_signal]
    return int(np.count_nonzero((pk >= boundary) & (pk < n - boundary)))


def designed_signals(maxL, seed):
    """chunks of a batch whose longest chunk has maxL bases: white noise, plateaus of exactly equal values, a constant with ulp-level
    variation (saturated occupancy), values below min_signal, maxima inside the boundary bands, and the short companions -- shorter
    than 2 * boundary, one base, all NaN, NaN runs at both ends"""
    rng = np.random.default_rng(seed)
    L0 = maxL
    L1 = max(1, maxL - 1)
    out = [rng.standard_normal(L0)]                                                     # white noise: dense maxima
    runs = rng.integers(1, 7, size=L1)                                                  # plateaus of exactly equal values
    out.append(np.repeat(rng.choice([0.25, 0.5, 1.0, 2.0], size=L1), runs)[:L1])
    out.append(1.0 + rng.integers(0, 3, size=L0) * np.finfo(np.float64).eps)            # saturated: 1 and 1 + 1 or 2 ulp
    low = rng.uniform(-1.0, 0.45, size=L0)                                              # below min_signal 0.5 but for a few
    low[rng.integers(0, L0, size=max(1, L0 // 50))] = rng.uniform(0.5, 0.6, size=max(1, L0 // 50))
    out.append(low)
    edge = 0.01 * rng.standard_normal(L1)                                               # maxima in and next to the boundary bands
    for p in (0, 1, 2, 30, 58, 59, 60, 61, 62, 119, 120, 121):
        for q in (p, L1 - 1 - p):
            if 0 <= q < L1:
                edge[q] = 1.0 + 0.001 * p
    out.append(edge)
    out.append(rng.standard_normal(min(maxL, 119)))                                     # shorter than 2 * boundary
    out.append(np.array([0.7]))                                                         # one base
    out.append(np.full(min(maxL, 300), np.nan))                                         # all NaN
    nan_ends = rng.standard_normal(L1)
    nan_ends[:min(L1, 37)] = np.nan
    nan_ends[max(0, L1 - 41):] = np.nan
    out.append(nan_ends)
    return out


def check_search(cc, cp, st, sigs, maxL, order, boundary, sep, min_signal, what):
    """device (cc, cp, status) == the host restatement for every chunk; the overflow flag exactly where the host predicts one"""
    arm = peak_arm(maxL, order)
    bounds = np.searchsorted(cc, np.arange(len(sigs) + 1))
    assert np.all(np.diff(cc) >= 0), what
    flagged = 0
    for k, s in enumerate(sigs):
        over = overflows(arm, maxL, order, surviving_maxima(s, min_signal, boundary, order))
        assert int(st[k]) & 2 == (2 if over else 0), (what, arm, k, len(s), int(st[k]))
        if over:
            flagged += 1
            continue
        want = np.asarray(call_peaks_stable(np.array(s, dtype=np.float64), min_signal=min_signal, sep=sep, boundary=boundary,
                                            order=order), np.int64)
        got = cp[int(bounds[k]):int(bounds[k + 1])]
        assert np.array_equal(got, want), (what, arm, k, len(s), got[:8], want[:8], len(got), len(want))
    return flagged


@pytest.mark.gpu
@pytest.mark.parametrize("maxL", LENGTHS)
def test_track_peaks_every_arm(ctx, maxL):
    """natac_run_track_peaks on designed signals (set_track) for every order / boundary / sep / min_signal of PARAMS: a fresh
    set of outputs per search (release_outputs)"""
    sigs = designed_signals(maxL, seed=maxL)
    lens = [len(s) for s in sigs]
    assert max(lens) == maxL
    b = ctx.upload(_packed(lens))
    flat = np.concatenate(sigs)
    try:
        for order, boundary, sep, min_signal in PARAMS:
            b.release_outputs()
            b.set_track(L.T_OCC, flat)
            cc, cp = b.run_track_peaks(L.T_OCC, min_signal=min_signal, sep=sep, boundary=boundary, order=order)
            check_search(cc, cp, b.status(), sigs, maxL, order, boundary, sep, min_signal,
                         ("track", maxL, order, boundary, sep, min_signal))
    finally:
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("maxL", NUC_LENGTHS)
def test_run_peaks_every_arm(ctx, maxL):
    """natac_run_peaks (norm + smoothed, with statistics) on natac_run_nuc output at the arms' lengths: positions == the host
    restatement, lr / var / z == natac_run_candidates at the same positions, bit for bit"""
    rng = np.random.default_rng(maxL + 7)
    lens = [maxL, max(130, maxL // 3), 130]
    frags = []
    for Lc in lens:
        n = rng.integers(30, 400, size=max(20, 3 * Lc // 10))
        c = np.sort(rng.integers(-150, Lc + 150, size=len(n)))
        frags.append((c - (n - 1) // 2, n))
    b = ctx.upload(_packed(lens, frags))
    try:
        sigs = None
        for order, boundary, sep, min_signal in NUC_PARAMS:
            b.release_outputs()
            b.run_nuc(10)
            if sigs is None:
                sigs = [x + y for x, y in zip(b.split(b.track(L.T_NORM)), b.split(b.track(L.T_SMOOTH)))]
            cc, cp, lr, var, z = b.run_peaks(min_signal=min_signal, sep=sep, boundary=boundary, order=order)
            check_search(cc, cp, b.status(), sigs, maxL, order, boundary, sep, min_signal, ("nuc", maxL, order, boundary, sep))
            assert len(cc) > 0
            lr2, var2, z2 = b.run_candidates(cc, cp)
            assert np.array_equal(lr, lr2, equal_nan=True) and np.array_equal(var, var2, equal_nan=True) and \
                np.array_equal(z, z2, equal_nan=True), ("stats", maxL, order)
    finally:
        b.free()


def _spikes(Lc, n, rng, ties=False):
    """n isolated maxima (every other base from base 2), zero elsewhere: exactly n surviving maxima at order 1, boundary 0"""
    x = np.zeros(Lc)
    h = np.ones(n) if ties else rng.uniform(0.5, 1.0, size=n)
    x[2:2 + 2 * n:2] = h
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("sep", [1, 4, 120])
def test_overflow_flag_at_the_boundary(ctx, sep):
    """a register kernel keeps PEAK_MAX = 2,048 maxima per chunk: 2,048 are not flagged and the result is exact; 2,049 set status
    value 2 for that chunk only (the other chunks of the batch stay exact); the same chunk in a batch whose longest chunk is over
    16,384 bases (segmented kernel, global lists) is not flagged and its whole result is exact"""
    rng = np.random.default_rng(sep)
    kw = dict(min_signal=0.0, sep=sep, boundary=0, order=1)
    sigs = [_spikes(5000, 2048, rng), _spikes(5000, 2049, rng), rng.standard_normal(4000), _spikes(5000, 2048, rng, ties=True),
            _spikes(4200, 2049, rng, ties=True), rng.standard_normal(300)]
    assert [surviving_maxima(s, **{k: kw[k] for k in ("min_signal", "boundary", "order")}) for s in sigs[:2]] == [2048, 2049]
    assert peak_arm(5000, 1) == Arm("reg", 1024, 5, "direct", False)
    b = ctx.upload(_packed([len(s) for s in sigs]))
    b.set_track(L.T_OCC, np.concatenate(sigs))
    cc, cp = b.run_track_peaks(L.T_OCC, **kw)
    st = b.status()
    assert list(st & 2) == [0, 2, 0, 0, 2, 0]
    assert check_search(cc, cp, st, sigs, 5000, **kw, what=("boundary", sep)) == 2
    b.free()
    seg = [sigs[1], sigs[4], rng.standard_normal(17000)]
    assert peak_arm(17000, 1) == Arm("seg", 256, None, None, True)
    b = ctx.upload(_packed([len(s) for s in seg]))
    b.set_track(L.T_OCC, np.concatenate(seg))
    cc, cp = b.run_track_peaks(L.T_OCC, **kw)
    st = b.status()
    assert not st.any()
    assert check_search(cc, cp, st, seg, 17000, **kw, what=("segmented", sep)) == 0
    if sep <= 2:                                  # maxima two bases apart: nothing to thin
        assert np.count_nonzero(cc == 0) == 2049
    b.free()


@pytest.mark.gpu
def test_overflow_flag_lifetime(ctx):
    """Pins the lifetime of the per-chunk status word (natac_batch_status): d_status is cleared when the batch is created and by
    natac_batch_release_outputs, and each stage drops its OWN bit for every chunk before it launches -- value 2 belongs to the peak
    search, value 1 to natac_run_occ.  So value 2 always describes the LAST search on the batch, whatever ran on it before (a search
    under another model included: natac.h, rule A), and a search never touches value 1.  The drivers read status() once, after all
    stages of a batch, and use value 2 only from a batch that ran a single peak search (occ: natac_run_occ_peaks; nuc:
    natac_run_peaks), so a set bit names the search whose result they replace."""
    rng = np.random.default_rng(5)
    sigs = [_spikes(5000, 2049, rng), rng.standard_normal(3000)]
    b = ctx.upload(_packed([len(s) for s in sigs]))
    assert not b.status().any()
    b.set_track(L.T_OCC, np.concatenate(sigs))
    b.run_track_peaks(L.T_OCC, min_signal=0.0, sep=1, boundary=0, order=1)
    assert list(b.status()) == [2, 0]
    # a search without overflow (order 3: at most 5000 / 4 + 1 maxima, lists sized for them) drops the flag of the one before it
    cc, cp = b.run_track_peaks(L.T_OCC, min_signal=0.0, sep=1, boundary=0, order=3)
    assert not b.status().any()
    assert np.array_equal(cp[cc == 0], call_peaks_stable(sigs[0].copy(), min_signal=0.0, sep=1, boundary=0, order=3))
    # ... and the overflowing search raises it again, for its chunk only
    b.run_track_peaks(L.T_OCC, min_signal=0.0, sep=1, boundary=0, order=1)
    assert list(b.status()) == [2, 0]
    b.release_outputs()
    assert not b.status().any()
    b.set_track(L.T_OCC, np.concatenate(sigs))
    b.run_track_peaks(L.T_OCC, min_signal=0.0, sep=1, boundary=0, order=3)
    assert not b.status().any()
    b.free()
