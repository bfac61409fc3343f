"""GPU: the window staging of natac_candidates_paired (natac_cand.hpp): a wave requests the metadata of its four candidates in two
rounds and then all 4 x 6 exp(bias) entries a lane holds of the four windows before the first one is used.  Checked against
natac_candidates4 (NATAC_CAND_OLD=1, which stages every window in its own loop) and the oracle, at the bounds of helpers._assert_stats.

  candidate counts     1, 2, 3, 5, 8: the tail lanes of the last wave recompute candidate k0.
  four chunks a wave   the candidates are ordered so that every wave's four come from four chunks of four lengths (the batch's first and
                       last chunk among them): four different bias offsets and lengths in one staging round.
  models               EW = W + upper - 2 = 370 (the sixth entry of lanes 0..49 only), 376 (the cap: lanes 0..55) and 314 (<= 320: the
                       sixth round of loads holds no entry at all, its clamped loads are discarded).
  slice ends           natac_run_nuc refuses a batch whose bias flanks are shorter than w + (upper - 2) / 2 on the left and
                       w + (upper - 1) / 2 + 1 on the right, and natac_run_candidates refuses positions outside [0, chunk_len): no caller
                       can make a window hang over an end of its chunk's bias slice, so the kernel's zero rule for such entries cannot be
                       reached from here.  What can be reached is the window flush with the ends: a batch with exactly the smallest
                       flanks, a middle chunk shorter than the window, every position of it (position 0 reads the slice's entry 0, the
                       last position its entry nb - 2), and a NaN in the neighbouring chunks' slices directly next to it (the last entry of
                       the slice in front and the first of the one behind): a staging load one entry off would read it.  The middle
                       chunk's results must not change by a bit.
  no bias              a batch without a bias track (every entry is 1.0, no load is formed).
  esmall arm           1e-160 (below the 2^-500 bound, product with a neighbour still > 0), 0 and NaN at the first and at the last staged
                       entry of each of the wave's four windows in turn: all three statistics and lr's NaN pattern equal
                       natac_candidates4's; with 0 and NaN that candidate's lr is NaN.  The same values one entry outside the window on
                       both sides: the NaN pattern of the clean batch, and natac_candidates4's values.
"""
import functools
import os

import numpy as np
import pytest

from helpers import _assert_stats, _reference_stats
from nucleoatac_amd.packing import PackedChunks
from test_gpu_candidates_table import LENS, _case, _model
from test_gpu_vplot_arms import BL, BR, _batch

pytestmark = pytest.mark.gpu

MODELS = [
    pytest.param(105, 251, 60, id="EW370"),
    pytest.param(105, 251, 63, id="EW376-cap"),
    pytest.param(105, 251, 32, id="EW314-no-sixth-entry"),
]
COUNTS = (1, 2, 3, 5, 8)
ONES = (1.0, 1.0, 1.0)


def _ew(lo, up, w):
    return 2 * w + 1 + ((up - 2) >> 1) + ((up - 1) >> 1)


def _both_arms(b, cc, cp):
    """lr / var / z of the default arm (natac_candidates_paired for these models) and of natac_candidates4 on the same batch"""
    mine = b.run_candidates(cc, cp)
    os.environ["NATAC_CAND_OLD"] = "1"                          # read at every launch
    try:
        old = b.run_candidates(cc, cp)
    finally:
        os.environ.pop("NATAC_CAND_OLD", None)
    return mine, old


def _wave_mixed_order(cc):
    """a permutation of the candidates in which consecutive ones come from different chunks: chunk 0, 3, 1, 2, 0, 3, ..."""
    per = [list(np.flatnonzero(cc == k)) for k in (0, 3, 1, 2)]
    order = []
    while any(per):
        for p in per:
            if p:
                order.append(p.pop(0))
    return np.array(order)


@pytest.mark.parametrize("lo,up,w", MODELS)
def test_counts_and_four_chunks_a_wave(lo, up, w):
    from nucleoatac_amd.device import Context
    assert _ew(lo, up, w) <= 376 and (_ew(lo, up, w) <= 320) == (w == 32)
    pk, cc, cp, ref, scales = _case(lo, up, w)
    vm, sizes = _model(lo, up, w)
    order = _wave_mixed_order(cc)
    assert len(order) == len(cc) and sorted(set(cc[order[:4]])) == [0, 1, 2, 3] and sorted(set(cc[order[4:8]])) == [0, 1, 2, 3]
    assert len(set(LENS)) == 4
    with Context(0) as c:
        c.set_vmat(vm, lo, up)
        c.set_sizes(sizes)
        b = c.upload(pk)
        b.run_nuc(10)
        for n in COUNTS + (len(order),):
            sel = order[:n]
            mine, old = _both_arms(b, cc[sel], cp[sel])
            for name, a, o, r in zip(("lr", "var", "z"), mine, old, ref):
                print("n = %d %s: max |paired - candidates4| = %g, max |paired - oracle| = %g"
                      % (n, name, np.nanmax(np.abs(a - o)), np.nanmax(np.abs(a - r[sel]))))
            _assert_stats(mine, old, tuple(s[sel] for s in scales), "n = %d candidates4" % n)
            _assert_stats(mine, tuple(r[sel] for r in ref), tuple(s[sel] for s in scales), "n = %d oracle" % n)
        b.free()


@functools.lru_cache(maxsize=None)
def _nobias_case():
    from oracle import natac_oracle as O
    lo, up, w = 105, 251, 60
    vm, sizes = _model(lo, up, w)
    pk0, fr = _batch(LENS, up, seed=77)
    pk = PackedChunks(pk0.chunk_start, pk0.chunk_len, pk0.frag_off, pk0.frag_lpos, pk0.frag_ilen, None, None)
    rng = np.random.default_rng(78)
    cc = np.repeat(np.arange(len(LENS)), 3).astype(np.int32)
    cp = np.concatenate([[0, Lc - 1, rng.integers(1, Lc - 1)] for Lc in LENS]).astype(np.int32)
    nts = [O.nuc_chunk_tracks(fr[k][0], fr[k][1], 0, Lc, None, 0, vm, lo, up, sizes, smooth_sd=10) for k, Lc in enumerate(LENS)]
    ref, scales = _reference_stats(nts, vm, lo, up, cc, cp)
    return pk, cc, cp, ref, scales


def test_batch_without_bias():
    from nucleoatac_amd.device import Context
    lo, up, w = 105, 251, 60
    pk, cc, cp, ref, scales = _nobias_case()
    vm, sizes = _model(lo, up, w)
    with Context(0) as c:
        c.set_vmat(vm, lo, up)
        c.set_sizes(sizes)
        b = c.upload(pk)
        b.run_nuc(10)
        mine, old = _both_arms(b, cc, cp)
        b.free()
    for name, a, o, r in zip(("lr", "var", "z"), mine, old, ref):
        print("%s: max |paired - candidates4| = %g, max |paired - oracle| = %g" % (name, np.nanmax(np.abs(a - o)), np.nanmax(np.abs(a - r))))
    assert np.isfinite(ref[0]).all()
    _assert_stats(mine, old, scales, "candidates4")
    _assert_stats(mine, ref, scales, "oracle")


def test_window_flush_with_the_slice_ends():
    from nucleoatac_amd.device import Context
    lo, up, w = 105, 251, 60
    A, Bh = (up - 2) >> 1, (up - 1) >> 1
    bl, br = w + A, w + Bh + 1                                   # the smallest flanks natac_run_nuc takes
    lens = [150, 70, 97]                                         # the middle chunk is shorter than the window (370 entries)
    assert lens[1] < _ew(lo, up, w) < lens[1] + bl + br
    vm, sizes = _model(lo, up, w)
    pk0, _ = _batch(lens, up, seed=5)
    nb = [Lc + bl + br for Lc in lens]
    boff = np.concatenate(([0], np.cumsum(nb)))
    clean = np.random.default_rng(6).normal(0, 0.7, size=int(boff[-1]))
    poisoned = clean.copy()
    poisoned[boff[1] - 1] = np.nan                               # last entry of the slice in front of the middle chunk's
    poisoned[boff[2]] = np.nan                                   # first entry of the slice behind it
    cp = np.arange(lens[1], dtype=np.int32)                      # p = 0 reads entry 0 of the slice, p = L - 1 entry nb - 2
    cc = np.ones(len(cp), np.int32)
    got = {}
    with Context(0) as c:
        c.set_vmat(vm, lo, up)
        c.set_sizes(sizes)
        for name, bias in (("clean", clean), ("poisoned", poisoned)):
            pk = PackedChunks(pk0.chunk_start, pk0.chunk_len, pk0.frag_off, pk0.frag_lpos, pk0.frag_ilen, boff, bias, bias_left=bl, bias_right=br)
            b = c.upload(pk)
            b.run_nuc(10)
            got[name] = _both_arms(b, cc, cp)
            b.free()
    for name in got:
        mine, old = got[name]
        assert np.isfinite(mine[0]).all(), name
        _assert_stats(mine, old, ONES, "%s: candidates4" % name)
    for name, a, p in zip(("lr", "var", "z"), got["clean"][0], got["poisoned"][0]):
        assert np.array_equal(a, p), "%s of the middle chunk changes with a NaN in its neighbours' slices" % name


VALUES = [pytest.param(np.log(1e-160), id="1e-160"), pytest.param(-np.inf, id="zero"), pytest.param(np.nan, id="nan")]


@pytest.mark.parametrize("lo,up,w", MODELS)
@pytest.mark.parametrize("logv", VALUES)
def test_small_zero_nan_at_the_window_ends(lo, up, w, logv):
    from nucleoatac_amd.device import Context
    A, Bh = (up - 2) >> 1, (up - 1) >> 1
    pk0 = _case(lo, up, w)[0]
    vm, sizes = _model(lo, up, w)
    # one wave: candidate q in chunk q, its window well inside the chunk's bias slice
    cc = np.arange(4, dtype=np.int32)
    cp = np.array([200, 17, 633, 350], np.int32)
    assert all(0 <= p < Lc for p, Lc in zip(cp, LENS)) and BL >= w + A + 1 and BR >= w + Bh + 2
    first = [int(pk0.bias_off[q]) + BL + int(cp[q]) - w - A for q in range(4)]      # index of window q's entry u = 0 in bias_log
    last = [f + _ew(lo, up, w) - 1 for f in first]                                  # ... of its entry u = EW - 1

    def run(c, damage):
        bias = pk0.bias_log.copy()
        bias[list(damage)] = logv
        pk = PackedChunks(pk0.chunk_start, pk0.chunk_len, pk0.frag_off, pk0.frag_lpos, pk0.frag_ilen, pk0.bias_off, bias, bias_left=BL, bias_right=BR)
        b = c.upload(pk)
        b.run_nuc(10)
        res = _both_arms(b, cc, cp)
        b.free()
        return res

    with Context(0) as c:
        c.set_vmat(vm, lo, up)
        c.set_sizes(sizes)
        clean, clean_old = run(c, ())
        assert np.isfinite(clean[0]).all()
        _assert_stats(clean, clean_old, ONES, "clean: candidates4")
        for q in range(4):
            for where, idx in (("first", (first[q],)), ("last", (last[q],)), ("outside", (first[q] - 1, last[q] + 1))):
                mine, old = run(c, idx)
                what = "window %d, %s entry" % (q, where)
                print(what, "lr paired", mine[0], "candidates4", old[0])
                _assert_stats(mine, old, ONES, what + ": candidates4")
                others = np.arange(4) != q
                assert np.isfinite(mine[0][others]).all(), what
                if where == "outside":
                    for a, cl in zip(mine, clean):
                        assert np.array_equal(np.isnan(a), np.isnan(cl)), what
                elif np.isfinite(logv):
                    assert np.isfinite(mine[0][q]), what          # 1e-160 times a neighbour is no zero
                else:
                    assert np.isnan(mine[0][q]), what             # the entry is a factor of the window's widest insert size
