"""GPU: natac_candidates_paired on its template stream (natac_cand_table, natac_cand.hpp) against natac_candidates4 (NATAC_CAND_OLD=1,
which reads the plain template) and the oracle, on small ragged batches.

The stream holds, per row pair and lane, the template values of columns `lane` and `lane + 64` of the pair's two rows; lanes without a
second column (lane + 64 >= W) hold +0.0 there, two zero pairs follow the last one, and the sweep walks it four pairs a trip, then two,
then one.

  second-column arms   W = 121: lanes 57..63 idle;  W = 65: lane 0 alone has a second column;  W = 127: lane 63 alone is idle.
                       (The API takes templates of 2 w + 1 columns, so 127 is the widest one the per-wave kernels see; no W = 128 exists.)
  loop tails, parity   R = 2, 4, 6, 10, 146 rows = 1, 2, 3, 5, 73 pairs: every exit of the four-pair loop, the two-pair loop and the
                       single-pair tail; odd and even `lower` (both instantiations); 43 candidates, not a multiple of 4 a wave.
  non-finite bias      +inf / NaN at one base.  An idle second column reads the window at the clamped column W - 1, the address lane
                       W - 65 reads for its live second column, so no window entry is read by idle lanes alone; the cases are the last
                       entry of a window (column W - 1 only: the idle lanes' address) and the first (column 0, a live first column),
                       with candidates on both sides of the border of the span that sees the base.  NaN patterns and infinities must
                       match natac_candidates4 entry for entry.
  model change         set_vmat / set_sizes on a live context, to fewer rows and back to other values of the first geometry: every
                       run equals a fresh context's bit for bit (the stream is keyed on the model generation).
"""
import functools
import os

import numpy as np
import pytest

from helpers import _assert_stats, _reference_stats
from nucleoatac_amd.packing import PackedChunks
from nucleoatac_amd.synth import synth_size_distribution
from test_gpu_vplot_arms import BL, BR, _batch, _vmat

pytestmark = pytest.mark.gpu

LENS = [403, 517, 640, 699]
NCAND = 43

GEOMETRIES = [
    pytest.param(105, 251, 60, id="W121-R146-odd"),
    pytest.param(105, 251, 32, id="W65-R146-odd"),
    pytest.param(105, 251, 63, id="W127-R146-odd"),
    pytest.param(104, 250, 60, id="W121-R146-even"),
    pytest.param(105, 107, 60, id="W121-R2-odd"),
    pytest.param(106, 110, 60, id="W121-R4-even"),
    pytest.param(105, 111, 60, id="W121-R6-odd"),
    pytest.param(106, 116, 60, id="W121-R10-even"),
]


def _model(lo, up, w):
    return _vmat(lo, up, w, False), synth_size_distribution(max(up, 251))[:up]


def _candidates(lens, seed):
    rng = np.random.default_rng(seed)
    cc, cp = [], []
    for k, Lc in enumerate(lens):
        n = NCAND // len(lens) + (1 if k < NCAND % len(lens) else 0)
        pos = np.sort(np.concatenate(([0, Lc - 1], rng.choice(np.arange(1, Lc - 1), size=n - 2, replace=False))))
        cc += [k] * len(pos)
        cp += list(pos)
    return np.array(cc, np.int32), np.array(cp, np.int32)


@functools.lru_cache(maxsize=None)
def _case(lo, up, w):
    """batch, candidates and the oracle's lr / var / z with their scales (computed once, read-only)"""
    from oracle import natac_oracle as O
    vm, sizes = _model(lo, up, w)
    pk, fr = _batch(LENS, up, seed=lo * 7 + up + w)
    cc, cp = _candidates(LENS, seed=lo + up + w)
    nts = [O.nuc_chunk_tracks(fr[k][0], fr[k][1], 0, Lc, pk.chunk_bias(k), -BL, vm, lo, up, sizes, smooth_sd=10)
           for k, Lc in enumerate(LENS)]
    ref, scales = _reference_stats(nts, vm, lo, up, cc, cp)
    for a in ref + scales:
        a.setflags(write=False)
    return pk, cc, cp, ref, scales


def _run(pk, vm, lo, up, sizes, cc, cp, old):
    """lr / var / z of the default arm (the paired kernel for these geometries) and, with `old`, of natac_candidates4 on the same batch"""
    from nucleoatac_amd.device import Context
    with Context(0) as c:
        c.set_vmat(vm, lo, up)
        c.set_sizes(sizes)
        b = c.upload(pk)
        b.run_nuc(10)
        mine = b.run_candidates(cc, cp)
        other = None
        if old:
            os.environ["NATAC_CAND_OLD"] = "1"                  # read at every launch
            try:
                other = b.run_candidates(cc, cp)
            finally:
                os.environ.pop("NATAC_CAND_OLD", None)
        b.free()
    return mine, other


@pytest.mark.parametrize("lo,up,w", GEOMETRIES)
def test_paired_equals_candidates4_and_oracle(lo, up, w):
    W, R = 2 * w + 1, up - lo
    assert lo >= 2 and R % 2 == 0 and 64 <= W <= 128 and W + ((up - 2) >> 1) + ((up - 1) >> 1) <= 376     # the paired kernel's domain
    pk, cc, cp, ref, scales = _case(lo, up, w)
    assert len(cc) == NCAND and NCAND % 4 != 0
    vm, sizes = _model(lo, up, w)
    mine, old = _run(pk, vm, lo, up, sizes, cc, cp, old=True)
    for name, a, o, r in zip(("lr", "var", "z"), mine, old, ref):
        print("%s: max |paired - candidates4| = %g, max |paired - oracle| = %g" % (name, np.nanmax(np.abs(a - o)), np.nanmax(np.abs(a - r))))
    assert not np.isnan(ref[0]).any() and np.isfinite(ref[1]).all()
    _assert_stats(mine, old, scales, "candidates4")
    _assert_stats(mine, ref, scales, "oracle")


NONFINITE = [pytest.param(v, where, id="%s-%s" % (n, where)) for n, v in (("inf", np.inf), ("nan", np.nan)) for where in ("last-entry", "first-entry")]


@pytest.mark.parametrize("value,where", NONFINITE)
def test_nonfinite_bias_next_to_idle_lanes(value, where):
    lo, up, w = 105, 251, 60
    A, Bh = (up - 2) >> 1, (up - 1) >> 1
    pk0 = _case(lo, up, w)[0]
    vm, sizes = _model(lo, up, w)
    k, a = 2, 300                                                # chunk 2 (640 bases), base 300
    bias = pk0.bias_log.copy()
    bias[int(pk0.bias_off[k]) + BL + a] = value
    pk = PackedChunks(pk0.chunk_start, pk0.chunk_len, pk0.frag_off, pk0.frag_lpos, pk0.frag_ilen, pk0.bias_off, bias, bias_left=BL, bias_right=BR)
    # a window at p spans p - w - A .. p + w + Bh.  Base `a` is its last entry (column W - 1 and the largest insert size only) at
    # p = a - w - Bh and its first entry (column 0) at p = a + w + A; three candidates beyond each border do not see it at all.
    edge = a - w - Bh if where == "last-entry" else a + w + A
    cp = np.arange(edge - 3, edge + 4, dtype=np.int32)
    cp = np.concatenate((cp, [a - 1, a, a + 1], [5, 600])).astype(np.int32)     # + the middle of the span and two far away: 12 candidates
    assert cp.min() >= 0 and cp.max() < LENS[k]
    cc = np.full(len(cp), k, np.int32)
    mine, old = _run(pk, vm, lo, up, sizes, cc, cp, old=True)
    for name, g, o in zip(("lr", "var", "z"), mine, old):
        print(name, "paired", g, "candidates4", o)
    sees = (cp >= a - w - Bh) & (cp <= a + w + A)
    assert np.isnan(mine[0][sees]).all()
    if np.isnan(value):                                          # the span is exact: one entry off and lr is finite (tests/test_gpu_damaged_bias.py)
        assert np.isfinite(mine[0][~sees]).all()
    ones = np.ones(len(cp))
    _assert_stats(mine, old, (ones, ones, ones), "candidates4")


def test_model_change_on_a_live_context():
    from nucleoatac_amd.device import Context
    rng = np.random.default_rng(11)
    models = []
    for lo, up, w, scale in ((105, 251, 60, False), (106, 116, 60, False), (105, 251, 60, True)):
        vm, sizes = _model(lo, up, w)
        if scale:                                                 # other values under the first geometry: same table size, new contents
            vm = vm * rng.uniform(0.5, 1.5, size=vm.shape)
            sizes = sizes * rng.uniform(0.5, 1.5, size=sizes.shape)
        models.append((vm, lo, up, sizes))
    pk, cc, cp, _, _ = _case(105, 251, 60)
    live = []
    with Context(0) as c:
        b = c.upload(pk)
        for vm, lo, up, sizes in models:
            c.set_vmat(vm, lo, up)
            c.set_sizes(sizes)
            b.run_nuc(10)
            live.append(b.run_candidates(cc, cp))
        b.free()
    for (vm, lo, up, sizes), got in zip(models, live):
        fresh, _ = _run(pk, vm, lo, up, sizes, cc, cp, old=False)
        for name, g, f in zip(("lr", "var", "z"), got, fresh):
            assert np.array_equal(g, f, equal_nan=True), "%s after a model change differs from a fresh context (lower=%d upper=%d)" % (name, lo, up)
    assert not np.array_equal(live[0][1], live[2][1])          # the third model is not the first
