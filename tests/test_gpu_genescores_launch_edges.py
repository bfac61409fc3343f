"""natac_gene_cell_scores (csrc/natac_genescores.hpp) where tests/test_gpu_genescores.py does not reach: the second trip of the
grid-stride loops.  gs_rows_table serves (row, tile) items with 8 workgroups a CU and puts its tile's zeros back as the words are read,
in the count pass and in the fill pass; gs_count_hits and gs_rows_wave serve rows with 4 x 16,384 waves, and a wave's second row
reuses its 2 x 64 key words.  Every array is compared for equality with the NumPy restatement of tests/genescores_ref.py; arm_rows is
asserted everywhere.

The table case is sized from the grid that natac_gene_cell_scores_plan reports for the device's own CU count: with tiles of 16 cells its
items exceed the grid by 500, and among the items a workgroup serves one after the other are full tiles followed by empty ones and the
reverse.  The wave case has more than 4 x 16,384 + 400 genes, and at least 100 waves take a first and a second row of 1 .. 64 hits each.
tests/test_genescores_host.py checks the sizing for 256 and 304 CUs without a GPU."""
import functools

import numpy as np
import pytest

import genescores_ref as R

pytestmark = pytest.mark.gpu

ENV = ("NATAC_GENESCORES_SHORT_MAX", "NATAC_GENESCORES_TILE")
WAVES = 4 * 16384       # of gs_count_hits and gs_rows_wave, once a call has that many rows


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _n_cu():
    return _ctx().device_info()["n_cu"]


def _force(monkeypatch, short_max=None, tile=None):
    for name, v in zip(ENV, (short_max, tile)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


@functools.lru_cache(maxsize=None)
def _case(n_frags, n_cells, n_genes):
    """a crafted chromosome and its restatement, formed once: (case, (indptr, indices, data, hits))"""
    case = R.make_case(seed=n_cells, n_frags=n_frags, n_cells=n_cells, n_genes=n_genes)
    want = R.gene_cell_scores(*R.case_args(case), with_hits=True)
    for a in list(case.values()) + list(want):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case, want


def _run(case):
    return _ctx().gene_cell_scores(*R.case_args(case), with_hits=True, with_arm_rows=True)


def _same(got, want):
    return all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))


def _arms(hits, short_max):
    return [int(np.count_nonzero((hits > 0) & (hits <= short_max))), int(np.count_nonzero(hits > short_max))]


# ---- the table arm's second trip, in the count pass and in the fill pass -----------------------------------------------------------------
def test_table_arm_second_trip(monkeypatch):
    from nucleoatac_amd.device import gene_cell_scores_plan as plan
    n_cu = _n_cu()
    _force(monkeypatch, short_max=1, tile=16)
    most = plan(1 << 20, 200, 1 << 20, n_cu=n_cu)
    assert (most["tile"], most["n_tiles"]) == (16, 13)
    n_genes = max(400, (most["grid"] + 500) // 13 + 60)                # nearly every gene of the case has more than one hit
    case, want = _case(6000, 200, n_genes)
    hits = want[3]
    rows = np.flatnonzero(hits > 1)
    p = plan(n_genes, 200, len(rows), n_cu=n_cu)
    assert (p["short_max"], p["tile"], p["n_tiles"], p["lds_bytes"], p["grid"]) == (1, 16, 13, 64, most["grid"])
    assert len(rows) * p["n_tiles"] > p["grid"] + 500
    # the items a workgroup serves one after the other: `it` and `it + grid`
    pairs = R.tile_pairs(want[0], want[1], rows, 16, 13)
    a, b = pairs[:len(pairs) - p["grid"]], pairs[p["grid"]:]
    assert ((a >= 8) & (b == 0)).sum() >= 40 and ((a == 0) & (b >= 8)).sum() >= 30 and ((a > 0) & (b > 0) & (a != b)).sum() >= 500 and pairs.max() == 16
    got = _run(case)
    assert _same(got[:4], want) and got[4].tolist() == _arms(hits, 1) == [int((hits == 1).sum()), len(rows)] and got[4][0] >= 1
    for tile in (64, None):                                            # 4 tiles and 1 tile of 256: the same bytes
        _force(monkeypatch, short_max=1, tile=tile)
        q = plan(n_genes, 200, len(rows), n_cu=n_cu)
        assert (q["tile"], q["n_tiles"]) == ((64, 4) if tile else (256, 1))
        other = _run(case)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, other)), tile


# ---- the wave kernels' second trip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short_max", [None, 1])
def test_wave_kernels_second_trip(short_max, monkeypatch):
    from nucleoatac_amd.device import gene_cell_scores_plan as plan
    case, want = _case(1500, 50, 66000)
    hits = want[3]
    assert len(hits) > WAVES + 400 and np.array_equal(hits, R.window_hits(case))
    a, b = hits[:len(hits) - WAVES], hits[WAVES:]                     # one wave's first and second row
    both = (a >= 1) & (a <= 64) & (b >= 1) & (b <= 64)
    assert both.sum() >= 100 and (both & (a != b)).sum() >= 50 and (b == 0).sum() >= 5 and (b > 64).sum() >= 5
    _force(monkeypatch, short_max=short_max)
    arms = _arms(hits, short_max or 64)
    p = plan(66000, 50, arms[1], n_cu=_n_cu())
    assert (p["short_max"], p["tile"], p["n_tiles"]) == (short_max or 64, 256, 1) and arms[0] >= 1000
    if short_max:                                                      # the table arm takes most rows, more than its grid; the waves stride over them
        assert arms[1] > p["grid"] + 500 and ((b == 1) & (a > 1)).sum() >= 3
    got = _run(case)
    assert _same(got[:4], want) and got[4].tolist() == arms
