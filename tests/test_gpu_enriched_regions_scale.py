"""natac_enriched_regions (csrc/natac_peakcall.hpp) at the shape `pyatac peaks` runs at: several segments of the default size, whose
prefix scans (dev_scan, natac_runtime.hpp) take more than one trip of 1024 block sums; pieces above NATAC_PEAKS_SHORT_MAX in several
segments; records that only the two searches of a dense range keep in or out; more records in one range than one trip of the
histogram's grid; coordinates up to 2^31 - 1 and the widest window allowed.  The cases are built in tests/peaks_ref.py, and
tests/test_peaks_host.py checks without a GPU that each reaches the arm it is built for.  As in tests/test_gpu_enriched_regions.py every
comparison is equality with the NumPy restatement in all six arrays and the two counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import peaks_ref as R
from conftest import ROOT
from test_gpu_enriched_regions import CHILD, _ctx, assert_same, both

pytestmark = pytest.mark.gpu


def device(case, **kw):
    pos, tlen, n, geom, min_pile, ts, tl = case
    return _ctx().enriched_regions(pos, tlen, n, ts, tl, min_pile, *geom, with_counts=True, **kw)


def in_child(cases, segment, tmp_path):
    """the answers of a fresh process with NATAC_PEAKS_SEGMENT = segment"""
    arrs = dict(n_cases=len(cases))
    for k, (p, t, n, g, mp, ts, tl) in enumerate(cases):
        arrs.update({"pos_%d" % k: p, "tlen_%d" % k: t, "ts_%d" % k: ts, "tl_%d" % k: tl, "geom_%d" % k: np.asarray([n, mp] + list(g), np.int64)})
    path, out = str(tmp_path / "cases.npz"), str(tmp_path / "out.npz")
    np.savez(path, **arrs)
    subprocess.run([sys.executable, "-c", CHILD, path, out], check=True, env=dict(os.environ, NATAC_PEAKS_SEGMENT=str(segment)), cwd=ROOT,
                   timeout=120)
    d = np.load(out)
    return [[d["r_%d_%d" % (k, j)] if j < 6 else int(d["r_%d_%d" % (k, j)]) for j in range(8)] for k in range(len(cases))]


# ---- 1. three default segments: the scans' trip borders, the segment borders, the counted second sweep ---------------------------------
@pytest.mark.parametrize("max_gap,kind", R.BORDER_CASES)
def test_default_segments_and_scan_trip_borders(max_gap, kind):
    """9.5 M bases: the histogram's scan takes three trips and the verdicts' two in each full segment, and a run, a gap of max_gap or one of
    max_gap + 1 bases lies across each of those borders and across both segment borders (R.border_case).  More regions than
    NATAC_PEAKS_FIRST_CAPACITY, so the first sweep over the three segments overflows, is counted and run again from a reset state."""
    case, spots, want = R.border_case_with_answer(max_gap, kind)
    assert len(want[0]) > R.FIRST_CAPACITY and case[2] > 2 * R.SEGMENT
    assert_same(device(case), want)


# ---- 2. pieces around NATAC_PEAKS_SHORT_MAX ------------------------------------------------------------------------------------------------
def test_regions_of_exactly_the_short_limit():
    """regions of SHORT_MAX - 1, SHORT_MAX and SHORT_MAX + 1 bases whose highest pileup lies on the first base, the last, base 63, base 64,
    or on the first and the last as equals (the long pieces of several segments are cases 4..6 of test_segment_size_changes_nothing)"""
    case, regions = R.piece_limit_case()
    want = both(*case)
    assert list(zip(*(a.tolist() for a in want[:3]))) == regions


# ---- 3. the reach ----------------------------------------------------------------------------------------------------------------------------
def test_reach_of_mixed_tlen_at_the_default_segment():
    want = both(*R.reach_case())
    assert want[5].tolist().count(8) >= 2                # the two summits with a far record's insertion at exactly `large`


def test_reach_of_mixed_tlen_at_segment_1000(tmp_path):
    """tlen from -3000 to 5000: the records that can touch a dense range are what the two searches say, and the far records' insertions
    are the first and the last base of a segment's dense range"""
    case = R.reach_case()
    assert_same(in_child([case], R.REACH_SEGMENT, tmp_path)[0], R.regions_of(case))


# ---- 4. more records in one dense range than the histogram's grid has threads ------------------------------------------------------------
def test_more_records_than_one_trip_of_the_histogram_grid():
    case = R.grid_stride_case()
    assert len(case[0]) > R.GRID_RECORDS
    want = both(*case)
    assert np.sum(want[0] >= 99_000) == 1                # the region of the records behind index 2^24


# ---- 5. the far end and the widest window ---------------------------------------------------------------------------------------------------
def test_far_end_of_the_coordinates():
    """chrom_len = 2^31 - 1 at the default segment (512 segments): the restatement cannot run there, but with nothing before base `large`
    it commutes with a shift (test_far_end_case_moves_with_a_shift), so the device runs the chromosome moved against the far end and
    the restatement runs it where it is"""
    case = R.far_end_case()
    d = 2 ** 31 - 1 - case[2]
    want = R.shift_answer(R.regions_of(case), d)
    assert want[1][-1] == 2 ** 31 - 1 and len(want[0]) >= 3
    assert_same(device(R.shifted(case, d)), want)


@pytest.fixture(scope="module")
def wide_cases():
    cases = R.wide_window_cases()
    return cases, [R.regions_of(c) for c in cases]


def test_widest_window_at_the_default_segment(wide_cases):
    for case, want in zip(*wide_cases):
        assert len(want[0]) >= 1
        assert_same(device(case), want)


def test_widest_window_at_segment_1000(wide_cases, tmp_path):
    """large = NATAC_PEAKS_MAX_WINDOW, as half_width too in the last case (then the second sweep's halo is 50 segments wide), and tables of
    two entries"""
    cases, want = wide_cases
    for got, w in zip(in_child(cases, 1000, tmp_path), want):
        assert_same(got, w)
