"""The operand checks the three calls over a sorted fragment table share (check_fragments, check_intervals, check_site_centres in
csrc/natac_sites.hpp; natac_region_counts, natac_region_cell_counts and natac_cell_site_qc call them), through raw ctypes calls at
the smallest shape that has every operand: 8 records, 3 cells, 2 regions, 2 sites, 2 peaks.  Every violation is applied to every entry
point that takes the operand: NATAC_E_ARG, the exact message, every output array as it was.  One case with two violations per entry
point pins the order of the checks, and one clean call per entry point against a brute-force count runs the checks' accepting side."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIM = 1 << 60
N_CELLS, LOWER, UPPER, FLANK, CENTER, EDGE, CAP = 3, 30, 180, 50, 10, 5, 8
SENTINEL = -7


def base():
    """the clean operands (a fresh copy): with the ATAC offsets the insert sizes are 50, 100, 32, 200, 60, -38, 150, 80"""
    return dict(pos=np.array([100, 120, 120, 150, 200, 260, 300, 420], np.int64), tlen=np.array([58, 108, 40, 208, 68, -30, 158, 88], np.int64),
                cell=np.array([0, 2, 1, 0, 2, 1, 1, 0], np.int32), start=np.array([90, 280], np.int64), end=np.array([210, 460], np.int64),
                centre=np.array([130, 310], np.int64), minus=np.array([0, 1], np.uint8), pstart=np.array([95, 290], np.int64),
                pend=np.array([160, 450], np.int64))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _lib_ctx():
    from nucleoatac_amd import _lib as L, get_context
    return L.load(), get_context()._h


def _outs(*sizes, dtypes=None):
    """sentinel-filled output arrays, two guard elements behind each"""
    return [np.full(n + 2, SENTINEL, t) for n, t in zip(sizes, dtypes or [np.int64] * len(sizes))]


def region_counts(d):
    lib, h = _lib_ctx()
    out, ms = _outs(2), C.c_double(SENTINEL)
    rc = lib.natac_region_counts(h, 8, _vp(d["pos"]), _vp(d["tlen"]), 2, _vp(d["start"]), _vp(d["end"]), LOWER, UPPER, 1, _vp(out[0]), C.byref(ms))
    return rc, lib.natac_last_error().decode(), out, ms.value


def region_cell_counts(d):
    lib, h = _lib_ctx()
    out, ms = _outs(3, CAP, CAP, dtypes=(np.int64, np.int32, np.int32)), C.c_double(SENTINEL)      # row_ptr, col, val
    rc = lib.natac_region_cell_counts(h, 8, _vp(d["pos"]), _vp(d["tlen"]), _vp(d["cell"]), N_CELLS, 2, _vp(d["start"]), _vp(d["end"]), LOWER, UPPER,
                                      1, _vp(out[0]), CAP, _vp(out[1]), _vp(out[2]), C.byref(ms))
    return rc, lib.natac_last_error().decode(), out, ms.value


def cell_site_qc(d):
    lib, h = _lib_ctx()
    out, ms = _outs(N_CELLS, N_CELLS, N_CELLS, 2 * FLANK + 1), C.c_double(SENTINEL)
    rc = lib.natac_cell_site_qc(h, 8, _vp(d["pos"]), _vp(d["tlen"]), _vp(d["cell"]), N_CELLS, 2, _vp(d["centre"]), _vp(d["minus"]), FLANK, CENTER,
                                EDGE, 2, _vp(d["pstart"]), _vp(d["pend"]), _vp(out[0]), _vp(out[1]), _vp(out[2]), _vp(out[3]), C.byref(ms))
    return rc, lib.natac_last_error().decode(), out, ms.value


# where a refused call leaves kernel_ms: the two region calls zero it ahead of their checks, natac_cell_site_qc behind them (natac.h)
ENTRY = {"region_counts": (region_counts, 0.0), "region_cell_counts": (region_cell_counts, 0.0), "cell_site_qc": (cell_site_qc, float(SENTINEL))}
FRAGMENTS, CELLS, REGIONS, QC = tuple(ENTRY), ("region_cell_counts", "cell_site_qc"), ("region_counts", "region_cell_counts"), ("cell_site_qc",)

# (the entry points that take the operand, [(operand, index, value)], the message)
VIOLATIONS = [
    (FRAGMENTS, [("pos", 3, LIM + 1)], "record 3: pos or tlen out of range"),
    (FRAGMENTS, [("pos", 0, -LIM - 1)], "record 0: pos or tlen out of range"),
    (FRAGMENTS, [("tlen", 5, -LIM - 1)], "record 5: pos or tlen out of range"),
    (FRAGMENTS, [("tlen", 7, LIM + 1)], "record 7: pos or tlen out of range"),
    (FRAGMENTS, [("pos", 4, 149)], "pos must be non-decreasing (record 4)"),
    (CELLS, [("cell", 6, 3)], "record 6: cell 3 outside [0, 3)"),
    (CELLS, [("cell", 0, -1)], "record 0: cell -1 outside [0, 3)"),
    (REGIONS, [("end", 1, 279)], "region 1: end 279 < start 280"),
    (REGIONS, [("start", 0, -LIM - 1)], "region 0: coordinates out of range"),
    (REGIONS, [("end", 1, LIM + 1)], "region 1: coordinates out of range"),
    (QC, [("pend", 1, 289)], "peak 1: end 289 < start 290"),
    (QC, [("pstart", 0, -LIM - 1)], "peak 0: coordinates out of range"),
    (QC, [("pend", 1, LIM + 1)], "peak 1: coordinates out of range"),
    (QC, [("pstart", 1, 159)], "peaks must be disjoint and ascending (peak 1 starts at 159, before the end 160 of the one before)"),
    (QC, [("centre", 1, LIM + 1)], "site 1: centre out of range"),
    (QC, [("centre", 0, -LIM - 1)], "site 0: centre out of range"),
    (QC, [("centre", 1, 129)], "site centres must be ascending (site 1)"),
    # two violations: the order of the checks.  Regions before records in the region calls; records, then sites, then peaks in cellqc;
    # per record its range, then its order, then its cell -- and an earlier record before a later one
    (REGIONS, [("end", 1, 279), ("pos", 4, 149)], "region 1: end 279 < start 280"),
    (REGIONS, [("pos", 0, -LIM - 1), ("start", 0, -LIM - 1)], "region 0: coordinates out of range"),
    (QC, [("centre", 1, 129), ("pos", 4, 149)], "pos must be non-decreasing (record 4)"),
    (QC, [("pstart", 1, 159), ("centre", 1, 129)], "site centres must be ascending (site 1)"),
    (FRAGMENTS, [("pos", 4, 149), ("tlen", 4, LIM + 1)], "record 4: pos or tlen out of range"),
    (CELLS, [("pos", 4, 149), ("cell", 4, 3)], "pos must be non-decreasing (record 4)"),
    (CELLS, [("cell", 3, 3), ("pos", 4, 149)], "record 3: cell 3 outside [0, 3)"),
]


@pytest.mark.parametrize("entry,edits,message", [(e, ed, m) for es, ed, m in VIOLATIONS for e in es])
def test_a_violation_is_refused_with_its_message_and_the_outputs_stay(entry, edits, message):
    d = base()
    for name, i, v in edits:
        d[name][i] = v
    call, ms_after = ENTRY[entry]
    rc, msg, out, ms = call(d)
    assert rc == -1 and msg == message                                  # NATAC_E_ARG
    assert all(np.all(o == SENTINEL) for o in out) and ms == ms_after


def _hits():
    """[region] -> the records that count for it (natac.h: the ATAC offsets, the size filter, either end inside)"""
    d = base()
    l, ilen = d["pos"] + 4, d["tlen"] - 8
    r = l + ilen - 1
    return d, [[i for i in range(8) if LOWER <= ilen[i] < UPPER and (s <= l[i] < e or s <= r[i] < e)] for s, e in zip(d["start"], d["end"])]


def _untouched_guards(out):
    return all(np.all(o[-2:] == SENTINEL) for o in out)


def test_region_counts_clean_call():
    d, hits = _hits()
    assert [len(h) for h in hits] == [4, 2]                              # both regions count, the filter drops records 3 and 5
    rc, _, out, ms = region_counts(d)
    assert rc == 0 and out[0][:2].tolist() == [len(h) for h in hits] and _untouched_guards(out) and ms > 0


def test_region_cell_counts_clean_call():
    d, hits = _hits()
    row_ptr, col, val = [0], [], []
    for h in hits:
        n = np.bincount(d["cell"][h], minlength=N_CELLS)
        col += [c for c in range(N_CELLS) if n[c]]
        val += [int(n[c]) for c in range(N_CELLS) if n[c]]
        row_ptr.append(len(col))
    assert row_ptr == [0, 3, 5] and val == [1, 1, 2, 1, 1]
    rc, _, out, ms = region_cell_counts(d)
    assert rc == 0 and out[0][:3].tolist() == row_ptr and out[1][:5].tolist() == col and out[2][:5].tolist() == val and ms > 0
    assert np.all(out[1][5:] == SENTINEL) and np.all(out[2][5:] == SENTINEL) and _untouched_guards(out)


def test_cell_site_qc_clean_call():
    d = base()
    l = d["pos"] + 4
    r = l + (d["tlen"] - 8) - 1
    want = [np.zeros(N_CELLS, np.int64) for _ in range(3)] + [np.zeros(2 * FLANK + 1, np.int64)]
    for i in range(8):
        for x in (l[i], r[i]):
            for c, m in zip(d["centre"], d["minus"]):
                dist = c - x if m else x - c
                if abs(dist) <= FLANK:
                    want[3][dist + FLANK] += 1
                    want[0][d["cell"][i]] += abs(dist) <= CENTER
                    want[1][d["cell"][i]] += abs(dist) > FLANK - EDGE
        want[2][d["cell"][i]] += any(s <= x < e for x in (l[i], r[i]) for s, e in zip(d["pstart"], d["pend"]))
    assert want[3].sum() >= 4 and want[0].sum() >= 1 and want[1].sum() >= 1 and 0 < want[2].sum() < 8      # every class is hit
    rc, _, out, ms = cell_site_qc(d)
    assert rc == 0 and all(np.array_equal(o[:-2], w) for o, w in zip(out, want)) and _untouched_guards(out) and ms > 0
