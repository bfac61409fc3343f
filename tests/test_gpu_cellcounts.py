"""The cell-by-region count matrix on the GPU (natac_region_cell_counts, csrc/natac_cellcounts.hpp; `pyatac cellcounts`,
nucleoatac_amd/pyatac/get_cellcounts.py) against the NumPy restatement of tests/cellcounts_ref.py and against natac_region_counts, which is
pinned to the reference.  Exact integers throughout: equality, no tolerance.

The row-size ladder builds regions with exactly h counting records for every h at which a row changes arm (the bounds are read from
include/natac.h), each with all hits in one cell, all in distinct cells, and in h mod 5 cells (5 where h is a multiple of 5: a row of
hits cannot lie in no cell)."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import cellcounts_ref as R
from conftest import ROOT
from helpers import bgzf_bytes
from sites_ref import region_counts_brute

pytestmark = pytest.mark.gpu

_HDR = open(os.path.join(ROOT, "include", "natac.h")).read()
WAVE_MAX = int(re.search(r"#define NATAC_CELLCOUNT_WAVE_MAX (\d+)", _HDR).group(1))
SHORT_MAX = int(re.search(r"#define NATAC_CELLCOUNT_SHORT_MAX (\d+)", _HDR).group(1))
MAX_CELLS = int(re.search(r"#define NATAC_SPLIT_MAX_BARCODES (\d+)", _HDR).group(1))
LADDER = sorted({1, 2, 63, 64, 65, WAVE_MAX, WAVE_MAX + 1, SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1, 3 * SHORT_MAX + 7})


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(pos, tlen, cell, n_cells, s, e, lower=0, upper=500, atac=1, cap=0, col=None, val=None, nf=None, nr=None, ptr="own"):
    """natac_region_cell_counts called directly -> (return code, row_ptr)"""
    from nucleoatac_amd import _lib as L
    lib = L.load()
    row_ptr = np.full((len(s) if nr is None else max(nr, 0)) + 1, -7, np.int64) if isinstance(ptr, str) else ptr
    rc = lib.natac_region_cell_counts(_ctx()._h, len(pos) if nf is None else nf, _vp(pos), _vp(tlen), _vp(cell), n_cells, len(s) if nr is None else nr,
                                      _vp(s), _vp(e), lower, upper, atac, _vp(row_ptr), cap, _vp(col), _vp(val), None)
    return rc, row_ptr


def _i64(x):
    return np.ascontiguousarray(x, dtype=np.int64)


def test_constants_are_what_the_arms_need():
    assert WAVE_MAX == 64 and 1024 <= SHORT_MAX <= 8192 and SHORT_MAX & (SHORT_MAX - 1) == 0 and MAX_CELLS == 1 << 23


def test_empty_inputs_both_ways():
    pos, tlen, cell = _i64([10, 20]), _i64([100, 100]), np.zeros(2, np.int32)
    s, e = _i64([0, 5]), _i64([50, 60])
    ptr, col, val = _ctx().region_cell_counts(pos[:0], tlen[:0], cell[:0], 4, s, e)
    assert ptr.tolist() == [0, 0, 0] and ptr.dtype == np.int64 and col.shape == val.shape == (0,) and col.dtype == val.dtype == np.int32
    ptr, col, val, ms = _ctx().region_cell_counts(pos, tlen, cell, 4, s[:0], e[:0], with_kernel_ms=True)
    assert ptr.tolist() == [0] and len(col) == len(val) == 0 and ms == 0
    # records and regions, and no record counts
    ptr, col, val = _ctx().region_cell_counts(pos, tlen, cell, 4, _i64([1000, 2000]), _i64([1500, 2000]))
    assert ptr.tolist() == [0, 0, 0] and len(col) == 0


def _mixed(rng, n_cells):
    lower, upper = 40, 180
    pos = np.sort(rng.integers(-30, 5000, 2000)).astype(np.int64)
    tlen = rng.integers(0, 400, 2000).astype(np.int64)
    cell = rng.integers(0, n_cells, 2000).astype(np.int32)
    s = rng.integers(-60, 5000, 300).astype(np.int64)
    e = s + rng.choice([0, 0, 1, 7, 90, 400, 2500], 300)
    s[100:120], e[100:120] = s[:20], e[:20]              # repeated regions
    s[-1], e[-1] = -100, 6000                            # everything
    return pos, tlen, cell, s, e, lower, upper


@pytest.mark.parametrize("atac", [0, 1])
@pytest.mark.parametrize("n_cells", [37, 1])
def test_mixed_small_case(atac, n_cells):
    rng = np.random.default_rng(100 + atac)
    pos, tlen, cell, s, e, lower, upper = _mixed(rng, n_cells)
    trim, shift = (8, 4) if atac else (0, 0)
    tlen[:50] = np.tile([lower - 1, lower, upper - 1, upper, 0], 10) + trim          # ilen at and beside both bounds, and 0
    # record 1000: both ends in one window (counts once there); its ends in two windows (counts in each)
    tlen[1000] = 100 + trim
    l = int(pos[1000]) + shift
    s[:3], e[:3] = [l - 5, l - 5, l + 90], [l + 120, l + 5, l + 105]
    assert pos.min() < 0 and np.any(e == s) and np.any(np.diff(s) < 0)
    want = R.cell_counts_brute(pos, tlen, cell, s, e, lower, upper, atac)
    mine = [int(want[2][a:b][want[1][a:b] == cell[1000]].sum()) for a, b in zip(want[0][:3], want[0][1:4])]
    alone = region_counts_brute(pos[1000:1001], tlen[1000:1001], s[:3], e[:3], lower, upper, atac)
    assert alone.tolist() == [1, 1, 1] and min(mine) >= 1
    assert np.array_equal(R.row_sums(want[0], want[2]), region_counts_brute(pos, tlen, s, e, lower, upper, atac))
    R.assert_same_csr(R.cell_counts_ref(pos, tlen, cell, n_cells, s, e, lower, upper, atac), want)
    got = _ctx().region_cell_counts(pos, tlen, cell, n_cells, s, e, lower, upper, bool(atac))
    R.assert_same_csr(got, want)
    assert want[0][-1] > (500 if n_cells > 1 else 100) and np.diff(want[0]).max() == min(n_cells, 37)
    # ilen == 0 is included when lower <= 0
    R.assert_same_csr(_ctx().region_cell_counts(pos, tlen, cell, n_cells, s, e, 0, upper, bool(atac)),
                      R.cell_counts_brute(pos, tlen, cell, s, e, 0, upper, atac))


def _ladder_case(variant):
    """clusters of h records 10,000 bases and more apart, five records that fail the size filter inside each; one region per cluster"""
    rng = np.random.default_rng(7)
    n_cells = max(LADDER) + 11
    pos, tlen, cell, s, e, base = [], [], [], [], [], 1000
    for h in LADDER:
        p = base + np.arange(h) // 4                     # four records per position
        k = {"one": 1, "distinct": h, "mod5": h % 5 or 5}[variant]
        ids = rng.choice(n_cells, size=k, replace=False)
        pos += p.tolist() + (base + rng.integers(0, max(h // 4, 1) + 1, 5)).tolist()
        tlen += [108] * h + [508] * 5                    # ilen 100 counts, ilen 500 == upper does not
        cell += ids[rng.permutation(h) % k].tolist() + [int(ids[0])] * 5
        s.append(base + 4)
        e.append(base + 4 + (h - 1) // 4 + 1)
        base += 10_000 + h
    o = np.argsort(pos, kind="stable")
    return _i64(pos)[o], _i64(tlen)[o], np.array(cell, np.int32)[o], n_cells, _i64(s), _i64(e)


@pytest.mark.parametrize("variant", ["one", "distinct", "mod5"])
def test_row_size_ladder(variant):
    pos, tlen, cell, n_cells, s, e = _ladder_case(variant)
    want = R.cell_counts_brute(pos, tlen, cell, s, e, 0, 500, 1)
    assert R.row_sums(want[0], want[2]).tolist() == LADDER                           # exactly h hits per region
    assert np.diff(want[0]).tolist() == [{"one": 1, "distinct": h, "mod5": min(h, h % 5 or 5)}[variant] for h in LADDER]
    got = _ctx().region_cell_counts(pos, tlen, cell, n_cells, s, e)
    R.assert_same_csr(got, want)
    perm = np.random.default_rng(3).permutation(len(s))                              # rows in any order, regions repeated
    perm = np.concatenate([perm, perm[:4]])
    R.assert_same_csr(_ctx().region_cell_counts(pos, tlen, cell, n_cells, s[perm], e[perm]),
                      R.cell_counts_brute(pos, tlen, cell, s[perm], e[perm], 0, 500, 1))


def test_cell_index_range():
    n_cells = (1 << 22) + 3
    ids = np.array([0, 65535, 65536, n_cells - 1], np.int32)
    n_long = SHORT_MAX + 900
    rng = np.random.default_rng(9)
    pos = _i64(np.concatenate([1000 + np.arange(40) // 2, 50_000 + np.arange(n_long) // 8]))
    tlen = np.full(len(pos), 108, np.int64)
    cell = np.concatenate([ids[rng.integers(0, 4, 40)], ids[rng.integers(0, 4, n_long)]]).astype(np.int32)
    cell[:4], cell[40:44] = ids, ids
    s, e = _i64([1004, 50_004, 900]), _i64([1004 + 20, 50_004 + n_long, 60_000])
    want = R.cell_counts_brute(pos, tlen, cell, s, e, 0, 500, 1)
    assert R.row_sums(want[0], want[2]).tolist() == [40, n_long, 40 + n_long] and np.diff(want[0]).tolist() == [4, 4, 4]
    assert want[1].tolist() == ids.tolist() * 3
    R.assert_same_csr(_ctx().region_cell_counts(pos, tlen, cell, n_cells, s, e), want)
    # one cell only
    zero = np.zeros(len(pos), np.int32)
    ptr, col, val = _ctx().region_cell_counts(pos, tlen, zero, 1, s, e)
    assert ptr.tolist() == [0, 1, 2, 3] and col.tolist() == [0, 0, 0] and val.tolist() == [40, n_long, 40 + n_long]


def test_many_rows():
    rng = np.random.default_rng(21)
    pos = np.sort(rng.integers(0, 700_000, 50_000)).astype(np.int64)
    tlen = rng.integers(8, 400, 50_000).astype(np.int64)
    cell = rng.integers(0, 3000, 50_000).astype(np.int32)
    s = 10 * np.arange(70_000, dtype=np.int64)
    e = s + 10
    want = R.cell_counts_ref(pos, tlen, cell, 3000, s, e, 0, 500, 1)
    sample = rng.choice(70_000, 200, replace=False)
    R.assert_same_csr(R.cell_counts_ref(pos, tlen, cell, 3000, s[sample], e[sample], 0, 500, 1),
                      R.cell_counts_brute(pos, tlen, cell, s[sample], e[sample], 0, 500, 1))
    got = _ctx().region_cell_counts(pos, tlen, cell, 3000, s, e, with_kernel_ms=True)
    R.assert_same_csr(got[:3], want)
    assert got[3] > 0 and want[0][-1] > 90_000 and np.count_nonzero(np.diff(want[0]) == 0) > 1000


def test_capacity_and_argument_errors():
    rng = np.random.default_rng(4)
    pos, tlen, cell, s, e, lower, upper = _mixed(rng, 37)
    want = R.cell_counts_brute(pos, tlen, cell, s, e, lower, upper, 1)
    nnz = int(want[0][-1])
    rc, ptr = _raw(pos, tlen, cell, 37, s, e, lower, upper)                          # the sizing call
    assert rc == 0 and np.array_equal(ptr, want[0])
    col, val = np.full(nnz + 3, -5, np.int32), np.full(nnz + 3, -6, np.int32)
    rc, ptr = _raw(pos, tlen, cell, 37, s, e, lower, upper, cap=nnz, col=col, val=val)
    assert rc == 0 and np.array_equal(ptr, want[0]) and np.array_equal(col[:nnz], want[1]) and np.array_equal(val[:nnz], want[2])
    assert col[nnz:].tolist() == [-5] * 3 and val[nnz:].tolist() == [-6] * 3
    col[:], val[:] = -5, -6
    from nucleoatac_amd import _lib as L
    rc, ptr = _raw(pos, tlen, cell, 37, s, e, lower, upper, cap=nnz - 1, col=col, val=val)
    assert rc == -1 and "cap" in L.load().natac_last_error().decode() and np.all(col == -5) and np.all(val == -6)     # NATAC_E_ARG
    bad = cell.copy()
    for k, v in ((1234, 37), (7, -1)):
        bad[:] = cell
        bad[k] = v
        rc, _ = _raw(pos, tlen, bad, 37, s, e, lower, upper, cap=nnz, col=col, val=val)
        assert rc == -1 and "record %d" % k in L.load().natac_last_error().decode() and np.all(col == -5)
    for kw in (dict(n_cells=0), dict(n_cells=MAX_CELLS + 1), dict(upper=lower), dict(cap=-1), dict(cap=5), dict(nf=-1), dict(nr=-1),
               dict(cap=nnz, col=col), dict(ptr=None)):
        args = dict(n_cells=37, lower=lower, upper=upper)
        args.update(kw)
        rc, _ = _raw(pos, tlen, cell, args.pop("n_cells"), s, e, **args)
        assert rc == -1 and L.load().natac_last_error(), kw
    assert _raw(pos[::-1].copy(), tlen, cell, 37, s, e, lower, upper)[0] == -1       # pos must be sorted
    assert _raw(pos, tlen, cell, 37, e + 1, e, lower, upper)[0] == -1                # end < start
    with pytest.raises(ValueError):
        _ctx().region_cell_counts(pos, tlen, cell[:5], 37, s, e)


def test_cross_checks_against_region_counts():
    rng = np.random.default_rng(31)
    n = 60_000
    pos = np.sort(rng.integers(0, 200_000, n)).astype(np.int64)
    tlen = rng.integers(8, 600, n).astype(np.int64)
    cell = rng.integers(0, 50, n).astype(np.int32)
    s = rng.integers(-500, 200_000, 400).astype(np.int64)
    e = s + rng.choice([1, 30, 500, 5000, 60_000], 400)
    s[0], e[0] = 0, 200_000
    ptr, col, val = _ctx().region_cell_counts(pos, tlen, cell, 50, s, e, 30, 400)
    total = _ctx().region_counts(pos, tlen, s, e, 30, 400)
    assert np.array_equal(R.row_sums(ptr, val), total) and total.max() > SHORT_MAX and total.min() <= WAVE_MAX
    assert all(np.all(np.diff(col[a:b]) > 0) for a, b in zip(ptr[:-1], ptr[1:])) and val.min() >= 1
    rows = np.repeat(np.arange(len(s)), np.diff(ptr))
    for b in (0, 17, 49):
        column = np.bincount(rows[col == b], weights=val[col == b], minlength=len(s)).astype(np.int64)
        assert np.array_equal(column, _ctx().region_counts(pos[cell == b], tlen[cell == b], s, e, 30, 400)), b


# ---- pyatac cellcounts ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from nucleoatac_amd.pyatac.chunk import read_bed_columns
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    d = tmp_path_factory.mktemp("cellcounts_cli")
    text, barcodes = R.crafted_cells()
    frag, bed, table = str(d / "cells.tsv.gz"), str(d / "my.windows.bed"), str(d / "cells.txt")
    open(frag, "wb").write(bgzf_bytes(text, blk=900))
    open(bed, "wb").write(R.crafted_windows())
    open(table, "wb").write(b"barcode\tcluster\n" + b"".join(b"%s\tc%d\n" % (b, k % 3) for k, b in enumerate(barcodes)))
    store, bc_count, n_un = FragmentStore.cells_fragments_python(frag, barcodes)
    names, chrom, start, end, _ = read_bed_columns(bed)
    dense = np.zeros((len(start), len(barcodes)), np.int64)      # the restatement, window by window
    for i in range(len(start)):
        c = names[chrom[i]]
        if c in store.pos:
            ptr, col, val = R.cell_counts_brute(store.pos[c], store.tlen[c], store.cell[c], start[i:i + 1], end[i:i + 1], 0, 500, 1)
            dense[i, col] = val
    return dict(d=d, frag=frag, bed=bed, table=table, barcodes=barcodes, dense=dense, names=names, chrom=chrom, start=start, end=end,
                bc_count=bc_count, n_un=n_un)


def test_command_end_to_end(files, tmp_path, monkeypatch, capsys):
    import scipy.io
    import scipy.sparse
    from nucleoatac_amd.pyatac.cli import main
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.get_counts import count_regions
    dense, names, chrom, start, end = (files[k] for k in ("dense", "names", "chrom", "start", "end"))
    monkeypatch.chdir(tmp_path)
    argv = ["cellcounts", "--fragments", files["frag"], "--bed", files["bed"], "--cells", files["table"], "--header"]
    assert main(argv) == 0
    assert sorted(os.listdir(".")) == ["my.windows.cellcounts." + x for x in ("barcodes.tsv", "mtx.gz", "regions.bed", "txt")]
    got = scipy.io.mmread("my.windows.cellcounts.mtx.gz").toarray()
    assert got.shape == dense.shape and np.array_equal(got, dense) and dense.sum() > 1000
    text = gzip.open("my.windows.cellcounts.mtx.gz").read().decode().splitlines()
    trip = np.array([x.split() for x in text[2:]], np.int64)
    assert text[0] == "%%MatrixMarket matrix coordinate integer general" and text[1] == "%d %d %d" % (dense.shape + (np.count_nonzero(dense),))
    assert np.all(np.diff(trip[:, 0] * 100 + trip[:, 1]) > 0)                        # row, then column
    assert open("my.windows.cellcounts.barcodes.tsv", "rb").read() == b"".join(b + b"\n" for b in files["barcodes"])
    assert open("my.windows.cellcounts.regions.bed").read() == "".join("%s\t%d\t%d\n" % (names[c], a, b) for c, a, b in zip(chrom, start, end))
    assert len(start) == len(R.crafted_windows().splitlines()) - 1                   # the zero-length window is dropped
    summary = dict(x.split("\t") for x in open("my.windows.cellcounts.txt").read().splitlines())
    n_data = int(files["bc_count"].sum()) + files["n_un"]
    assert summary == dict(barcodes_listed="30", barcodes_seen="30", data_lines=str(n_data), unassigned_lines=str(files["n_un"]),
                           windows=str(len(start)), nnz=str(np.count_nonzero(dense)))
    # a window on a chromosome the file never mentions, and one on a chromosome without a listed line: empty rows
    nowhere = [i for i in range(len(start)) if names[chrom[i]] in ("chrNowhere", "chrOnlyUnassigned")]
    assert len(nowhere) == 2 and not dense[nowhere].any() and not got[nowhere].any()
    # the npz holds the same matrix
    assert main(argv + ["--format", "npz", "--out", "sub"]) == 0
    z = np.load("sub.cellcounts.npz")
    assert sorted(z.files) == sorted(["indptr", "indices", "data", "shape", "barcodes", "region_chrom", "region_start", "region_end"])
    m = scipy.sparse.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=tuple(z["shape"]))
    assert z["indptr"].dtype == np.int64 and z["indices"].dtype == z["data"].dtype == np.int32 and np.array_equal(m.toarray(), dense)
    assert z["barcodes"].tolist() == files["barcodes"] and z["region_chrom"].tolist() == [names[c] for c in chrom]
    assert np.array_equal(z["region_start"], start) and np.array_equal(z["region_end"], end) and os.path.exists("sub.cellcounts.txt")
    # three columns against `pyatac counts` over that cell's lines alone (windows on chromosomes of the file)
    known = np.array([names[c] != "chrNowhere" for c in chrom])
    sub_names = [c for c in names if c != "chrNowhere"]
    sub_chrom = np.array([sub_names.index(names[c]) for c in chrom[known]], np.int32)
    for b in (0, 13, 29):
        one = FragmentStore.from_fragments(files["frag"], barcodes=[files["barcodes"][b]])
        assert np.array_equal(count_regions(sub_names, sub_chrom, start[known], end[known], one), got[known, b]), b
    capsys.readouterr()


def test_command_writes_nothing_on_error(files, tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac.cli import main
    monkeypatch.chdir(tmp_path)
    three = str(tmp_path / "three.tsv")
    open(three, "wb").write(b"chr1\t5\t9\t" + files["barcodes"][0] + b"\nchr1\t5\t9\n")
    twice = str(tmp_path / "twice.txt")
    open(twice, "wb").write(b"AA\tx\nAA\ty\n")
    before = sorted(os.listdir("."))
    base = ["cellcounts", "--fragments", files["frag"], "--bed", files["bed"], "--cells", files["table"], "--header"]
    for argv, message in ((base + ["--lower", "500"], "--upper (500) must be larger than --lower (500)"),
                          (base[:2] + [three] + base[3:], "three.tsv: line 2: no barcode field"),
                          (base[:2] + [str(tmp_path / "missing.tsv.gz")] + base[3:], "missing.tsv.gz"),
                          (base[:6] + [twice], "twice.txt: line 2: barcode AA is in group y")):
        assert main(argv) == 1
        err = capsys.readouterr().err
        assert err.startswith("pyatac cellcounts: ") and message in err
        assert sorted(os.listdir(".")) == before
