"""`pyatac cellcounts`: the cell-by-window count matrix of a single-cell fragment file.  This command is this package's own, like `split`:
the reference has no such tool.

`pyatac counts` gives one number per BED window for a whole file; per-cell numbers used to need the text filtered once per cell.  Here the
fragment file is read ONCE with the cell of every record kept (FragmentStore.from_fragments_cells; the host decoder answers), the windows
are grouped by chromosome, and one natac_region_cell_counts call per chromosome that has windows uploads that chromosome's records once
and reduces the (window, cell) hits to a sparse matrix on the device (csrc/natac_cellcounts.hpp): rows of up to 64 hits are sorted in the
registers of one wave, rows of up to 4,096 in the LDS of one workgroup, longer rows are counted into a dense array of per-cell counters.
The per-chromosome matrices are put back into BED row order on the host.  All numbers are exact integers.

The counting rule is that of `pyatac counts` (get_counts.py) with the ATAC offsets, per window and cell: a record of the cell counts once
if lower <= ilen < upper and its left or its right end lies in the window.  Windows with end - start < 1 are dropped as `counts` drops
them, rows stay in BED order; overlapping, repeated and unsorted windows are counted independently.  A fragment file has no sequence
dictionary, so a window on a chromosome the file never mentions is an empty row, not an error.  The matrix columns are the barcodes of
the --cells table (the table `split --groups` takes; its group column is not used) in order of first appearance; lines of other barcodes
are unassigned and only counted in the summary.  Discovering the barcodes from the file is not part of the command: `pyatac cells`
(get_cells.py) does that and writes the table this command takes.

Measured on the MI355X box (tools/bench_cellcounts.py, one box, one run: 10 M fragments in 10,000 cells, 99 MB BGZF, 100,000
non-overlapping 500-base windows on 4 chromosomes, 3.13 M entries at 31 hits per row): the tagged read 0.56 s, the four device calls
0.099 s (upload, the host's operand checks and two round trips included; 7.4 ms between their first and last kernel), the MatrixMarket
text 0.31 s; the same matrix from the same arrays with np.searchsorted + scipy.sparse.coo_matrix(...).tocsr() on that box 0.69 s, and equal.
"""
import gzip
import os
import time

import numpy as np

from .chunk import read_bed_columns
from .get_counts import CountsError

TEXT_ROWS = 1 << 16      # matrix entries per % operation of mtx_text


def cell_counts(store, n_cells, names, chrom, start, end, lower=0, upper=500, timing=None):
    """CSR (indptr int64, indices int32, data int32) of the windows (columns of read_bed_columns), rows in their order, columns the
    cells of the tagged `store`: one natac_region_cell_counts call per chromosome that has windows and is in the store."""
    from .. import get_context
    t = timing if timing is not None else {}
    t.setdefault("device_s", 0.0)
    t.setdefault("kernel_ms", 0.0)
    n_rows = len(start)
    row_nnz = np.zeros(n_rows, np.int64)
    parts = []
    for k, c in enumerate(names):
        if c not in store.pos:
            continue                         # the file never mentions it: empty rows
        idx = np.flatnonzero(chrom == k)
        t0 = time.perf_counter()
        ptr, col, val, ms = get_context().region_cell_counts(store.pos[c], store.tlen[c], store.cell[c], n_cells, start[idx], end[idx],
                                                             lower, upper, True, with_kernel_ms=True)
        t["device_s"] += time.perf_counter() - t0
        t["kernel_ms"] += ms
        row_nnz[idx] = np.diff(ptr)
        parts.append((idx, ptr, col, val))
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(row_nnz, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), np.int32)
    data = np.empty(int(indptr[-1]), np.int32)
    for idx, ptr, col, val in parts:         # entry q of the chromosome's row j goes to indptr[idx[j]] + (q - ptr[j])
        dest = np.repeat(indptr[idx] - ptr[:-1], np.diff(ptr)) + np.arange(len(col), dtype=np.int64)
        indices[dest] = col
        data[dest] = val
    return indptr, indices, data


def mtx_text(indptr, indices, data, n_cols):
    """the MatrixMarket coordinate text of a CSR matrix as bytes: 1-based `row col val` lines in row-then-column order, TEXT_ROWS entries
    per % operation"""
    n_rows = len(indptr) - 1
    rows = np.repeat(np.arange(1, n_rows + 1, dtype=np.int64), np.diff(indptr))
    trip = np.stack([rows, np.asarray(indices, np.int64) + 1, np.asarray(data, np.int64)], axis=1)
    out = [("%%%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (n_rows, n_cols, len(rows))).encode("ascii")]
    for i in range(0, len(rows), TEXT_ROWS):
        block = trip[i:i + TEXT_ROWS]
        out.append((("%d %d %d\n" * len(block)) % tuple(block.ravel().tolist())).encode("ascii"))
    return b"".join(out)


def get_cellcounts(args, timing=None):
    """`pyatac cellcounts`: writes BASE.cellcounts.mtx.gz + .barcodes.tsv + .regions.bed (--format mtx) or BASE.cellcounts.npz, and
    BASE.cellcounts.txt; returns (indptr, indices, data).  Everything is computed before the first file is written."""
    from .cellgroups import CellGroupError, read_groups
    from .fragments import FragmentStore
    if args.out is None:
        args.out = ".".join(os.path.basename(args.bed).split(".")[0:-1])
    if args.upper <= args.lower:
        raise CountsError("--upper (%d) must be larger than --lower (%d)" % (args.upper, args.lower))
    t = timing if timing is not None else {}
    for path in (args.cells, args.bed):
        if not os.path.exists(path):
            raise CellGroupError("%s: no such file" % path)
    barcodes = read_groups(args.cells, header=args.header).barcodes
    t0 = time.perf_counter()
    names, chrom, start, end, _ = read_bed_columns(args.bed)
    t["bed_s"] = time.perf_counter() - t0
    if not os.path.exists(args.fragments):
        raise CellGroupError("%s: no such file" % args.fragments)
    t0 = time.perf_counter()
    store, bc_count, n_unassigned = FragmentStore.from_fragments_cells(args.fragments, barcodes)
    t["read_s"] = time.perf_counter() - t0
    indptr, indices, data = cell_counts(store, len(barcodes), names, chrom, start, end, args.lower, args.upper, timing=t)
    t0 = time.perf_counter()
    base = args.out + ".cellcounts"
    region_chrom = np.array(names, dtype=object)[chrom] if len(chrom) else np.zeros(0, dtype=object)
    summary = ("barcodes_listed\t%d\nbarcodes_seen\t%d\ndata_lines\t%d\nunassigned_lines\t%d\nwindows\t%d\nnnz\t%d\n"
               % (len(barcodes), int(np.count_nonzero(bc_count)), int(bc_count.sum()) + n_unassigned, n_unassigned, len(start), len(indices)))
    if args.format == "npz":
        t["text_s"] = 0.0
        np.savez_compressed(base + ".npz", indptr=indptr, indices=indices, data=data, shape=np.array([len(start), len(barcodes)], np.int64),
                            barcodes=np.array(barcodes, dtype="S"), region_chrom=region_chrom.astype("U"), region_start=start, region_end=end)
    else:
        text = mtx_text(indptr, indices, data, len(barcodes))
        bed = "".join(["%s\t%d\t%d\n" % r for r in zip(region_chrom.tolist(), start.tolist(), end.tolist())])
        t["text_s"] = time.perf_counter() - t0
        with gzip.open(base + ".mtx.gz", "wb") as f:
            f.write(text)
        with open(base + ".barcodes.tsv", "wb") as f:
            f.write(b"".join([b + b"\n" for b in barcodes]))
        with open(base + ".regions.bed", "w") as f:
            f.write(bed)
    with open(base + ".txt", "w") as f:
        f.write(summary)
    return indptr, indices, data
