"""Wall time by phase of `pyatac cellcounts` (nucleoatac_amd/pyatac/get_cellcounts.py) on a synthetic single-cell workload, kernel
milliseconds against wall time, and the same matrix built on the CPU with np.searchsorted + scipy.sparse.coo_matrix(...).tocsr() on the
same box as the point of comparison.  Prints one JSON line.

The workload: --records fragments of 30 to 600 bases, uniform over --refs chromosomes of --windows x 2,000 / --refs bases, each in one of
--cells cells (uniform), written as a BGZF fragment file with every cell listed; --windows windows of 500 bases, one in each 2,000-base
slot at a random offset (a peak set: they do not overlap), in random BED order.  About records x 1,000 / (windows x 2,000) hits per row.

  gen_s      making the file (not part of any figure)
  read_s     FragmentStore.from_fragments_cells: the host decoder with the cell of every record kept, and the store's sort
  device_s   the natac_region_cell_counts calls, one per chromosome: upload, kernels, two host round trips, download
  kernel_ms  first to last kernel of those calls on the stream (device events; the round trips in between are inside)
  merge_s    device_s plus putting the per-chromosome matrices into BED row order (get_cellcounts.cell_counts)
  text_s     the MatrixMarket text (mtx_text; no gzip)
  scipy_s    the CPU formulation on the store's arrays: two searchsorted per chromosome, one coo_matrix(...).tocsr() (no read, no text)
  equal      the two matrices are the same
usage: python tools/bench_cellcounts.py [--records 10000000] [--cells 10000] [--windows 100000] [--refs 4] [--out DIR] [--no-scipy]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOT, WIDTH = 2000, 500


def scipy_matrix(store, n_cells, names, chrom, start, end, lower, upper):
    """the windows of one chromosome do not overlap: an end lies in the last window that starts at or before it, or in none"""
    import scipy.sparse
    rows, cols = [], []
    for k, c in enumerate(names):
        idx = np.flatnonzero(chrom == k)
        o = np.argsort(start[idx], kind="stable")
        s, e, idx = start[idx][o], end[idx][o], idx[o]
        ilen = store.tlen[c] - 8
        ok = (ilen >= lower) & (ilen < upper)
        l = store.pos[c][ok] + 4
        r = l + ilen[ok] - 1
        cell = store.cell[c][ok]
        jl = np.searchsorted(s, l, "right") - 1
        jr = np.searchsorted(s, r, "right") - 1
        in_l = (jl >= 0) & (l < e[np.maximum(jl, 0)])
        in_r = (jr >= 0) & (r < e[np.maximum(jr, 0)]) & ~(in_l & (jl == jr))          # both ends in one window count once
        rows += [idx[jl[in_l]], idx[jr[in_r]]]
        cols += [cell[in_l], cell[in_r]]
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    m = scipy.sparse.coo_matrix((np.ones(len(rows), np.int32), (rows, cols)), shape=(len(start), n_cells)).tocsr()
    m.sort_indices()
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--windows", type=int, default=100_000)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--out")
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.get_cellcounts import cell_counts, mtx_text
    from nucleoatac_amd.writer import bgzip_file
    d = a.out or tempfile.mkdtemp(prefix="bench_cellcounts_")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    names = ["chr%d" % (k + 1) for k in range(a.refs)]
    per_ref = (a.windows + a.refs - 1) // a.refs
    L = per_ref * SLOT
    barcodes = [b"BC%010d-1" % k for k in range(a.cells)]
    t0 = time.perf_counter()
    plain = os.path.join(d, "cells.tsv")
    with open(plain, "w") as f:
        f.write("# id=bench\n")
        for k, c in enumerate(names):
            n = a.records // a.refs + (1 if k < a.records % a.refs else 0)
            s = np.sort(rng.integers(0, L - 600, n))
            e = s + rng.integers(30, 601, n)
            b = rng.integers(0, a.cells, n)
            row = c + "\t%d\t%d\tBC%010d-1\t1\n"
            for o in range(0, n, 1 << 16):
                blk = np.stack([s[o:o + (1 << 16)], e[o:o + (1 << 16)], b[o:o + (1 << 16)]], axis=1)
                f.write((row * len(blk)) % tuple(blk.ravel().tolist()))
    frag = bgzip_file(plain, os.path.join(d, "cells.tsv.gz"))
    w = np.arange(a.windows)
    chrom = (w // per_ref).astype(np.int32)
    start = (w % per_ref) * SLOT + rng.integers(0, SLOT - WIDTH, a.windows)
    order = rng.permutation(a.windows)
    chrom, start = chrom[order], start[order].astype(np.int64)
    end = start + WIDTH
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    dev = ctx.device_info()["name"]
    ctx.region_cell_counts([0, 5], [100, 100], [0, 1], 2, [0], [50])      # warm-up: code objects
    t0 = time.perf_counter()
    store, bc_count, n_un = FragmentStore.from_fragments_cells(frag, barcodes)
    t_read = time.perf_counter() - t0
    tm = {}
    t0 = time.perf_counter()
    indptr, indices, data = cell_counts(store, a.cells, names, chrom, start, end, 0, 500, timing=tm)
    t_merge = time.perf_counter() - t0
    t0 = time.perf_counter()
    text = mtx_text(indptr, indices, data, a.cells)
    t_text = time.perf_counter() - t0
    hits = int(np.asarray(data, np.int64).sum())
    out = dict(tool="bench_cellcounts", device=dev, records=a.records, cells=a.cells, windows=a.windows, refs=a.refs, file_bytes=os.path.getsize(frag),
               unassigned=n_un, nnz=int(indptr[-1]), hits=hits, hits_per_row=round(hits / max(a.windows, 1), 1), text_bytes=len(text),
               gen_s=round(t_gen, 3), read_s=round(t_read, 3), device_s=round(tm["device_s"], 4), kernel_ms=round(tm["kernel_ms"], 3),
               merge_s=round(t_merge, 4), text_s=round(t_text, 3))
    if not a.no_scipy:
        t0 = time.perf_counter()
        m = scipy_matrix(store, a.cells, names, chrom, start, end, 0, 500)
        out["scipy_s"] = round(time.perf_counter() - t0, 3)
        out["equal"] = bool(np.array_equal(m.indptr, indptr) and np.array_equal(m.indices, indices) and np.array_equal(m.data, data))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
