"""Wall time by phase of `pyatac genescores` (nucleoatac_amd/pyatac/get_genescores.py) on the synthetic single-cell workload of
tools/bench_cellcounts.py, kernel milliseconds against wall time, and the NumPy restatement of tests/genescores_ref.py on a stated subset
of the genes on the same box, with equality asserted there.  One box, one process, --runs runs after a warm-up call.  Prints one JSON line.

The workload: --records fragments of 30 to 600 bases, uniform over --refs chromosomes of 50 Mbp (at the defaults), each in one of --cells
cells (uniform), written as a BGZF fragment file with every cell listed; --genes genes, one per 10 kb slot at a random offset in its first
half, lengths drawn from 1 to 50 kb, random strands, in random BED order, with the command's default geometry (upstream 5,000, windows of
1,000 to 100,000 bases beyond the body that stop at the nearest gene wholly beyond, decay 5,000, unit 256, sizes 0 to 1000).

  gen_s       making the file (not part of any figure)
  read_s      FragmentStore.from_fragments_cells: the host decoder with the cell of every record kept, and the store's sort
  device_s    per run: the natac_gene_cell_scores calls, two per chromosome (sizing, filling): uploads, kernels, host round trips, download
  kernel_ms   per run: first to last kernel of those calls on the stream (device events; the round trips in between are inside)
  merge_s     per run: device_s plus putting the per-chromosome matrices into BED row order (get_genescores.gene_scores)
  hits, entries, rows_short, rows_table, short_max, tile, n_tiles
  ref_genes   the subset the restatement ran on: every (genes // ref_genes)-th gene in BED order
  ref_s       its time on the store's arrays (no read, no text); equal: its rows are the device's rows
--also-short-max-1 repeats the device runs in the same process with NATAC_GENESCORES_SHORT_MAX=1, which sends every row of more than one
hit to the table arm, prints a second JSON line and asserts the same bytes: the sweep that decides what the short arm is worth.  At the
default 10 M records every row has thousands of hits and none is short; --records 100000 (a shallow sample) puts the rows around 64 hits.
usage: python tools/bench_genescores.py [--records 10000000] [--cells 10000] [--genes 20000] [--refs 4] [--runs 3] [--ref-genes 200] [--out DIR]
                                        [--also-short-max-1]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SLOT = 10000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--genes", type=int, default=20_000)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ref-genes", type=int, default=200)
    ap.add_argument("--out")
    ap.add_argument("--also-short-max-1", action="store_true")
    a = ap.parse_args()
    import genescores_ref as R
    from nucleoatac_amd import get_context
    from nucleoatac_amd.device import gene_cell_scores_plan
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.get_genescores import gene_scores, gene_windows, weight_table
    from nucleoatac_amd.writer import bgzip_file
    d = a.out or tempfile.mkdtemp(prefix="bench_genescores_")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    names = ["chr%d" % (k + 1) for k in range(a.refs)]
    per_ref = (a.genes + a.refs - 1) // a.refs
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
    g = np.arange(a.genes)
    chrom = (g // per_ref).astype(np.int64)
    start = (g % per_ref) * SLOT + rng.integers(0, SLOT // 2, a.genes)
    end = np.minimum(start + rng.integers(1000, 50001, a.genes), L)
    minus = rng.random(a.genes) < 0.5
    order = rng.permutation(a.genes)
    chrom, start, end, minus = chrom[order], start[order].astype(np.int64), end[order].astype(np.int64), minus[order]
    t_gen = time.perf_counter() - t0
    bs, be, wl, wh = gene_windows(chrom, start, end, minus)
    weight = weight_table(100000, 5000, 256)
    ctx = get_context()
    dev = ctx.device_info()["name"]
    ctx.gene_cell_scores([0, 5], [100, 100], [0, 1], 2, [0], [40], [10], [20], [3, 2, 1] + [1] * 20, 0, 1000)      # warm-up: code objects
    t0 = time.perf_counter()
    store, bc_count, n_un = FragmentStore.from_fragments_cells(frag, barcodes)
    t_read = time.perf_counter() - t0

    def device_runs():
        dev_s, ker_ms, merge_s = [], [], []
        for _ in range(a.runs):
            tm = {}
            t0 = time.perf_counter()
            res = gene_scores(store, a.cells, names, chrom, wl, wh, bs, be, weight, 0, 1000, timing=tm)
            merge_s.append(round(time.perf_counter() - t0, 4))
            dev_s.append(round(tm["device_s"], 4))
            ker_ms.append(round(tm["kernel_ms"], 3))
        return res, dev_s, ker_ms, merge_s

    (indptr, indices, data, hits, arms), dev_s, ker_ms, merge_s = device_runs()
    plan = gene_cell_scores_plan(a.genes, a.cells, int(arms[1]))
    out = dict(tool="bench_genescores", device=dev, records=a.records, cells=a.cells, genes=a.genes, refs=a.refs, file_bytes=os.path.getsize(frag),
               unassigned=n_un, gen_s=round(t_gen, 3), read_s=round(t_read, 3), device_s=dev_s, kernel_ms=ker_ms, merge_s=merge_s,
               hits=int(hits.sum()), hits_per_row=round(float(hits.mean()), 1), longest_row_hits=int(hits.max()), entries=int(indptr[-1]),
               rows_short=int(arms[0]), rows_table=int(arms[1]), short_max=plan["short_max"], tile=plan["tile"], n_tiles=plan["n_tiles"],
               window_bases_mean=round(float((wh - wl).mean()), 1))
    if a.ref_genes > 0:
        sub = np.arange(0, a.genes, max(1, a.genes // a.ref_genes))
        t0 = time.perf_counter()
        equal = True
        for k, c in enumerate(names):
            idx = sub[chrom[sub] == k]
            ptr, col, val, h = R.gene_cell_scores(store.pos[c], store.tlen[c], store.cell[c], a.cells, wl[idx], wh[idx], bs[idx], be[idx], weight, 0,
                                                  1000, with_hits=True)
            for j, row in enumerate(idx):
                lo, hi = indptr[row], indptr[row + 1]
                equal = equal and np.array_equal(indices[lo:hi], col[ptr[j]:ptr[j + 1]]) and np.array_equal(data[lo:hi], val[ptr[j]:ptr[j + 1]]) \
                    and hits[row] == h[j]
        out.update(ref_genes=len(sub), ref_s=round(time.perf_counter() - t0, 3), ref_entries=int((indptr[sub + 1] - indptr[sub]).sum()), equal=bool(equal))
        assert equal, "the restatement's rows differ from the device's"
    print(json.dumps(out))
    if a.also_short_max_1:
        # the same store and genes once more with every row of more than one hit in the table arm (the entry reads the variable per call)
        os.environ["NATAC_GENESCORES_SHORT_MAX"] = "1"
        (ip2, ix2, da2, _, arms2), dev_s, ker_ms, merge_s = device_runs()
        same = bool(np.array_equal(ip2, indptr) and np.array_equal(ix2, indices) and np.array_equal(da2, data))
        print(json.dumps(dict(tool="bench_genescores", device=dev, records=a.records, cells=a.cells, genes=a.genes, short_max=1, device_s=dev_s,
                              kernel_ms=ker_ms, merge_s=merge_s, rows_short=int(arms2[0]), rows_table=int(arms2[1]), same_bytes=same)))
        assert same, "NATAC_GENESCORES_SHORT_MAX=1 changed the matrix"


if __name__ == "__main__":
    main()
