"""Wall time by phase of `pyatac cellqc` (nucleoatac_amd/pyatac/get_cellqc.py) on a synthetic single-cell workload, kernel milliseconds
against wall time, and the same four arrays from the NumPy restatement (tests/cellqc_ref.py: searchsorted + bincount) on the same box as
the point of comparison.  Prints one JSON line.

The workload: --records fragments of 30 to 600 bases over --refs chromosomes of --peaks x 2,000 / --refs bases, each in one of --cells
cells (uniform), written as a BGZF fragment file with every cell listed; one fragment in five starts within 300 bases of a site, the
others are uniform.  --sites sites at random positions and strands; --peaks peaks of 500 bases, one in each 2,000-base slot at a random
offset.  The geometry is the command's default: flank 1000, center 500, edge 100.

  gen_s      making the file (not part of any figure)
  read_s     FragmentStore.from_fragments_cells: the host decoder with the cell of every record kept, and the store's sort
  device_s   the natac_cell_site_qc calls of one run, one per chromosome: the host's operand checks, upload, kernel, download; one figure
             per run (--runs)
  kernel_ms  the kernels of those calls (device events), per run
  numpy_s    the restatement on the store's arrays, per chromosome and added up (no read)
  equal      the two results are the same
usage: python tools/bench_cellqc.py [--records 10000000] [--cells 10000] [--sites 20000] [--peaks 100000] [--refs 4] [--runs 3] [--out DIR]
                                    [--no-numpy]"""
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
FLANK, CENTER, EDGE = 1000, 500, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--sites", type=int, default=20_000)
    ap.add_argument("--peaks", type=int, default=100_000)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.get_cellqc import cell_qc
    from nucleoatac_amd.writer import bgzip_file
    d = a.out or tempfile.mkdtemp(prefix="bench_cellqc_")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    names = ["chr%d" % (k + 1) for k in range(a.refs)]
    per_ref = (a.peaks + a.refs - 1) // a.refs
    L = per_ref * SLOT
    barcodes = [b"BC%010d-1" % k for k in range(a.cells)]
    t0 = time.perf_counter()
    sites, peaks = {}, {}
    for k, c in enumerate(names):
        n = a.sites // a.refs + (1 if k < a.sites % a.refs else 0)
        sites[c] = (np.sort(rng.integers(FLANK, L - FLANK, n)).astype(np.int64), rng.integers(0, 2, n).astype(np.uint8))
        n = min(per_ref, a.peaks - k * per_ref)
        s = np.arange(n, dtype=np.int64) * SLOT + rng.integers(0, SLOT - WIDTH, n)
        peaks[c] = (s, s + WIDTH)
    plain = os.path.join(d, "cells.tsv")
    with open(plain, "w") as f:
        f.write("# id=bench\n")
        for k, c in enumerate(names):
            n = a.records // a.refs + (1 if k < a.records % a.refs else 0)
            s = rng.integers(0, L - 600, n)
            near = rng.random(n) < 0.2
            if len(sites[c][0]):
                s = np.where(near, sites[c][0][rng.integers(0, len(sites[c][0]), n)] + rng.integers(-300, 300, n), s)
            s = np.sort(np.clip(s, 0, L - 600))
            e = s + rng.integers(30, 601, n)
            b = rng.integers(0, a.cells, n)
            row = c + "\t%d\t%d\tBC%010d-1\t1\n"
            for o in range(0, n, 1 << 16):
                blk = np.stack([s[o:o + (1 << 16)], e[o:o + (1 << 16)], b[o:o + (1 << 16)]], axis=1)
                f.write((row * len(blk)) % tuple(blk.ravel().tolist()))
    frag = bgzip_file(plain, os.path.join(d, "cells.tsv.gz"))
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    dev = ctx.device_info()["name"]
    ctx.cell_site_qc([0, 5], [100, 100], [0, 1], 2, [50], None, 10, 2, 2, [0], [50])      # warm-up: code objects
    t0 = time.perf_counter()
    store, bc_count, n_un = FragmentStore.from_fragments_cells(frag, barcodes)
    t_read = time.perf_counter() - t0
    device_s, kernel_ms = [], []
    for _ in range(max(a.runs, 1)):
        tm = {}
        got = cell_qc(store, a.cells, sites, peaks, FLANK, CENTER, EDGE, timing=tm)
        device_s.append(round(tm["device_s"], 4))
        kernel_ms.append(round(tm["kernel_ms"], 3))
    out = dict(tool="bench_cellqc", device=dev, records=a.records, cells=a.cells, sites=a.sites, peaks=a.peaks, refs=a.refs,
               flank=FLANK, center=CENTER, edge=EDGE, file_bytes=os.path.getsize(frag), unassigned=n_un, pairs=int(got[3].sum()),
               tss_center=int(got[0].sum()), tss_flank=int(got[1].sum()), in_peaks=int(got[2].sum()), gen_s=round(t_gen, 3),
               read_s=round(t_read, 3), runs=len(device_s), device_s=device_s, kernel_ms=kernel_ms)
    if not a.no_numpy:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from cellqc_ref import cellqc_ref
        t0 = time.perf_counter()
        want = None
        for c in store.references:
            part = cellqc_ref(store.pos[c], store.tlen[c], store.cell[c], a.cells, sites[c][0], sites[c][1], FLANK, CENTER, EDGE, *peaks[c])
            want = part if want is None else tuple(x + y for x, y in zip(want, part))
        out["numpy_s"] = round(time.perf_counter() - t0, 3)
        out["equal"] = bool(all(np.array_equal(x, y) for x, y in zip(got, want)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
