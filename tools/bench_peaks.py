"""Wall time of the device part of `pyatac peaks` (nucleoatac_amd/pyatac/get_peaks.py: call_peaks, one natac_enriched_regions call per
chromosome) on a synthetic genome, kernel milliseconds against wall time, and the same regions from the NumPy restatement
(tests/peaks_ref.py: bincount, cumsum, clipped differences) on the same box as the only point of comparison.  Prints one JSON line.

The workload: --records fragments of 30 to 600 bases over --refs chromosomes of --genome / --refs bases each; one fragment in five
starts within 150 bases of one of --hotspots planted centres, the others are uniform.  The store is made in memory (no file is read).
The command's default geometry: half_width 75, small 500, large 5000, mlog10p 5, max_gap 75, min_length 150.

  gen_s      making and sorting the arrays (not part of any figure)
  warmup_s   one small call before the runs: the code objects and the context (not part of any figure)
  device_s   the natac_enriched_regions calls of one run, one per chromosome: the host's operand checks, upload, both sweeps with the
             host's steps between them, download; one figure per run (--runs).  The first run's launches are in its figure; the pool keeps
             the device memory for the later runs
  kernel_ms  device events around the first and the last kernel of every call (the host's steps between the sweeps included), per run
  host_s     call_peaks whole, per run: device_s plus the critical-value tables (scipy), the kept-insertion count and the scores
  numpy_s    call_peaks whole with the restatement as its per-chromosome finder, on the same arrays (compare with host_s)
  equal      the two results are the same in all six arrays and both counts
usage: python tools/bench_peaks.py [--records 10000000] [--genome 200000000] [--refs 4] [--hotspots 10000] [--runs 3] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--genome", type=int, default=200_000_000)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--hotspots", type=int, default=10_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.get_peaks import call_peaks
    rng = np.random.default_rng(1)
    names = ["chr%d" % (k + 1) for k in range(a.refs)]
    n = a.genome // a.refs
    t0 = time.perf_counter()
    pos, tlen = {}, {}
    for k, c in enumerate(names):
        m = a.records // a.refs
        centres = rng.integers(1000, n - 1000, max(a.hotspots // a.refs, 1))
        p = rng.integers(0, n - 700, m)
        hot = rng.random(m) < 0.2
        p[hot] = centres[rng.integers(0, len(centres), int(hot.sum()))] + rng.integers(-150, 151, int(hot.sum()))
        p.sort()
        pos[c], tlen[c] = p.astype(np.int64), rng.integers(30, 601, m).astype(np.int64)
    store = FragmentStore(names, [n] * a.refs, pos, tlen)
    sizes = store.chrom_sizes()
    gen_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    get_context().enriched_regions([0, 5], [100, 100], 1000, [0, 9], [0, 9], 1, 2, 5, 20, 0, 1)      # warm-up: code objects
    warmup_s = time.perf_counter() - t0
    runs, res = [], None
    for _ in range(a.runs):
        t = {}
        t0 = time.perf_counter()
        res = call_peaks(store, sizes, timing=t)
        runs.append(dict(host_s=round(time.perf_counter() - t0, 4), device_s=round(t["device_s"], 4), kernel_ms=round(t["kernel_ms"], 3)))
    out = dict(records=a.records, genome=a.genome, refs=a.refs, hotspots=a.hotspots, segment=os.environ.get("NATAC_PEAKS_SEGMENT", "default"),
               gen_s=round(gen_s, 2), warmup_s=round(warmup_s, 3), runs=runs, regions_found=res["regions_found"],
               regions_kept=res["regions_kept"], significant_bases=res["significant_bases"], min_pileup=res["min_pileup"])
    if not a.no_numpy:
        import peaks_ref as R
        t0 = time.perf_counter()
        ref = call_peaks(store, sizes, regions=lambda *x: R.enriched_regions(*x, counts=True))
        out["numpy_s"] = round(time.perf_counter() - t0, 2)
        keys = ("chrom", "start", "end", "summit", "pileup", "n_small", "n_large")
        out["equal"] = bool(all(np.array_equal(res[k], ref[k]) and res[k].dtype == ref[k].dtype for k in keys) and
                            all(res[k] == ref[k] for k in ("regions_found", "regions_kept", "significant_bases")))
    print(json.dumps(out))
    return 0 if out.get("equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
