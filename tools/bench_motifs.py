"""Wall time of the device part of `pyatac motifs` (nucleoatac_amd/pyatac/get_motifs.py: scan, one natac_motif_scan call per chromosome)
on a synthetic genome, kernel milliseconds against wall time, the table look-up rate, and the same sites and matrix from the NumPy
restatement (tests/motifs_ref.py) on a stated fraction of the windows as the only point of comparison.  Prints one JSON line.

The workload (fixed seeds): --refs chromosomes of --genome / --refs random bases each, --windows non-overlapping windows of --width bases
spread evenly over them, --motifs random count matrices of 8 to 20 columns, thresholds at --pvalue under a uniform background.

  gen_s        making the genome, the windows and the motifs (not part of any figure)
  warmup_s     one small call before the runs: the code objects and the context (not part of any figure)
  device_s     the natac_motif_scan calls of one run, one per chromosome: the host's operand checks and table building, the upload of
               the chromosome, all kernels, the round trip for the hit count, the download of hits and counts; one figure per run
  kernel_ms    device events around the first and the last kernel of every call (the round trip between them included), per run
  lookups      column look-ups of one run: for every motif, its columns times the window starts it is scored at.  One look-up is one
               ds_read_b32 that serves both strands (all these motifs take the packed accumulator; `wide_motifs` says if not)
  lookups_per_s  lookups / kernel time, and lds_peak = 32 lanes x CUs x --clock-ghz, the ds_read_b32 rate of the LDS
  numpy_s      the restatement on the first --numpy-windows windows of the first chromosome (fraction = that / --windows), the device on the
               same windows, and `equal` = all five arrays the same
usage: python tools/bench_motifs.py [--genome 200000000] [--refs 4] [--windows 100000] [--width 500] [--motifs 500] [--runs 3]
                                    [--numpy-windows 100] [--clock-ghz 2.4]"""
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
    ap.add_argument("--genome", type=int, default=200_000_000)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--windows", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=500)
    ap.add_argument("--pvalue", type=float, default=1e-4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--numpy-windows", type=int, default=100)
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    a = ap.parse_args()
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.get_motifs import scan, scores, threshold
    from nucleoatac_amd.pyatac.seq import FastaStore
    import motifs_ref as R
    t0 = time.perf_counter()
    rng = np.random.default_rng(1)
    names = ["chr%d" % (k + 1) for k in range(a.refs)]
    n = a.genome // a.refs
    acgt = np.frombuffer(b"ACGT", np.uint8)
    fasta = FastaStore({c: acgt[rng.integers(0, 4, n, dtype=np.uint8)] for c in names})
    per = a.windows // a.refs
    step = n // per
    assert step > a.width, "the windows would touch"
    start1 = np.arange(per, dtype=np.int64) * step + rng.integers(0, step - a.width, per)
    fc = np.repeat(np.arange(a.refs, dtype=np.int32), per)
    start = np.tile(start1, a.refs)
    end = start + a.width
    bg = np.full(4, 0.25)
    mrng = np.random.default_rng(2)
    S_list = [scores(R.random_counts(mrng, int(w)), bg, 0.8) for w in mrng.integers(8, 21, a.motifs)]
    widths = np.array([len(S) for S in S_list], np.int32)
    S_flat = np.concatenate(S_list).astype(np.int32)
    T = np.array([threshold(S, bg, a.pvalue)[0] for S in S_list], np.int32)
    wide = int(sum(int((S.max(axis=1) - S.min(axis=1)).sum()) > 65535 for S in S_list))
    gen_s = time.perf_counter() - t0
    ctx = get_context()
    t0 = time.perf_counter()
    ctx.motif_scan(fasta.seqs[names[0]][:4096], [0], [4096], widths[:2], S_flat[:int(widths[:2].sum())], T[:2])
    warmup_s = time.perf_counter() - t0
    runs, hits, matrix = [], None, None
    for _ in range(a.runs):
        t = {}
        t0 = time.perf_counter()
        hits, matrix = scan(fasta, fc, start, end, widths, S_flat, T, timing=t)
        runs.append(dict(host_s=round(time.perf_counter() - t0, 4), device_s=round(t["device_s"], 4), kernel_ms=round(t["kernel_ms"], 3)))
    lookups = int(((a.width - widths.astype(np.int64) + 1).clip(0) * widths).sum()) * len(start)
    best_ms = min(r["kernel_ms"] for r in runs)
    n_cu = ctx.device_info()["n_cu"]
    out = dict(genome=a.genome, refs=a.refs, windows=len(start), width=a.width, motifs=a.motifs, pvalue=a.pvalue, wide_motifs=wide,
               columns=int(widths.sum()), gen_s=round(gen_s, 2), warmup_s=round(warmup_s, 3), runs=runs, hits=int(len(hits[1])),
               nnz=int(len(matrix[1])), lookups=lookups, lookups_per_s=round(lookups / (best_ms * 1e-3), 0),
               lds_peak_lookups_per_s=32.0 * n_cu * a.clock_ghz * 1e9, cus=int(n_cu))
    if a.numpy_windows > 0:
        k = min(a.numpy_windows, per)
        seq = fasta.seqs[names[0]][:int(end[k - 1])]           # the restatement works on whole arrays: the chromosome up to the last window
        t0 = time.perf_counter()
        want = R.scan(seq, start[:k], end[:k], widths, S_flat, T)
        out["numpy_s"] = round(time.perf_counter() - t0, 2)
        out["numpy_windows"] = k
        out["numpy_fraction"] = k / float(len(start))
        got = ctx.motif_scan(seq, start[:k], end[:k], widths, S_flat, T)
        out["equal"] = bool(all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, want)))
    print(json.dumps(out))
    return 0 if out.get("equal", True) else 1


if __name__ == "__main__":
    sys.exit(main())
