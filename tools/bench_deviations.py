"""Wall time of the device part of `pyatac deviations` (Context.motif_deviations, csrc/natac_deviations.hpp) on a synthetic count matrix and
motif matrix, its kernel time against that wall time, and the same result through scipy.sparse products on the same arrays on the same box
as the point of comparison.  Prints one JSON line.

The workload (fixed seeds): the count matrix of tools/bench_lsi.py -- --entries (window, cell) draws over --windows x --cells, half of them
uniform and half inside the cell group's own tenth of the windows, duplicates summed -- with every window and cell given at least one
count; --motifs motifs that each hit a window with probability --hit-density (the density tools/bench_motifs.py measures: 4.57 M entries
in 100,000 x 500); a uniform random GC content per window; the background table by the command's own rule, --iterations sets.

  gen_s        making the matrices and the background table (not part of any figure)
  warmup_s     one small call before the runs: the code objects and the context (not part of any figure)
  device_s     one Context.motif_deviations call per run: the binding's stable sort of the hits by motif, the host's operand checks and row
               split, the uploads, the kernel, the download of the three fp64 arrays
  kernel_ms    device events around the kernel, per run
  gathered     entries of X the kernel adds up: for every motif and set, the entries of the rows it visits; and gathered / kernel time
  scipy_s      the restatement: for every set b the product H^T X[bg_b] with scipy.sparse (int64), E_b from the row sums, then the fp64
               statistics in NumPy in the rule's order (--no-scipy skips)
  equal        the three fp64 arrays the same bytes as the restatement's; int_equal: O_b and E_b of the first --int-motifs motifs from the
               entry's testing output equal to the restatement's
usage: python tools/bench_deviations.py [--cells 10000] [--windows 100000] [--entries 3100000] [--motifs 500] [--hit-density 0.0914]
                                        [--iterations 50] [--runs 3] [--int-motifs 3] [--no-scipy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scipy_deviations(X, H, bg, d, T):
    """(raw, bg_mean, bg_m2, O of every set for the first motifs' check, E) through scipy.sparse products"""
    Ht = H.T.tocsr().astype(np.int64)
    rs = np.asarray(X.sum(axis=1)).ravel().astype(np.int64)
    df, Tf = d.astype(np.float64), np.float64(T)
    mean = m2 = raw = None
    O_all, E_all = [], []
    for b in range(bg.shape[0] + 1):
        Xb = X if b == 0 else X[bg[b - 1]]
        O = np.asarray((Ht @ Xb).todense(), dtype=np.int64)
        E = Ht @ (rs if b == 0 else rs[bg[b - 1]])
        O_all.append(O[:8].copy())
        E_all.append(E)
        x = E.astype(np.float64)[:, None] * df[None, :]
        x /= Tf
        Y = (O.astype(np.float64) - x) / x
        if b == 0:
            raw, mean, m2 = Y, np.zeros_like(Y), np.zeros_like(Y)
            continue
        delta = Y - mean
        mean = mean + delta / np.float64(b)
        m2 = m2 + delta * (Y - mean)
    return raw, mean, m2, np.array(O_all), np.array(E_all)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--windows", type=int, default=100_000)
    ap.add_argument("--entries", type=int, default=3_100_000)
    ap.add_argument("--motifs", type=int, default=500)
    ap.add_argument("--hit-density", type=float, default=0.0914)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--int-motifs", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    import scipy.sparse as sp
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.get_deviations import background_table
    t0 = time.perf_counter()
    rng = np.random.default_rng(1)
    cell = rng.integers(0, a.cells, a.entries)
    tenth = max(a.windows // 10, 1)
    own = (cell % 10) * tenth + rng.integers(0, tenth, a.entries)
    win = np.where(rng.random(a.entries) < 0.5, own, rng.integers(0, a.windows, a.entries))
    win = np.concatenate([win, np.arange(a.windows), rng.integers(0, a.windows, a.cells)])       # no empty window, no empty cell
    cell = np.concatenate([cell, rng.integers(0, a.cells, a.windows), np.arange(a.cells)])
    X = sp.coo_matrix((np.ones(len(win), np.int64), (win, cell)), shape=(a.windows, a.cells)).tocsr()
    X.sort_indices()
    H = sp.csr_matrix(rng.random((a.windows, a.motifs)) < a.hit_density)
    H.sort_indices()
    keep = np.flatnonzero(np.diff(H.tocsc().indptr) > 0)                                         # a motif without a hit is not passed on
    H = H[:, keep].tocsr()
    H.sort_indices()
    M = H.shape[1]
    rs = np.asarray(X.sum(axis=1)).ravel().astype(np.int64)
    d = np.asarray(X.sum(axis=0)).ravel().astype(np.int64)
    T = int(rs.sum())
    bg, grid, extremes = background_table(rng.random(a.windows), rs, a.iterations)
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    ip, ix, da = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(np.int32)
    hp, hx = H.indptr.astype(np.int64), H.indices.astype(np.int64)
    t0 = time.perf_counter()
    ctx.motif_deviations([0, 1, 2], [0, 0], [1, 1], 1, [0, 1, 1], [0], 1, [[0, 1], [1, 1]])
    t_warm = time.perf_counter() - t0
    runs = []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        raw, mean, m2, ms = ctx.motif_deviations(ip, ix, da, a.cells, hp, hx, M, bg, with_kernel_ms=True)
        runs.append(dict(device_s=round(time.perf_counter() - t0, 4), kernel_ms=round(ms, 3)))
    row_len = np.diff(ip)
    per_window = np.asarray(H.sum(axis=1)).ravel().astype(np.int64)                             # motifs that visit window p in set 0
    gathered = int((row_len * per_window).sum()) + sum(int((row_len[bg[b]] * per_window).sum()) for b in range(a.iterations))
    best = min(r["kernel_ms"] for r in runs)
    out = dict(tool="bench_deviations", device=ctx.device_info()["name"], cells=a.cells, windows=a.windows, nnz=int(ip[-1]), total=T, motifs=M,
               hits=int(hp[-1]), iterations=a.iterations, grid=list(grid), grid_extremes=list(extremes), gen_s=round(t_gen, 3),
               warmup_s=round(t_warm, 3), runs=runs, gathered=gathered, gathered_per_s=round(gathered / (best / 1e3), 1))
    if not a.no_scipy:
        t0 = time.perf_counter()
        r_raw, r_mean, r_m2, r_O, r_E = scipy_deviations(X, H, bg, d, T)
        out["scipy_s"] = round(time.perf_counter() - t0, 3)
        out["equal"] = bool(raw.tobytes() == r_raw.tobytes() and mean.tobytes() == r_mean.tobytes() and m2.tobytes() == r_m2.tobytes())
        with np.errstate(invalid="ignore", divide="ignore"):
            out["max_abs_diff"] = [float(np.abs(x - y).max()) for x, y in ((raw, r_raw), (mean, r_mean), (m2, r_m2))]
        k = min(a.int_motifs, M, 8)
        sub = H[:, :k].tocsr()
        sub.sort_indices()
        got = ctx.motif_deviations(ip, ix, da, a.cells, sub.indptr.astype(np.int64), sub.indices.astype(np.int64), k, bg, with_sums=True)
        out["int_motifs"] = k
        out["int_equal"] = bool(np.array_equal(got[3], r_O[:, :k]) and np.array_equal(got[4], r_E[:, :k]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
