"""Wall time of the truncated SVD behind `pyatac cluster` (Context.sparse_lsi, csrc/natac_lsi.hpp) on a synthetic cell-by-window matrix,
its kernel span against that wall time, and the same algorithm in NumPy / scipy.sparse on the same arrays on the same box as the point of
comparison.  Prints one JSON line.

The workload: --entries (window, cell) draws over --windows x --cells, half of them uniform and half inside the cell group's own tenth of
the windows (ten groups), duplicates summed to counts; TF-IDF weights as the command forms them; r = --r columns, --iterations rounds, the
log transform.

  gen_s      making the matrix and its weights (not part of any figure)
  device_s   one Context.sparse_lsi call: operand checks, the host's counting sort for the cell-order copy, upload, every kernel, the
             host's r x r steps and their round trips, download, the sign rule
  kernel_ms  first to last kernel of that call on the stream (device events; the round trips in between are inside)
  scipy_s    the restatement: the weighted matrix as scipy CSR and its transpose, numpy.linalg.qr for orth, numpy.linalg.eigh (--no-scipy skips)
  sigma_diff max |sigma_device - sigma_scipy| / sigma[0]
usage: python tools/bench_lsi.py [--cells 10000] [--windows 100000] [--entries 3100000] [--r 40] [--iterations 4] [--no-scipy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scipy_lsi(indptr, indices, data, n_cells, row_weight, col_scale, r, n_iter, q0, scale):
    import scipy.sparse as sp
    m = len(indptr) - 1
    rows = np.repeat(np.arange(m), np.diff(indptr))
    v = np.log1p(data.astype(np.float64) * col_scale[indices] * row_weight[rows] * scale)
    Xt = sp.csr_matrix((v, indices, indptr), shape=(m, n_cells))
    X = Xt.T.tocsr()
    q0 = q0.copy()
    q0[~(row_weight > 0)] = 0.0
    Q = np.linalg.qr(q0)[0]
    for _ in range(n_iter):
        Y = np.linalg.qr(X.dot(Q))[0]
        Q = np.linalg.qr(Xt.dot(Y))[0]
    Y = X.dot(Q)
    lam, W = np.linalg.eigh(Y.T.dot(Y))
    return np.sqrt(lam[::-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--windows", type=int, default=100_000)
    ap.add_argument("--entries", type=int, default=3_100_000)
    ap.add_argument("--r", type=int, default=40)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    import scipy.sparse as sp
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.get_cluster import SCALE, tfidf_weights
    t0 = time.perf_counter()
    rng = np.random.default_rng(1)
    cell = rng.integers(0, a.cells, a.entries)
    tenth = max(a.windows // 10, 1)
    own = (cell % 10) * tenth + rng.integers(0, tenth, a.entries)
    win = np.where(rng.random(a.entries) < 0.5, own, rng.integers(0, a.windows, a.entries))
    A = sp.coo_matrix((np.ones(a.entries, np.int32), (win, cell)), shape=(a.windows, a.cells)).tocsr()
    A.sort_indices()
    indptr, indices, data = A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.int32)
    total, row_weight, col_scale = tfidf_weights(indptr, indices, data, a.cells)
    q0 = rng.standard_normal((a.windows, a.r))
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    dev = ctx.device_info()["name"]
    ctx.sparse_lsi([0, 1, 2], [0, 1], [1, 1], 2, [1.0, 1.0], [1.0, 1.0], 1, 1, [[1.0], [2.0]])      # warm-up: code objects
    t0 = time.perf_counter()
    sigma, U, V, ms = ctx.sparse_lsi(indptr, indices, data, a.cells, row_weight, col_scale, a.r, a.iterations, q0, scale=SCALE,
                                     with_kernel_ms=True)
    t_dev = time.perf_counter() - t0
    out = dict(tool="bench_lsi", device=dev, cells=a.cells, windows=a.windows, nnz=int(indptr[-1]), r=a.r, iterations=a.iterations,
               max_row=int(np.diff(indptr).max()), max_col=int(np.bincount(indices, minlength=a.cells).max()), gen_s=round(t_gen, 3),
               device_s=round(t_dev, 4), kernel_ms=round(ms, 3), kernel_share=round(ms / 1e3 / t_dev, 3), sigma0=float(sigma[0]))
    if not a.no_scipy:
        t0 = time.perf_counter()
        s_ref = scipy_lsi(indptr, indices, data, a.cells, row_weight, col_scale, a.r, a.iterations, q0, SCALE)
        out["scipy_s"] = round(time.perf_counter() - t0, 3)
        out["sigma_diff"] = float(np.abs(sigma - s_ref).max() / s_ref[0])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
