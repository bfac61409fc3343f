"""Wall time of the device part of `pyatac markers` (Context.group_rank_sums, csrc/natac_markers.hpp) on a synthetic count matrix, its
kernel time against that wall time, the rows every arm took, and the exact restatement of tests/markers_ref.py on a subset of the rows on
the same box as the point of comparison.  Prints one JSON line.

The workload (fixed seeds): the count matrix of tools/bench_lsi.py -- --entries (window, cell) draws over --windows x --cells, half of them
uniform and half inside the cell group's own tenth of the windows, duplicates summed -- in which the first --open-rows windows are also
open in every second cell (a draw per cell), as promoters are; the depth is the column sum; the cells are dealt to the groups in turn.
Every group count of --groups is a run of its own.

  gen_s        making the matrix (not part of any figure)
  warmup_s     one small call before the runs: the code objects and the context (not part of any figure)
  device_s     one Context.group_rank_sums call per run: the host's operand checks and row lists, the uploads, the kernels, the download of
               the four integer arrays
  kernel_ms    device events around the call's kernels, per run
  arm_rows     the rows the short, block and long arm took
  arms         the --open-rows windows alone, once under the defaults (the block arm takes them) and once with NATAC_MARKERS_BLOCK_MAX
               = 4096 (the long arm takes them, two chunks a row): kernel_ms and entries per second of each, and whether the bytes agree
  ref_s        tests/markers_ref.rank_sums (exact rationals, one row at a time) on --ref-rows rows, the first --ref-open of them from the
               open rows, with ref_entries entries; ref_equal: the device's four arrays equal it on those rows
With --sweep instead: the arms by row length.  For every L of --lengths, --sweep-rows rows of exactly L entries over --cells cells in 8
groups go through the block arm (NATAC_MARKERS_SHORT_MAX = 16, block_max 8192), through the long arm (block_max = the largest power of two
below L, so two chunks a row) and, up to 64 entries, through the short arm: the best kernel_ms of --runs each and whether the bytes agree.
usage: python tools/bench_markers.py [--cells 10000] [--windows 100000] [--entries 3100000] [--open-rows 1000] [--groups 8 64] [--runs 3]
                                     [--ref-rows 2000] [--ref-open 20] [--no-ref]
       python tools/bench_markers.py --sweep [--lengths 48 96 ...] [--sweep-rows 2000] [--cells 10000] [--runs 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def take_rows(ip, ix, da, rows):
    n = np.diff(ip)[rows]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(n, out=ptr[1:])
    src = np.repeat(ip[:-1][rows] - ptr[:-1], n) + np.arange(int(ptr[-1]), dtype=np.int64)
    return ptr, ix[src], da[src]


def sweep(a):
    from nucleoatac_amd import get_context
    ctx = get_context()
    N, G = a.cells, 8
    rng = np.random.default_rng(5)
    depth = rng.integers(200, 2000, N).astype(np.int64)
    group = (np.arange(N) % G).astype(np.int32)
    ctx.group_rank_sums([0, 1, 2], [0, 1], [1, 1], 2, [1, 1], [0, 1], 2)
    out = []
    for L in a.lengths:
        ix = np.concatenate([np.sort(rng.choice(N, L, replace=False)) for _ in range(a.sweep_rows)]).astype(np.int32)
        da = rng.integers(1, 4, a.sweep_rows * L).astype(np.int32)
        ip = np.arange(a.sweep_rows + 1, dtype=np.int64) * L
        rec, first = dict(L=L), None
        below = 1 << (int(L).bit_length() - 1)
        for name, short, block in (("block", 16, 8192), ("long", 16, below if below < L else below // 2), ("short", 64, 8192)):
            if name == "short" and L > 64:
                continue
            os.environ["NATAC_MARKERS_SHORT_MAX"], os.environ["NATAC_MARKERS_BLOCK_MAX"] = str(short), str(block)
            best = None
            for _ in range(a.runs):
                got = ctx.group_rank_sums(ip, ix, da, N, depth, group, G, with_arm_rows=True, with_kernel_ms=True)
                best = got[5] if best is None else min(best, got[5])
            now = [x.tobytes() for x in got[:4]]
            first = first or now
            rec[name] = dict(block_max=block, arm_rows=got[4].tolist(), kernel_ms=round(best, 3), same=now == first)
        out.append(rec)
    print(json.dumps(dict(tool="bench_markers --sweep", device=ctx.device_info()["name"], cells=N, rows=a.sweep_rows, lengths=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--windows", type=int, default=100_000)
    ap.add_argument("--entries", type=int, default=3_100_000)
    ap.add_argument("--open-rows", type=int, default=1000)
    ap.add_argument("--groups", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ref-rows", type=int, default=2000)
    ap.add_argument("--ref-open", type=int, default=20)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--lengths", type=int, nargs="+", default=[48, 96, 192, 384, 768, 1536, 3072, 6144])
    ap.add_argument("--sweep-rows", type=int, default=2000)
    a = ap.parse_args()
    if a.sweep:
        return sweep(a)
    import scipy.sparse as sp
    from nucleoatac_amd import get_context
    t0 = time.perf_counter()
    rng = np.random.default_rng(1)
    cell = rng.integers(0, a.cells, a.entries)
    tenth = max(a.windows // 10, 1)
    own = (cell % 10) * tenth + rng.integers(0, tenth, a.entries)
    win = np.where(rng.random(a.entries) < 0.5, own, rng.integers(0, a.windows, a.entries))
    half = np.arange(0, a.cells, 2)
    win = np.concatenate([win, np.repeat(np.arange(a.open_rows), len(half)), rng.integers(0, a.windows, a.cells)])      # no empty cell
    cell = np.concatenate([cell, np.tile(half, a.open_rows), np.arange(a.cells)])
    X = sp.coo_matrix((np.ones(len(win), np.int64), (win, cell)), shape=(a.windows, a.cells)).tocsr()
    X.sort_indices()
    ip, ix, da = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(np.int32)
    depth = np.asarray(X.sum(axis=0)).ravel().astype(np.int64)
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    t0 = time.perf_counter()
    ctx.group_rank_sums([0, 1, 2], [0, 1], [1, 1], 2, [1, 1], [0, 1], 2)
    t_warm = time.perf_counter() - t0
    row_len = np.diff(ip)
    out = dict(tool="bench_markers", device=ctx.device_info()["name"], cells=a.cells, windows=a.windows, nnz=int(ip[-1]), open_rows=a.open_rows,
               longest_row=int(row_len.max()), mean_row=round(float(row_len.mean()), 2), gen_s=round(t_gen, 3), warmup_s=round(t_warm, 3), groups=[])
    open_csr = take_rows(ip, ix, da, np.arange(a.open_rows))
    ref_rows = np.unique(np.concatenate([np.arange(min(a.ref_open, a.open_rows)),
                                         np.random.default_rng(2).choice(a.windows, min(a.ref_rows, a.windows), replace=False)]))
    for G in a.groups:
        group = (np.arange(a.cells) % G).astype(np.int32)
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            res = ctx.group_rank_sums(ip, ix, da, a.cells, depth, group, G, with_arm_rows=True, with_kernel_ms=True)
            runs.append(dict(device_s=round(time.perf_counter() - t0, 4), kernel_ms=round(res[5], 3)))
        rec = dict(n_groups=G, runs=runs, arm_rows=res[4].tolist())
        arms = {}
        for name, forced in (("block", None), ("long", "4096")):
            if forced is None:
                os.environ.pop("NATAC_MARKERS_BLOCK_MAX", None)
            else:
                os.environ["NATAC_MARKERS_BLOCK_MAX"] = forced
            best, got = None, None
            for _ in range(a.runs):
                got = ctx.group_rank_sums(open_csr[0], open_csr[1], open_csr[2], a.cells, depth, group, G, with_arm_rows=True, with_kernel_ms=True)
                best = got[5] if best is None else min(best, got[5])
            arms[name] = dict(arm_rows=got[4].tolist(), kernel_ms=round(best, 3), entries_per_s=round(int(open_csr[0][-1]) / (best / 1e3), 1),
                              bytes=[x.tobytes() for x in got[:4]])
        os.environ.pop("NATAC_MARKERS_BLOCK_MAX", None)
        arms["same_bytes"] = arms["block"].pop("bytes") == arms["long"].pop("bytes")
        rec["arms"] = arms
        if not a.no_ref:
            import markers_ref
            sub = take_rows(ip, ix, da, ref_rows)
            t0 = time.perf_counter()
            want = markers_ref.rank_sums(sub[0], sub[1], sub[2], a.cells, depth, group, G)
            rec["ref_s"] = round(time.perf_counter() - t0, 3)
            rec["ref_rows"], rec["ref_entries"] = len(ref_rows), int(sub[0][-1])
            rec["ref_equal"] = bool(all(np.array_equal(x[ref_rows], y) for x, y in zip(res[:4], want)))
        out["groups"].append(rec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
