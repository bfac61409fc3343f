"""Wall time of the device part of `pyatac coaccess` (Context.window_pair_sums, csrc/natac_coaccess.hpp) on a synthetic count matrix, the
kernel time of both arms on that matrix, and the scipy.sparse restatement of tests/coaccess_ref.py on a subset of the owners on the same
box as the point of comparison.  Prints one JSON line.

The workload (fixed seeds): the count matrix of tools/bench_markers.py -- --entries (window, cell) draws over --windows x --cells, half of
them uniform and half inside the cell group's own tenth of the windows, duplicates summed, the first --open-rows windows also open in every
second cell -- with the windows laid out on --chroms chromosomes, --spacing bases apart; every window is listed, and the pairs are those of
get_coaccess.pair_lists at --max-distance.

  gen_s        making the matrix and the pair lists (not part of any figure)
  warmup_s     one small call before the runs: the code objects and the context (not part of any figure)
  pairs        the pairs of the call; owners, mean_partners, lanes as the plan states them
  device_s     one Context.window_pair_sums call per run: the host's operand checks, the uploads, the kernel, the download of both arrays
  table_ms     device events around the table arm's kernel, per run (the default arm at this number of cells)
  search_ms    the same matrix with NATAC_COACCESS_TABLE_MAX=1: the search arm's kernel, per run; same_bytes: both arms agree
  ref_s        tests/coaccess_ref.pair_sums_sparse (scipy.sparse int64 products) on the first --ref-owners owners, ref_pairs pairs;
               ref_equal: the device's two arrays equal it there
usage: python tools/bench_coaccess.py [--cells 10000] [--windows 100000] [--entries 3100000] [--open-rows 1000] [--chroms 4]
                                      [--spacing 2000] [--max-distance 250000] [--runs 3] [--ref-owners 2000] [--no-ref]"""
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
    ap.add_argument("--cells", type=int, default=10_000)
    ap.add_argument("--windows", type=int, default=100_000)
    ap.add_argument("--entries", type=int, default=3_100_000)
    ap.add_argument("--open-rows", type=int, default=1000)
    ap.add_argument("--chroms", type=int, default=4)
    ap.add_argument("--spacing", type=int, default=2000)
    ap.add_argument("--max-distance", type=int, default=250_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ref-owners", type=int, default=2000)
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    import scipy.sparse as sp
    from nucleoatac_amd import get_context
    from nucleoatac_amd.device import window_pair_sums_plan
    from nucleoatac_amd.pyatac.get_coaccess import pair_lists
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
    per = (a.windows + a.chroms - 1) // a.chroms
    chrom = np.array(["chr%d" % (w // per + 1) for w in range(a.windows)])
    start = (np.arange(a.windows, dtype=np.int64) % per) * a.spacing
    order, hi = pair_lists(chrom, start, start + 500, np.ones(a.windows, bool), a.max_distance)
    t_gen = time.perf_counter() - t0
    k = len(order)
    n_part = hi - np.arange(k) - 1
    ctx = get_context()
    t0 = time.perf_counter()
    ctx.window_pair_sums([0, 1, 2], [0, 0], [1, 1], 1, [0, 1], [2, 2])
    t_warm = time.perf_counter() - t0
    row_len = np.diff(ip)
    os.environ.pop("NATAC_COACCESS_TABLE_MAX", None)
    plan = window_pair_sums_plan(a.windows, a.cells, int(ip[-1]), k, int(row_len[order].sum()), ctx.device_info()["n_cu"])
    out = dict(tool="bench_coaccess", device=ctx.device_info()["name"], cells=a.cells, windows=a.windows, nnz=int(ip[-1]), chroms=a.chroms,
               max_distance=a.max_distance, longest_row=int(row_len.max()), mean_row=round(float(row_len.mean()), 2), owners=k,
               pairs=int(n_part.sum()), mean_partners=round(float(n_part.mean()), 2), lanes=plan["lanes"], default_arm=plan["arm"],
               gen_s=round(t_gen, 3), warmup_s=round(t_warm, 3))
    res = {}
    for name, forced in (("table", None), ("search", "1")):
        if forced is None:
            os.environ.pop("NATAC_COACCESS_TABLE_MAX", None)
        else:
            os.environ["NATAC_COACCESS_TABLE_MAX"] = forced
        runs = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            got = ctx.window_pair_sums(ip, ix, da, a.cells, order, hi, with_arm_owners=True, with_kernel_ms=True)
            runs.append(dict(device_s=round(time.perf_counter() - t0, 4), kernel_ms=round(got[3], 3)))
        res[name] = got
        out[name + "_ms"] = [r["kernel_ms"] for r in runs]
        out[name + "_device_s"] = [r["device_s"] for r in runs]
        out[name + "_arm_owners"] = got[2].tolist()
    os.environ.pop("NATAC_COACCESS_TABLE_MAX", None)
    out["same_bytes"] = all(x.tobytes() == y.tobytes() for x, y in zip(res["table"][:2], res["search"][:2]))
    if not a.no_ref:
        import coaccess_ref
        n_own = min(a.ref_owners, k)
        end = int(hi[:n_own].max())
        h = np.concatenate([hi[:n_own], np.arange(n_own + 1, end + 1)])               # the partners past the subset own nothing
        t0 = time.perf_counter()
        want = coaccess_ref.pair_sums_sparse(ip, ix, da, a.cells, order[:end], h)
        out["ref_s"] = round(time.perf_counter() - t0, 3)
        out["ref_owners"], out["ref_pairs"] = n_own, len(want[0])
        out["ref_equal"] = bool(all(np.array_equal(x[:len(y)], y) for x, y in zip(res["table"][:2], want)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
