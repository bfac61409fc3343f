"""Time of Context.knn (natac_knn, nucleoatac_amd/csrc/natac_knn.hpp) at the size `pyatac doublets` gives it: --real + --sim unit rows in
--dim dimensions, k = --k, the queries the first --real rows with themselves excluded.  One box, one process, --runs runs after a warm-up
call.  Prints one JSON line per measurement.

  call_s      per run: the whole call (value checks, uploads, kernel, downloads)
  kernel_ms   per run: the kernel on the stream (device events)
  clock_mhz   the shader clock while the same call runs once more under the context's clock sampler (Context.clock_trace_start):
              [median, highest] of its samples; the samples between the kernel and the copies are in it, so the highest is the one used
  vector_share  the best run's 3 x pairs x dim fp64 operations (a subtraction, a multiplication, an addition per pair and dimension, none
              fused) over kernel time, against n_cu x 4 SIMDs x 16 lanes x the highest sampled clock (null when the sampler gave nothing)
  plan        device.knn_plan for the call
--also-k64 repeats at k = 64 under the wave arm and, with NATAC_KNN_WAVE_K_MAX=1, under the lds arm, and asserts the same bytes.
--sweep-tiles repeats the main size under every NATAC_KNN_QUERY_TILE and asserts the same bytes.
--ref-queries N times the NumPy restatement of tests/knn_ref.py on the first N queries and asserts equality there.
usage: python tools/bench_knn.py [--real 10000] [--sim 20000] [--dim 30] [--k 150] [--runs 3] [--ref-queries 200] [--also-k64] [--sweep-tiles]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _clock(ctx, call):
    """[median, highest] MHz of the shader clock sampled while call() runs, or None"""
    try:
        ctx.clock_trace_start(max_samples=40000, interval_us=50)
        call()
        ctx.sync()
        ghz = ctx.clock_trace_stop()["ghz"]
    except Exception as e:           # the figure is optional: the times stand without it
        sys.stderr.write("bench_knn: no clock samples (%s)\n" % e)
        return None
    ghz = ghz[np.isfinite(ghz)]
    return [round(float(np.median(ghz)) * 1e3, 1), round(float(ghz.max()) * 1e3, 1)] if len(ghz) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--real", type=int, default=10_000)
    ap.add_argument("--sim", type=int, default=20_000)
    ap.add_argument("--dim", type=int, default=30)
    ap.add_argument("--k", type=int, default=150)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ref-queries", type=int, default=200)
    ap.add_argument("--also-k64", action="store_true")
    ap.add_argument("--sweep-tiles", action="store_true")
    a = ap.parse_args()
    import knn_ref as R
    from nucleoatac_amd import get_context
    from nucleoatac_amd.device import knn_plan
    rng = np.random.default_rng(1)
    P = rng.standard_normal((a.real + a.sim, a.dim))
    P /= np.sqrt((P * P).sum(axis=1))[:, None]
    Q = P[:a.real]
    ctx = get_context()
    dev, n_cu = ctx.device_info()["name"], ctx.device_info()["n_cu"]
    ctx.knn(P[:300], 5)                      # warm-up: code objects
    ctx.knn(P[:300], 70)

    def runs(k):
        call_s, ker_ms = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            idx, d2, arms, ms = ctx.knn(P, k, queries=Q, self_offset=0, with_arm_queries=True, with_kernel_ms=True)
            call_s.append(round(time.perf_counter() - t0, 4))
            ker_ms.append(round(ms, 3))
        mhz = _clock(ctx, lambda: ctx.knn(P, k, queries=Q, self_offset=0))
        ops = 3.0 * a.real * (a.real + a.sim) * a.dim
        share = round(ops / (min(ker_ms) * 1e-3) / (n_cu * 4 * 16 * mhz[1] * 1e6), 4) if mhz else None
        return (idx, d2), dict(k=k, call_s=call_s, kernel_ms=ker_ms, arm="wave" if arms[0] else "lds", clock_mhz=mhz, vector_share=share,
                               plan=knn_plan(a.real, a.real + a.sim, a.dim, k, n_cu=n_cu))

    head = dict(tool="bench_knn", device=dev, n_cu=n_cu, real=a.real, sim=a.sim, dim=a.dim)
    got, out = runs(a.k)
    if a.ref_queries > 0:
        n = min(a.ref_queries, a.real)
        t0 = time.perf_counter()
        want = R.knn(P, a.k, queries=Q[:n], self_offset=0)
        equal = R.same((got[0][:n], got[1][:n]), want)
        out.update(ref_queries=n, ref_s=round(time.perf_counter() - t0, 3), equal=bool(equal))
        assert equal, "the restatement's rows differ from the device's"
    print(json.dumps(dict(head, **out)), flush=True)
    if a.sweep_tiles:
        for qt in (4, 8, 16, 32):
            os.environ["NATAC_KNN_QUERY_TILE"] = str(qt)
            g2, o2 = runs(a.k)
            same = R.same(g2, got)
            print(json.dumps(dict(head, forced_query_tile=qt, same_bytes=bool(same), **o2)), flush=True)
            assert same, "NATAC_KNN_QUERY_TILE=%d changed the result" % qt
        del os.environ["NATAC_KNN_QUERY_TILE"]
    if a.also_k64:
        gw, ow = runs(64)
        print(json.dumps(dict(head, **ow)), flush=True)
        os.environ["NATAC_KNN_WAVE_K_MAX"] = "1"
        gl, ol = runs(64)
        del os.environ["NATAC_KNN_WAVE_K_MAX"]
        same = R.same(gw, gl)
        print(json.dumps(dict(head, wave_k_max=1, same_bytes=bool(same), **ol)), flush=True)
        assert same, "NATAC_KNN_WAVE_K_MAX=1 changed the result"


if __name__ == "__main__":
    main()
