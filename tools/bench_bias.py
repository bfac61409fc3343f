"""Wall time by phase of a genome-wide `pyatac bias` (nucleoatac_amd/pyatac/make_bias_track.py) on a synthetic genome (4 x 50 Mbp, 2 % N,
the built-in Human PWM), and the new kernel against the one it could have reused.  Prints two JSON lines.

  tool = bench_bias_kernel   natac_pwm_track (one 4.5 Mbp sub-batch of 1-kb chunks, profile slot pwm_track) against natac_pwm_score on the
                             same bases in the same process (Context.pwm_bias between timer_start / timer_stop: its upload, kernel and
                             8-byte-per-base download): the median of --reps launches after a warm-up, with the minimum and maximum.
                             natac_pwm_score has no profile slot: for its kernel time alone run this tool under
                             `rocprofv3 --kernel-trace` (e.g. with --refs 1 --ref-len 6000000) and compare the two kernels there
  tool = bench_bias          fasta_s    the FASTA (.npz) load
                             pack_s     the sequence windows of every sub-batch (host, on the prefetch threads)
                             device_s   upload + natac_pwm_track + synchronisation, summed over the sub-batches
                             kernel_ms  natac_pwm_track alone, summed (profile slot)
                             writer_s   device bedGraph + BGZF formatting, the copy of the members, the file writes and the .tbi
                             wall_s     the command end to end; mbp_per_s = genome bases / wall_s
usage: python tools/bench_bias.py [--refs 4] [--ref-len 50000000] [--reps 20] [--out DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_comparison(ctx, fs, pwm, reps):
    """one sub-batch of 1-kb chunks through natac_pwm_track (event time of the kernel alone), and the same bases as one sequence through
    natac_pwm_bias (stream timer around the whole call: natac_pwm_score is not in a profile slot)"""
    from nucleoatac_amd import _lib as L
    from nucleoatac_amd.pipeline import SUB_BATCH_BP
    from nucleoatac_amd.pyatac.chunk import Chunk
    from nucleoatac_amd.pyatac.make_bias_track import pack_seq_windows
    c = fs.references[0]
    n = min(SUB_BATCH_BP, len(fs.seqs[c]) - pwm.up - pwm.down)
    n -= n % 1000
    sub = [Chunk(c, pwm.up + i, pwm.up + i + 1000) for i in range(0, n, 1000)]
    pk = pack_seq_windows(sub, fs, pwm.up, pwm.down)
    logp = np.log(pwm.mat)
    nucs = np.frombuffer("".join(pwm.nucleotides).encode("ascii"), dtype=np.uint8)
    seq = fs.seqs[c][:n + pwm.up + pwm.down]
    b = ctx.upload(pk)
    track_ms, call_ms, score_ms = [], [], []
    try:
        for r in range(reps + 3):
            ctx.profile_reset()
            t0 = time.perf_counter()
            b.run_pwm_track(pk.track_seq_off, pk.track_seq, logp, nucs)
            ctx.sync()
            dt = (time.perf_counter() - t0) * 1e3
            ms = ctx.profile()["pwm_track"][0]
            ctx.timer_start()
            ref = ctx.pwm_bias(seq, pwm.mat, pwm.nucleotides)
            sms = ctx.timer_stop()
            if r >= 3:
                track_ms.append(ms)
                call_ms.append(dt)
                score_ms.append(sms)
        got = b.track(L.T_BIAS)
    finally:
        b.free()
    assert np.array_equal(got, ref)
    q = lambda v: dict(median=round(float(np.median(v)), 4), min=round(float(np.min(v)), 4), max=round(float(np.max(v)), 4))
    return dict(bases=int(n), chunks=len(sub), reps=reps, pwm_track_kernel_ms=q(track_ms), pwm_track_call_ms=q(call_ms),
                pwm_bias_call_ms=q(score_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="directory for the synthetic inputs and outputs (default: a temporary one)")
    a = ap.parse_args()
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.bias import PWM
    from nucleoatac_amd.pyatac.make_bias_track import make_bias_track
    from nucleoatac_amd.pyatac.seq import FastaStore
    d = a.out or tempfile.mkdtemp(prefix="bench_bias_")
    os.makedirs(d, exist_ok=True)
    t0 = time.perf_counter()
    rng = np.random.default_rng(1)
    fa = os.path.join(d, "synth.fa.npz")
    names = ["chr%d" % (r + 1) for r in range(a.refs)]
    np.savez(fa, chrom_names=np.array(names), chrom_lengths=np.array([a.ref_len] * a.refs),
             **{"seq_" + c: rng.choice(np.frombuffer(b"ACGTN", np.uint8), a.ref_len, p=[0.29, 0.2, 0.2, 0.29, 0.02]) for c in names})
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    pwm = PWM.open("Human")
    t0 = time.perf_counter()
    fs = FastaStore.open(fa)
    fasta_s = time.perf_counter() - t0
    ctx.profile_enable(True)
    bed = os.path.join(d, "warm.bed")
    with open(bed, "w") as f:
        f.write("%s\t0\t5000\n" % names[0])
    make_bias_track(argparse.Namespace(fasta=fa, pwm="Human", bed=bed, out=os.path.join(d, "warm"), cores=1))   # code objects, first launches
    print(json.dumps(dict(tool="bench_bias_kernel", device=ctx.device_info()["name"], **kernel_comparison(ctx, fs, pwm, a.reps))), flush=True)
    ctx.profile_reset()
    args = argparse.Namespace(fasta=fa, pwm="Human", bed=None, out=os.path.join(d, "bias"), cores=1)
    tm = {}
    t0 = time.perf_counter()
    path = make_bias_track(args, timing=tm)
    wall_s = time.perf_counter() - t0
    kernel_ms, launches = ctx.profile()["pwm_track"]
    ctx.profile_enable(False)
    genome_bp = a.refs * a.ref_len
    print(json.dumps(dict(
        tool="bench_bias", device=ctx.device_info()["name"], genome_bp=genome_bp, pwm="Human", sub_batches=int(tm["sub_batches"]),
        generate_inputs_s=round(t_gen, 2), fasta_s=round(fasta_s, 3), pack_s=round(tm["pack_s"], 3), device_s=round(tm["device_s"], 3),
        kernel_ms=round(kernel_ms, 3), kernel_launches=int(launches), writer_s=round(tm["writer_s"], 3), wall_s=round(wall_s, 3),
        mbp_per_s=round(genome_bp / wall_s / 1e6, 1), output_bytes=os.path.getsize(path))), flush=True)


if __name__ == "__main__":
    main()
