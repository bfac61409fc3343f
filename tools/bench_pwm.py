"""Wall time by phase of a genome-wide `pyatac pwm` (nucleoatac_amd/pyatac/get_pwm.py) on a synthetic workload: a coordinate-sorted BAM
of N paired-end records (tools/bench_bam.py's generator; half are forward proper pairs, so N = 21 M gives ~10.5 M fragments) on a
random 4 x 50 Mbp genome.  Prints one JSON line:
  decode_s      BAM -> FragmentStore (FragmentStore.from_bam)
  pack_s        natac_pack_chunks + the sequence windows of every sub-batch (host)
  upload_s      the device calls minus their kernels: host -> device copies, the 4K-entry result copy, synchronisation
  kernel_ms     natac_ins_seq_counts, summed over the sub-batches (device events)
  background_s  getNucFreqs (natac_base_counts over the genome, including its upload)
  finish_s      normalise + symmetrise + write the .PWM.txt (host)
  pwm_wall_s    the whole driver once more with the BAM already decoded (its packing overlaps the device calls)
usage: python tools/bench_pwm.py [--records 21000000] [--flank 10] [--out DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=21_000_000)
    ap.add_argument("--flank", type=int, default=10)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    ap.add_argument("--out", default=None, help="directory for the synthetic inputs (default: a temporary one)")
    a = ap.parse_args()
    import bench_bam
    bench_bam.ThreadPoolExecutor = lambda n: ThreadPoolExecutor(min(int(n or 4), 16))     # 16 CPUs per job
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac import get_pwm as GP
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.seq import ACGT, getNucFreqs
    d = a.out or tempfile.mkdtemp(prefix="bench_pwm_")
    os.makedirs(d, exist_ok=True)
    bam = os.path.join(d, "synth.bam")
    t0 = time.perf_counter()
    bench_bam.synth_bam(bam, a.records, n_refs=a.refs, ref_len=a.ref_len)
    rng = np.random.default_rng(1)
    fa = os.path.join(d, "synth.fa.npz")
    names = ["chr%d" % (r + 1) for r in range(a.refs)]
    np.savez(fa, chrom_names=np.array(names), chrom_lengths=np.array([a.ref_len] * a.refs),
             **{"seq_" + c: rng.choice(np.frombuffer(b"ACGTN", np.uint8), a.ref_len, p=[0.29, 0.2, 0.2, 0.29, 0.02]) for c in names})
    t_gen = time.perf_counter() - t0

    ctx = get_context()
    t0 = time.perf_counter()
    st = FragmentStore.from_bam(bam)
    decode_s = time.perf_counter() - t0
    FragmentStore.register(bam, st)
    n_frags = sum(len(st.pos[c]) for c in st.references)
    chrs = {c: a.ref_len for c in names}
    chunks = GP.genome_regions(chrs, a.flank)
    GP.count_windows(chunks[:1], bam, fa, a.flank, prefetch=False)          # warm-up: code objects, the FASTA load
    tm = {}
    t0 = time.perf_counter()
    M, n = GP.count_windows(chunks, bam, fa, a.flank, timing=tm, prefetch=False)
    count_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    freqs = getNucFreqs(fa, ACGT)
    background_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    res = GP.finish_pwm(M, n, freqs, a.flank, True)
    from nucleoatac_amd.pyatac.bias import PWM
    PWM(res, a.flank, a.flank, list(ACGT)).save(os.path.join(d, "phases.PWM.txt"), py2_floats=True)
    finish_s = time.perf_counter() - t0
    args = argparse.Namespace(bam=bam, fasta=fa, bed=None, flank=a.flank, lower=0, upper=2000, atac=True, sym=True, dinucleotide=False,
                              cores=1, out=os.path.join(d, "wall"))
    t0 = time.perf_counter()
    res2 = GP.get_pwm(args)
    pwm_wall_s = time.perf_counter() - t0
    assert np.array_equal(res, res2)
    print(json.dumps(dict(
        tool="bench_pwm", device=ctx.device_info()["name"], records=a.records, fragments=int(n_frags), insertions=int(n),
        genome_bp=a.refs * a.ref_len, flank=a.flank, sub_batches=int(tm["sub_batches"]), generate_inputs_s=round(t_gen, 2), decode_s=round(decode_s, 3),
        pack_s=round(tm["pack_s"], 3), upload_s=round(tm["device_s"] - tm["kernel_ms"] / 1e3, 3), kernel_ms=round(tm["kernel_ms"], 3),
        count_phase_wall_s=round(count_s, 3), background_s=round(background_s, 3), finish_s=round(finish_s, 4),
        pwm_wall_s=round(pwm_wall_s, 3))))


if __name__ == "__main__":
    main()
