"""Wall time by phase of genome-wide `pyatac ins` and `pyatac cov` (nucleoatac_amd/pyatac/get_ins.py, get_cov.py) on a synthetic workload:
a coordinate-sorted BAM of N paired-end records (tools/bench_bam.py's generator; half are forward proper pairs, so N = 21 M gives
~10.5 M fragments) on 4 x 50 Mbp chromosomes, cut into the reference's 1-kb chunks.  Prints one JSON line per command:
  decode_s    BAM -> FragmentStore (FragmentStore.from_bam), once for all commands
  pack_s      natac_pack_chunks of every sub-batch (host, on the prefetch threads: it overlaps the device work)
  device_s    upload + the track kernel + synchronisation, summed over the sub-batches
  kernel_ms   the track kernel alone (profile(): insertions / ins_smooth / center_cov)
  writer_s    device bedGraph + BGZF formatting, the copy of the members to the host, the file writes and the .tbi
  wall_s      the command end to end with the BAM already decoded; mbp_per_s = genome bases / wall_s
usage: python tools/bench_tracks.py [--records 21000000] [--out DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = {"ins": "insertions", "ins_smooth": "ins_smooth", "cov": "center_cov"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=21_000_000)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--ref-len", type=int, default=50_000_000)
    ap.add_argument("--out", default=None, help="directory for the synthetic inputs and outputs (default: a temporary one)")
    a = ap.parse_args()
    import bench_bam
    bench_bam.ThreadPoolExecutor = lambda n: ThreadPoolExecutor(min(int(n or 4), 16))     # 16 CPUs per job
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.get_cov import get_cov
    from nucleoatac_amd.pyatac.get_ins import get_ins
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    d = a.out or tempfile.mkdtemp(prefix="bench_tracks_")
    os.makedirs(d, exist_ok=True)
    bam = os.path.join(d, "synth.bam")
    t0 = time.perf_counter()
    bench_bam.synth_bam(bam, a.records, n_refs=a.refs, ref_len=a.ref_len)
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    t0 = time.perf_counter()
    st = FragmentStore.from_bam(bam)
    decode_s = time.perf_counter() - t0
    FragmentStore.register(bam, st)
    n_frags = sum(len(st.pos[c]) for c in st.references)
    genome_bp = sum(st.chrom_sizes().values())
    base = dict(cores=1, bed=None, lower=0, upper=2000, atac=True)
    runs = [("ins", get_ins, dict(smooth=None)), ("ins_smooth", get_ins, dict(smooth=75)), ("cov", get_cov, dict(window=121, scale=10.0))]
    ctx.profile_enable(True)
    for name, fn, extra in runs:
        args = argparse.Namespace(bam=bam, out=os.path.join(d, "warm_" + name), **base, **extra)
        bed = os.path.join(d, "warm.bed")
        with open(bed, "w") as f:
            f.write("%s\t0\t5000\n" % st.references[0])
        args.bed = bed
        fn(args)                                    # warm-up: code objects, the kernels' first launch
        ctx.profile_reset()
        args = argparse.Namespace(bam=bam, out=os.path.join(d, name), **base, **extra)
        tm = {}
        t0 = time.perf_counter()
        fn(args, timing=tm)
        wall_s = time.perf_counter() - t0
        kernel_ms = ctx.profile()[KERNEL[name]][0]
        out = args.out + (".cov" if name == "cov" else ".ins") + ".bedgraph.gz"
        print(json.dumps(dict(
            tool="bench_tracks", command=name, device=ctx.device_info()["name"], records=a.records, fragments=int(n_frags),
            genome_bp=int(genome_bp), options=extra, sub_batches=int(tm["sub_batches"]), generate_inputs_s=round(t_gen, 2),
            decode_s=round(decode_s, 3), pack_s=round(tm["pack_s"], 3), device_s=round(tm["device_s"], 3), kernel_ms=round(kernel_ms, 3),
            writer_s=round(tm["writer_s"], 3), wall_s=round(wall_s, 3), mbp_per_s=round(genome_bp / wall_s / 1e6, 1),
            output_bytes=os.path.getsize(out))), flush=True)
    ctx.profile_enable(False)


if __name__ == "__main__":
    main()
