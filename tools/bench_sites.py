"""Wall time by phase of `pyatac counts` and `pyatac nucleotide` (nucleoatac_amd/pyatac/get_counts.py, get_nucleotide.py) end to end on a
synthetic workload, kernel milliseconds against wall time, and the NumPy restatement of tests/sites_ref.py on the same inputs as the
point of comparison.  Prints one JSON line per tool.

The workload: a fragment store at the density of the configs[2] benchmark (50 M fragments over --refs x --ref-len bases, 500 per
2,120 bases), registered in memory (the BAM decode is tools/bench_bam.py's number); --windows windows of 500 bases for `counts`; a
random genome of the same size, saved as a FastaStore .npz, and --sites sites with a strand column for `nucleotide` at the default
+-250, mono and --dinucleotide.

  tool = bench_counts      bed_s      reading the BED into columns (host)
                           device_s   the natac_region_counts calls: upload of each chromosome's records and regions, kernels, download
                           kernel_ms  the range search and the two counting kernels alone (device events), summed over the chromosomes
                           text_s     formatting and gzip of the .counts.txt.gz (host)
                           wall_s     the command end to end; numpy_s the restatement's counting alone (no BED, no text)
  tool = bench_nucleotide  bed_s, fasta_s (the .npz load), device_s, kernel_ms, text_s, wall_s and numpy_s likewise, for word = 1 and 2
usage: python tools/bench_sites.py [--fragments 50000000] [--windows 1000000] [--sites 1000000] [--refs 4] [--ref-len 53000000]
                                   [--no-numpy] [--out DIR]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fragments", type=int, default=50_000_000)
    ap.add_argument("--windows", type=int, default=1_000_000)
    ap.add_argument("--sites", type=int, default=1_000_000)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--ref-len", type=int, default=53_000_000)
    ap.add_argument("--no-numpy", action="store_true", help="skip the NumPy restatement (minutes at the default sizes)")
    ap.add_argument("--out", default=None, help="directory for the synthetic inputs (default: a temporary one)")
    a = ap.parse_args()
    import sites_ref as R
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.chunk import read_bed_columns
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.get_counts import get_counts
    from nucleoatac_amd.pyatac.get_nucleotide import get_nucleotide, site_centers
    from nucleoatac_amd.pyatac.seq import FastaStore
    d = a.out or tempfile.mkdtemp(prefix="bench_sites_")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(1)
    names = ["chr%d" % (r + 1) for r in range(a.refs)]
    t0 = time.perf_counter()
    per = a.fragments // a.refs
    pos = {c: np.sort(rng.integers(0, a.ref_len - 1000, size=per)) for c in names}
    tlen = {c: np.where(rng.random(per) < 0.6, rng.integers(38, 150, size=per), rng.integers(150, 700, size=per)) for c in names}
    st = FragmentStore(names, [a.ref_len] * a.refs, pos, tlen)
    bam = os.path.join(d, "synth_store.npz")
    FragmentStore.register(bam, st)
    windows = os.path.join(d, "windows.bed")
    with open(windows, "w") as f:
        c = rng.integers(0, a.refs, size=a.windows)
        s = rng.integers(0, a.ref_len - 500, size=a.windows)
        f.write("".join("%s\t%d\t%d\n" % (names[k], x, x + 500) for k, x in zip(c.tolist(), s.tolist())))
    fasta = os.path.join(d, "synth.fa.npz")
    np.savez(fasta, chrom_names=np.array(names), chrom_lengths=np.array([a.ref_len] * a.refs),
             **{"seq_" + c: rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), a.ref_len, p=[0.22, 0.16, 0.16, 0.22, 0.06, 0.05, 0.05, 0.06, 0.02])
                for c in names})
    sites = os.path.join(d, "sites.bed")
    with open(sites, "w") as f:
        c = rng.integers(0, a.refs, size=a.sites)
        s = rng.integers(0, a.ref_len - 147, size=a.sites)
        m = rng.random(a.sites) < 0.5
        f.write("".join("%s\t%d\t%d\tn\t0\t%s\n" % (names[k], x, x + 147, "-" if y else "+") for k, x, y in zip(c.tolist(), s.tolist(), m.tolist())))
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    dev = ctx.device_info()["name"]
    ctx.region_counts(pos[names[0]][:1000], tlen[names[0]][:1000], [0], [10])                       # warm-up: code objects
    ctx.site_seq_counts(np.frombuffer(b"ACGT" * 300, np.uint8), [600], None, 250, 250, 2)

    tm = {}
    args = argparse.Namespace(bam=bam, bed=windows, out=os.path.join(d, "bench"), atac=True, lower=0, upper=500)
    t0 = time.perf_counter()
    counts = get_counts(args, timing=tm)
    wall = time.perf_counter() - t0
    numpy_s = None
    if not a.no_numpy:
        cn, cc, cs, ce, _ = read_bed_columns(windows)
        t0 = time.perf_counter()
        want = np.zeros(len(cs), np.int64)
        for k, c in enumerate(cn):
            idx = np.flatnonzero(cc == k)
            want[idx] = R.region_counts_ref(st.pos[c], st.tlen[c], cs[idx], ce[idx], 0, 500, 1)
        numpy_s = round(time.perf_counter() - t0, 2)
        assert np.array_equal(want, counts)
    print(json.dumps(dict(tool="bench_counts", device=dev, fragments=per * a.refs, windows=a.windows, counted=int(counts.sum()),
                          generate_inputs_s=round(t_gen, 1), bed_s=round(tm["bed_s"], 3), decode_s=round(tm["decode_s"], 3),
                          device_s=round(tm["device_s"], 3), kernel_ms=round(tm["kernel_ms"], 3), text_s=round(tm["text_s"], 3),
                          wall_s=round(wall, 3), numpy_s=numpy_s)), flush=True)

    for di in (False, True):
        tm = {}
        args = argparse.Namespace(fasta=fasta, bed=sites, dinucleotide=di, up=250, down=250, strand=6, out=os.path.join(d, "bench%d" % di),
                                  cores=1, norm=False)
        t0 = time.perf_counter()
        res = get_nucleotide(args, timing=tm)
        wall = time.perf_counter() - t0
        numpy_s = None
        if not a.no_numpy:
            fs = FastaStore.open_cased(fasta)
            cn, cc, cs, ce, cm = read_bed_columns(sites, strand_col=6)
            ctr = site_centers(cs, ce, cm)
            t0 = time.perf_counter()
            M, n = 0, 0
            for k, c in enumerate(cn):
                idx = np.flatnonzero(cc == k)
                m, u = R.site_counts_ref(fs.seqs[c], ctr[idx], cm[idx], 250, 250, 2 if di else 1)
                M, n = M + m, n + u
            numpy_s = round(time.perf_counter() - t0, 2)
            assert np.array_equal(np.asarray(M, np.float64) / float(n), res)
        print(json.dumps(dict(tool="bench_nucleotide", device=dev, word=2 if di else 1, sites=a.sites, columns=501,
                              genome_bp=a.refs * a.ref_len, bed_s=round(tm["bed_s"], 3), fasta_s=round(tm["fasta_s"], 3),
                              device_s=round(tm["device_s"], 3), kernel_ms=round(tm["kernel_ms"], 3), text_s=round(tm["text_s"], 4),
                              wall_s=round(wall, 3), numpy_s=numpy_s)), flush=True)


if __name__ == "__main__":
    main()
