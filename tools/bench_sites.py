"""Wall time by phase of `pyatac counts`, `pyatac nucleotide` and `pyatac signal` (nucleoatac_amd/pyatac/get_counts.py, get_nucleotide.py,
signal_around_sites.py) end to end on a synthetic workload, kernel milliseconds against wall time, and the NumPy restatement of
tests/sites_ref.py / tests/signal_ref.py on the same inputs as the point of comparison.  Prints one JSON line per tool.

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
  tool = bench_signal      (mode `signal`) `pyatac signal` on a synthetic bedGraph of --refs x --signal-ref-len bases in records of
                           1 to 19 bases with holes, bgzipped and indexed by the package's writers, and --signal-sites stranded sites
                           at +-250: bed_s, read_s (span merging and natac_tbx_read_regions), device_s (the natac_site_signal calls:
                           upload, kernels, download), kernel_ms, text_s and wall_s of get_signal without --all, for no transform and
                           for --exp --positive --scale; kernel_ms_matrix, the kernels of one natac_site_signal call over all sites
                           with the matrix written; floor_ms, n x K x 8 bytes read (and written, with the matrix) at 8 TB/s;
                           numpy_s, the restatement of tests/signal_ref.py on the same value buffer (rows and aggregate, no read)
usage: python tools/bench_sites.py [sites|signal] [--fragments 50000000] [--windows 1000000] [--sites 1000000] [--refs 4]
                                   [--ref-len 53000000] [--signal-sites 100000] [--signal-ref-len 2500000] [--no-numpy] [--out DIR]"""
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


def bench_signal(a):
    import signal_ref as R
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.chunk import read_bed_columns
    from nucleoatac_amd.pyatac.signal_around_sites import get_signal, merge_spans, site_windows
    from nucleoatac_amd.tabix import NativeTabix
    from nucleoatac_amd.writer import bgzip_file, tabix_index
    d = a.out or tempfile.mkdtemp(prefix="bench_signal_")
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(2)
    names = ["chr%d" % (r + 1) for r in range(a.refs)]
    L, K = a.signal_ref_len, 501
    t0 = time.perf_counter()
    plain = os.path.join(d, "track.bedgraph")
    n_records = 0
    with open(plain, "w") as f:
        for c in names:
            edges = np.cumsum(rng.integers(1, 20, size=L // 9))
            edges = edges[edges < L]
            b, e = edges[:-1], edges[1:]
            keep = rng.random(len(b)) > 0.03                        # holes: NaN
            v = np.round(rng.normal(0.2, 1.0, len(b)), 4)
            f.write("".join("%s\t%d\t%d\t%s\n" % (c, x, y, repr(z)) for x, y, z in zip(b[keep].tolist(), e[keep].tolist(), v[keep].tolist())))
            n_records += int(keep.sum())
    bg = bgzip_file(plain)
    tabix_index(bg)
    sizes = os.path.join(d, "genome.sizes")
    with open(sizes, "w") as f:
        f.write("".join("%s\t%d\n" % (c, L) for c in names))
    sites = os.path.join(d, "signal_sites.bed")
    with open(sites, "w") as f:
        c = rng.integers(0, a.refs, size=a.signal_sites)
        s = rng.integers(0, L - 147, size=a.signal_sites)
        m = rng.random(a.signal_sites) < 0.5
        f.write("".join("%s\t%d\t%d\tn\t0\t%s\n" % (names[k], x, x + 147, "-" if y else "+") for k, x, y in zip(c.tolist(), s.tolist(), m.tolist())))
    t_gen = time.perf_counter() - t0
    ctx = get_context()
    dev = ctx.device_info()["name"]
    for flags in (0, 7):                                            # warm-up: code objects
        ctx.site_signal(np.zeros(600), [0, 50], [501, 501], [0, 0], [0, 1], K, exp=bool(flags & 1), positive=bool(flags & 2),
                        scale=bool(flags & 4), want_matrix=True)
    cn, cc, cs, ce, cm = read_bed_columns(sites, strand_col=6)
    ws, we, lead, _ = site_windows(cn, cc, cs, ce, cm, {c: L for c in names}, 250, 250)
    sc, ss, se, off, src = merge_spans(cc, ws, we)
    tbx = NativeTabix(bg)
    vals, _ = tbx.read_regions([cn[k] for k in sc.tolist()], ss, se, empty=np.nan, value_col=4)
    tbx.close()
    length = (we - ws).astype(np.int32)
    n = len(cs)
    for flags in (0, 7):
        kw = dict(exp=bool(flags & 1), positive=bool(flags & 2), scale=bool(flags & 4))
        tm = {}
        args = argparse.Namespace(bed=sites, bg=bg, sizes=sizes, out=os.path.join(d, "bench_signal%d" % flags), cores=1, all=False,
                                  no_agg=False, up=250, down=250, weight=None, strand=6, norm=False, **kw)
        t0 = time.perf_counter()
        agg, _ = get_signal(args, timing=tm)
        wall = time.perf_counter() - t0
        ms_mat = min(ctx.site_signal(vals, src, length, lead, cm, K, want_matrix=True, with_kernel_ms=True, **kw)[2] for _ in range(3))
        ms_agg = min(ctx.site_signal(vals, src, length, lead, cm, K, want_matrix=False, with_kernel_ms=True, **kw)[2] for _ in range(3))
        numpy_s = None
        if not a.no_numpy:
            t0 = time.perf_counter()
            want, mag = np.zeros(K), np.zeros(K)
            for i in range(0, n, 8192):
                m = R.rows_ref_fast(vals, src[i:i + 8192], length[i:i + 8192], lead[i:i + 8192], cm[i:i + 8192], K, flags)
                want += R.aggregate(m)
                mag += np.nansum(np.abs(m), axis=0)
            numpy_s = round(time.perf_counter() - t0, 2)
            assert np.all(np.abs(agg - want) <= (2 * n + K + 4) * 2.0 ** -52 * mag)
        print(json.dumps(dict(tool="bench_signal", device=dev, flags=flags, sites=n, columns=K, track_records=n_records,
                              values_read=int(off[-1]), generate_inputs_s=round(t_gen, 1), bed_s=round(tm["bed_s"], 3),
                              read_s=round(tm["read_s"], 3), device_s=round(tm["device_s"], 3), kernel_ms=round(tm["kernel_ms"], 3),
                              kernel_ms_aggregate_only=round(ms_agg, 3), kernel_ms_matrix=round(ms_mat, 3),
                              floor_ms_aggregate_only=round(n * K * 8 / 8e12 * 1e3, 4), floor_ms_matrix=round(2 * n * K * 8 / 8e12 * 1e3, 4),
                              text_s=round(tm["text_s"], 4), wall_s=round(wall, 3), numpy_s=numpy_s)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="sites", choices=["sites", "signal"],
                    help="sites: counts and nucleotide (the default); signal: pyatac signal")
    ap.add_argument("--signal-sites", type=int, default=100_000)
    ap.add_argument("--signal-ref-len", type=int, default=2_500_000)
    ap.add_argument("--fragments", type=int, default=50_000_000)
    ap.add_argument("--windows", type=int, default=1_000_000)
    ap.add_argument("--sites", type=int, default=1_000_000)
    ap.add_argument("--refs", type=int, default=4)
    ap.add_argument("--ref-len", type=int, default=53_000_000)
    ap.add_argument("--no-numpy", action="store_true", help="skip the NumPy restatement (minutes at the default sizes)")
    ap.add_argument("--out", default=None, help="directory for the synthetic inputs (default: a temporary one)")
    a = ap.parse_args()
    if a.mode == "signal":
        return bench_signal(a)
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
