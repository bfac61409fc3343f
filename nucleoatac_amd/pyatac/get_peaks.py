"""`pyatac peaks`: enriched regions (peaks) of a fragment store.  This command is this package's own, like `cells`, `cellqc`, `split` and
`cellcounts`: the reference has no peak caller, and every command here that does real work wants a peak set (`nucleoatac run/occ/nuc
--bed`, `pyatac counts --bed`, `cellqc --peaks`, `cellcounts --bed`).  In the single-cell order it is the last link: `cells` -> `cellqc`
-> `split` -> `peaks` per group -> `nucleoatac run --bed`.

The rule, per chromosome of length n (include/natac.h).  Every record gives two insertions, l = pos + 4 and r = pos + tlen - 5, without a
size filter; one outside [0, n) is dropped on its own.  C_w(x) is the number of insertions within w bases of x (the window clipped at the
chromosome's ends, its width for rates always the nominal 2w + 1).  p = C_h (--half_width), s = C_S (--small), g = C_L (--large),
1 <= h <= S <= L <= 50000.

Host, once: with P = 10^-q (q = --mlog10p), Lam[0] = 0 and Lam[k] = gammaincinv(k, P) for 1 <= k < 65536, the largest rate at which a
Poisson count reaches k with probability at most P; thr_small[k] = floor(Lam[k] (2S + 1) / (2h + 1)), thr_large[k] likewise with L, both
int32; min_pileup = max(1, the smallest k with Lam[k] >= lam_g), lam_g = (2h + 1) N / G with N the insertions kept over all chromosomes
and G the sum of the chromosome lengths.  These tables and min_pileup are all the device sees of the statistics.

Device (natac_enriched_regions, csrc/natac_peakcall.hpp), integers only, one call per chromosome with records: base x is significant when
p(x) >= min_pileup, s(x) <= thr_small[k] and g(x) <= thr_large[k], k = min(p(x), 65535) -- the pileup is improbable at the largest of the
genome-wide, the 1-kb and the 10-kb local rate.  Significant bases with at most --max_gap others between them are one region [first,
last + 1); one shorter than --min_length is dropped.  summit = (a + b) // 2, a / b the first / last base where p is largest in the region.

Host, per region: lam = (2h + 1) max(N / G, s / (2S + 1), g / (2L + 1)) at the summit, mlog10p = -poisson.logsf(p - 1, lam) / ln 10,
fold = p / lam.  --fixed_width W: every region gives [summit - W // 2, summit - W // 2 + W); one that leaves [0, n) is dropped; the rest are
ranked by (mlog10p descending, p descending, chromosome index, start) and kept greedily when they overlap no interval kept before on
that chromosome: the disjoint set `cellcounts --bed` and `nucleoatac run --bed` want, written in coordinate order.

BASE.peaks.narrowPeak   chrom start end name score . fold mlog10p -1 summit-start; name = <BASE's file name>_peak_<i> from 1 in file order,
                        score = min(1000, int(10 * mlog10p)), fold %.4f, mlog10p %.2f; an infinite mlog10p (the tail probability
                        underflows a double, past about 323) is written as 1000.00 (MLOG10P_INF);
BASE.peaks.fixed.bed    with --fixed_width: chrom start end;
BASE.peaks.txt          records, insertions_kept, insertions_dropped, genome_length, lam_g, min_pileup, significant_bases, regions_found,
                        regions_kept, fixed_width_kept (NA without --fixed_width).
Everything is computed before the first file is written, so an error leaves nothing behind; "no region" is not an error.

Measured on the MI355X box (tools/bench_peaks.py, one box, one process, three runs after a warm-up call: 10 M fragments on 4 chromosomes
of 50 Mbp, 10,000 planted hotspots, default geometry, 9,754 regions): the four device calls 0.040 s in the first run and 0.025 s in the
next two (the host's operand checks, upload and download included; 11.1 ms between their first and last kernel); the same regions through
the NumPy restatement of tests/peaks_ref.py on that box 6.1 s, and equal.
"""
import argparse
import os
import time

import numpy as np

K_TABLE = 65536
MLOG10P_INF = 1000.0        # what an infinite mlog10p is written as: above every finite value (-log10 of the smallest double is 323.3)
INT32_TOP = 2 ** 31 - 1     # table entries are clipped to it: no count reaches it (a call takes fewer than 2^30 records)


class PeaksError(ValueError):
    """`pyatac peaks` cannot answer: arguments that break a rule, a missing file, a store without records"""


def check_args(args):
    """the argument rules of the command -> PeaksError"""
    from .._lib import PEAKS_MAX_WINDOW
    if not 1 <= args.half_width <= args.small <= args.large <= PEAKS_MAX_WINDOW:
        raise PeaksError("1 <= --half_width (%d) <= --small (%d) <= --large (%d) <= %d must hold"
                         % (args.half_width, args.small, args.large, PEAKS_MAX_WINDOW))
    if not args.mlog10p > 0 or not np.isfinite(args.mlog10p):
        raise PeaksError("--mlog10p (%s) must be positive" % args.mlog10p)
    if args.max_gap < 0:
        raise PeaksError("--max_gap (%d) must not be negative" % args.max_gap)
    if args.min_length < 1:
        raise PeaksError("--min_length (%d) must be at least 1" % args.min_length)
    if args.fixed_width is not None and args.fixed_width < 1:
        raise PeaksError("--fixed_width (%d) must be at least 1" % args.fixed_width)


def critical_tables(half_width, small, large, mlog10p, n_table=K_TABLE):
    """(Lam float64[n_table], thr_small int32[n_table], thr_large int32[n_table])"""
    from scipy.special import gammaincinv
    lam = np.zeros(n_table, np.float64)
    lam[1:] = gammaincinv(np.arange(1, n_table, dtype=np.float64), 10.0 ** -float(mlog10p))
    w = float(2 * half_width + 1)
    return (lam, np.minimum(np.floor(lam * (2 * small + 1) / w), INT32_TOP).astype(np.int32),
            np.minimum(np.floor(lam * (2 * large + 1) / w), INT32_TOP).astype(np.int32))


def min_pileup_for(lam, lam_g):
    """max(1, the smallest k with Lam[k] >= lam_g) -> PeaksError when the table has no such k"""
    k = int(np.searchsorted(lam, lam_g, "left"))
    if k >= len(lam):
        raise PeaksError("the genome-wide rate (%.6g insertions per pileup window) is beyond the critical-value table (%d entries)"
                         % (lam_g, len(lam)))
    return max(1, k)


def device_regions(pos, tlen, n, h, S, L, max_gap, min_length, min_pile, thr_small, thr_large, timing=None):
    """one natac_enriched_regions call -> (start, end, summit, pileup, n_small, n_large, regions found, significant bases)"""
    from .. import get_context
    t0 = time.perf_counter()
    out = get_context().enriched_regions(pos, tlen, n, thr_small, thr_large, min_pile, h, S, L, max_gap, min_length, with_counts=True,
                                         with_kernel_ms=True)
    if timing is not None:
        timing["device_s"] = timing.get("device_s", 0.0) + time.perf_counter() - t0
        timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + out[8]
    return out[:8]


def score(pileup, n_small, n_large, half_width, small, large, rate):
    """(mlog10p, fold) per region; rate = N / G"""
    from scipy.stats import poisson
    p = np.asarray(pileup, np.float64)
    lam = (2 * half_width + 1) * np.maximum(np.maximum(np.asarray(n_small) / float(2 * small + 1), np.asarray(n_large) / float(2 * large + 1)),
                                            rate)
    with np.errstate(divide="ignore"):
        return -poisson.logsf(p - 1, lam) / np.log(10.0), p / lam


def fixed_width_set(chrom, summit, mlog10p, pileup, lengths, width):
    """the disjoint fixed-width intervals: chrom = chromosome index per region, lengths[index] = its length -> (chrom, start) of the
    kept intervals in coordinate order (chromosome index, start); every interval is [start, start + width)"""
    chrom, summit = np.asarray(chrom, np.int64), np.asarray(summit, np.int64)
    start = summit - width // 2
    inside = (start >= 0) & (start + width <= np.asarray(lengths, np.int64)[chrom]) if len(chrom) else np.zeros(0, bool)
    idx = np.flatnonzero(inside)
    order = idx[np.lexsort((start[idx], chrom[idx], -np.asarray(pileup, np.int64)[idx], -np.asarray(mlog10p, np.float64)[idx]))]
    kept = {}                       # chromosome -> sorted starts kept
    out = []
    import bisect
    for i in order.tolist():
        have = kept.setdefault(int(chrom[i]), [])
        s = int(start[i])
        j = bisect.bisect_left(have, s)
        if (j > 0 and have[j - 1] + width > s) or (j < len(have) and s + width > have[j]):
            continue
        have.insert(j, s)
        out.append((int(chrom[i]), s))
    out.sort()
    return np.asarray([c for c, _ in out], np.int64), np.asarray([s for _, s in out], np.int64)


def call_peaks(store, sizes, half_width=75, small=500, large=5000, mlog10p=5.0, max_gap=75, min_length=150, regions=None, timing=None):
    """the regions of every chromosome of `store` with records.  sizes: {chromosome: length} (every chromosome counts for the genome
    length).  regions: the per-chromosome finder (default: device_regions; the tests' host path passes the NumPy restatement).
    -> dict(chrom = index into store.references per region, start, end, summit, pileup, n_small, n_large, mlog10p, fold, and the
    summary's numbers)"""
    find = regions if regions is not None else (lambda *a: device_regions(*a, timing=timing))
    chroms = [c for c in store.references if len(store.pos[c])]
    if not chroms:
        raise PeaksError("the store holds no records")
    missing = [c for c in chroms if c not in sizes]
    if missing:
        raise PeaksError("chromosome %s has records but no length" % ", ".join(missing))
    genome = int(sum(int(v) for v in sizes.values()))
    records = kept = 0
    for c in chroms:
        p, t, n = store.pos[c], store.tlen[c], int(sizes[c])
        l, r = p + 4, p + t - 5
        records += len(p)
        kept += int(np.count_nonzero((l >= 0) & (l < n))) + int(np.count_nonzero((r >= 0) & (r < n)))
    rate = kept / float(genome)
    lam_g = (2 * half_width + 1) * rate
    lam, thr_small, thr_large = critical_tables(half_width, small, large, mlog10p)
    min_pile = min_pileup_for(lam, lam_g)
    cols = [[] for _ in range(7)]
    found = significant = 0
    for c in chroms:
        out = find(store.pos[c], store.tlen[c], int(sizes[c]), half_width, small, large, max_gap, min_length, min_pile, thr_small, thr_large)
        cols[0].append(np.full(len(out[0]), store.references.index(c), np.int64))
        for col, a in zip(cols[1:], out[:6]):
            col.append(np.asarray(a))
        found += int(out[6])
        significant += int(out[7])
    names = ("chrom", "start", "end", "summit", "pileup", "n_small", "n_large")
    res = {k: np.concatenate(v) for k, v in zip(names, cols)}
    res["mlog10p"], res["fold"] = score(res["pileup"], res["n_small"], res["n_large"], half_width, small, large, rate)
    res.update(records=records, insertions_kept=kept, insertions_dropped=2 * records - kept, genome_length=genome, lam_g=lam_g,
               min_pileup=min_pile, significant_bases=significant, regions_found=found, regions_kept=len(res["start"]))
    return res


def texts(res, references, base_name, fixed=None):
    """{suffix: bytes} of the command's files; fixed = (chrom, start, width) of the fixed-width set or None"""
    rows = []
    for i in range(len(res["start"])):
        m = float(res["mlog10p"][i])
        shown = m if np.isfinite(m) else MLOG10P_INF
        rows.append("%s\t%d\t%d\t%s_peak_%d\t%d\t.\t%.4f\t%.2f\t-1\t%d\n"
                    % (references[int(res["chrom"][i])], res["start"][i], res["end"][i], base_name, i + 1, min(1000, int(10 * shown)),
                       res["fold"][i], shown, res["summit"][i] - res["start"][i]))
    out = {".peaks.narrowPeak": "".join(rows).encode("ascii")}
    if fixed is not None:
        fc, fs, width = fixed
        out[".peaks.fixed.bed"] = "".join("%s\t%d\t%d\n" % (references[c], s, s + width) for c, s in zip(fc.tolist(), fs.tolist())).encode("ascii")
    out[".peaks.txt"] = ("records\t%d\ninsertions_kept\t%d\ninsertions_dropped\t%d\ngenome_length\t%d\nlam_g\t%.6g\nmin_pileup\t%d\n"
                         "significant_bases\t%d\nregions_found\t%d\nregions_kept\t%d\nfixed_width_kept\t%s\n"
                         % (res["records"], res["insertions_kept"], res["insertions_dropped"], res["genome_length"], res["lam_g"],
                            res["min_pileup"], res["significant_bases"], res["regions_found"], res["regions_kept"],
                            "NA" if fixed is None else "%d" % len(fixed[0]))).encode("ascii")
    return out


def get_peaks(args, regions=None, timing=None):
    """`pyatac peaks`: writes BASE.peaks.narrowPeak, BASE.peaks.txt and, with --fixed_width, BASE.peaks.fixed.bed; returns (res, texts)"""
    from .fragments import FragmentStore
    from .trackfiles import default_out
    from .utils import read_chrom_sizes, read_chrom_sizes_from_fasta
    base = default_out(argparse.Namespace(out=args.out, bam=args.bam, bed=None))      # before anything is read
    check_args(args)
    for path in (args.bam, args.fasta, args.sizes):
        if path is not None and not os.path.exists(path):
            raise PeaksError("%s: no such file" % path)
    t = timing if timing is not None else {}
    t0 = time.perf_counter()
    store = FragmentStore.open(args.bam)
    t["read_s"] = time.perf_counter() - t0
    if args.fasta is not None:
        sizes = read_chrom_sizes_from_fasta(args.fasta)
    elif args.sizes is not None:
        sizes = read_chrom_sizes(args.sizes)
    else:
        sizes = store.chrom_sizes()
    res = call_peaks(store, sizes, args.half_width, args.small, args.large, args.mlog10p, args.max_gap, args.min_length, regions=regions,
                     timing=t)
    fixed = None
    if args.fixed_width is not None:
        lengths = [int(sizes.get(c, 0)) for c in store.references]
        fixed = fixed_width_set(res["chrom"], res["summit"], res["mlog10p"], res["pileup"], lengths, args.fixed_width) + (args.fixed_width,)
    out = texts(res, store.references, os.path.basename(base), fixed)
    for suffix, text in out.items():
        with open(base + suffix, "wb") as fh:
            fh.write(text)
    return res, out
