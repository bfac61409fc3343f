"""`pyatac cellqc`: per-cell TSS enrichment and FRiP of a single-cell fragment file.  This command is this package's own, like `cells`,
`split` and `cellcounts`: the reference has no such tool.  It stands between them: `cells` discovers the barcodes with their fragment
counts and nucleosome signal, `cellqc` adds the two numbers single-cell ATAC users filter on before they cluster or split, and
`split --groups` / `cellcounts --cells` take the table of passing barcodes it writes.

The fragment file is read ONCE with the cell of every record kept (FragmentStore.from_fragments_cells), the --tss sites are centred as
Chunk.center does (plus: start + (end - start) // 2, minus: end - (end - start) // 2 - 1) and sorted per chromosome, the --peaks rows are
merged per chromosome into disjoint ascending intervals (rows that overlap are joined, rows that only touch stay apart), and one
natac_cell_site_qc call per chromosome that is in the store and has sites or peaks counts on the device (csrc/natac_cellqc.hpp); the
results are added up in the order of the store's chromosomes.  All counts are exact integers.

The counting rule (include/natac.h): every record counts, with its two insertions l = pos + 4 and r = l + ilen - 1, ilen = tlen - 8; there
is no size filter.  For an insertion x and a site (c, minus), d = x - c, or c - x on the minus strand; a pair with |d| <= flank adds 1 to
the profile at offset d, 1 to the cell's tss_center if |d| <= center and 1 to its tss_flank if |d| > flank - edge.  A record whose l or r
lies in a merged peak interval [start, end) adds 1 to the cell's in_peaks, once.  Repeated and overlapping sites are separate sites; a site
or a peak on a chromosome the file never mentions adds nothing (a fragment file has no sequence dictionary, so that is not an error).

BASE.cellqc.tsv             every listed barcode behind a header line that begins with '#': barcode, fragments, tss_center, tss_flank,
                            tss_enrichment = (tss_center / (2 * center + 1)) / (tss_flank / (2 * edge)) (%.4f; NA when tss_flank is 0),
                            in_peaks, frip = in_peaks / fragments (%.4f; NA when fragments is 0), pass; the columns of an input that
                            was not given hold NA.  pass is 1 when every given threshold holds (>=); an NA fails a given threshold.
BASE.cellqc.cells.tsv       the passing barcodes, one per line, in table order;
BASE.cellqc.tss_profile.txt with --tss: offset TAB count for offset -flank .. flank, summed over the listed cells, strand-aware;
BASE.cellqc.txt             barcodes_listed, barcodes_seen, data_lines, unassigned_lines, sites, peak_intervals, passing.
Everything is computed before the first file is written, so an error leaves nothing behind.

Measured on the MI355X box (tools/bench_cellqc.py, one box, three runs: 10 M fragments in 10,000 cells, 99 MB BGZF, 20,000 sites, 100,000
peaks, flank 1000 / center 500 / edge 100, 8.0 M insertion-site pairs): the tagged read 0.32 s, the four device calls 0.020 s in the first
run and 0.010 s in the next two (the host's operand checks, upload and download included; 0.94 ms in their kernels); the NumPy restatement
of the same arrays (searchsorted + bincount) on that box 1.54 s, and equal.
"""
import os
import time

import numpy as np

from .chunk import read_bed_columns
from .get_nucleotide import site_centers

HEADER = b"#barcode\tfragments\ttss_center\ttss_flank\ttss_enrichment\tin_peaks\tfrip\tpass\n"


class CellQCError(ValueError):
    """`pyatac cellqc` cannot answer: arguments that break a rule, a missing file, or thresholds no cell passes"""


def merge_peaks(start, end):
    """the rows [start, end) of one chromosome as disjoint ascending intervals: rows with end - start < 1 are dropped, rows that overlap
    are joined, rows that only touch stay apart -> (start int64, end int64)"""
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    keep = end - start >= 1
    start, end = start[keep], end[keep]
    if not len(start):
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    o = np.argsort(start, kind="stable")
    s, e = start[o], end[o]
    reach = np.maximum.accumulate(e)                     # the furthest end of the rows so far
    head = np.ones(len(s), bool)
    head[1:] = s[1:] >= reach[:-1]                       # a row starts an interval when no row before it goes past its start
    first = np.flatnonzero(head)
    last = np.append(first[1:], len(s)) - 1
    return s[first], reach[last]


def check_args(args):
    """the argument rules of the command -> CellQCError"""
    from .._lib import CELLQC_MAX_FLANK
    if args.tss is None and args.peaks is None:
        raise CellQCError("at least one of --tss and --peaks is required")
    if args.min_tss_enrichment is not None and args.tss is None:
        raise CellQCError("--min_tss_enrichment needs --tss")
    if args.min_frip is not None and args.peaks is None:
        raise CellQCError("--min_frip needs --peaks")
    if not 1 <= args.flank <= CELLQC_MAX_FLANK:
        raise CellQCError("--flank (%d) must be in [1, %d]" % (args.flank, CELLQC_MAX_FLANK))
    if args.center < 0:
        raise CellQCError("--center (%d) must not be negative" % args.center)
    if args.edge < 1:
        raise CellQCError("--edge (%d) must be at least 1" % args.edge)
    if args.center + args.edge > args.flank:
        raise CellQCError("--center (%d) + --edge (%d) must not exceed --flank (%d)" % (args.center, args.edge, args.flank))


def cell_qc(store, n_cells, sites=None, peaks=None, flank=1000, center=500, edge=100, timing=None):
    """(tss_center, tss_flank, in_peaks int64[n_cells], profile int64[2 * flank + 1]) of the tagged `store`.  sites: {chromosome: (centres
    ascending, minus)} or None; peaks: {chromosome: (start, end)} merged, or None.  One natac_cell_site_qc call per chromosome of the store
    that has sites or peaks, added up in the store's order."""
    from .. import get_context
    t = timing if timing is not None else {}
    t.setdefault("device_s", 0.0)
    t.setdefault("kernel_ms", 0.0)
    total = [np.zeros(n_cells, np.int64) for _ in range(3)] + [np.zeros(2 * flank + 1, np.int64)]
    for c in store.references:
        sc, sm = sites.get(c, (None, None)) if sites else (None, None)
        ps, pe = peaks.get(c, (None, None)) if peaks else (None, None)
        if not len(store.pos[c]) or ((sc is None or not len(sc)) and (ps is None or not len(ps))):
            continue
        t0 = time.perf_counter()
        out = get_context().cell_site_qc(store.pos[c], store.tlen[c], store.cell[c], n_cells, sc, sm, flank, center, edge, ps, pe,
                                         with_kernel_ms=True)
        t["device_s"] += time.perf_counter() - t0
        t["kernel_ms"] += out[4]
        for a, b in zip(total, out[:4]):
            a += b
    return tuple(total)


def sites_by_chrom(names, chrom, start, end, minus):
    """{chromosome: (centres ascending, minus uint8)}: a stable sort, so equal centres keep the order of the file"""
    center = site_centers(start, end, minus)
    out = {}
    for k, c in enumerate(names):
        idx = np.flatnonzero(chrom == k)
        o = np.argsort(center[idx], kind="stable")
        out[c] = (center[idx][o].astype(np.int64), minus[idx][o].astype(np.uint8))
    return out


def peaks_by_chrom(names, chrom, start, end):
    """{chromosome: merge_peaks of its rows}"""
    return {c: merge_peaks(start[chrom == k], end[chrom == k]) for k, c in enumerate(names)}


def finish(barcodes, fragments, tss_center, tss_flank, in_peaks, profile, flank, center, edge, min_tss_enrichment=None, min_frip=None,
           n_unassigned=0, n_sites=0, n_peaks=0):
    """the host finish from the integer arrays: formulas, NA, pass and the file texts.  tss_center / tss_flank / profile are None without
    --tss, in_peaks is None without --peaks.  -> (passing bool[n], {suffix: bytes}) with the suffixes .cellqc.tsv, .cellqc.cells.tsv,
    .cellqc.txt and, with sites, .cellqc.tss_profile.txt.  CellQCError when no cell passes."""
    fragments = np.asarray(fragments, np.int64)
    n = len(barcodes)
    ok = np.ones(n, bool)
    enrich = frip = None
    if tss_center is not None:
        tc, tf = np.asarray(tss_center, np.int64), np.asarray(tss_flank, np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            enrich = (tc / float(2 * center + 1)) / (tf / float(2 * edge))
        enrich[tf == 0] = np.nan
        if min_tss_enrichment is not None:
            ok &= (tf > 0) & (np.nan_to_num(enrich, nan=-np.inf) >= min_tss_enrichment)
    if in_peaks is not None:
        ip = np.asarray(in_peaks, np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            frip = ip / fragments.astype(np.float64)
        frip[fragments == 0] = np.nan
        if min_frip is not None:
            ok &= (fragments > 0) & (np.nan_to_num(frip, nan=-np.inf) >= min_frip)
    if not ok.any():
        raise CellQCError("no cell passes (%d barcodes listed; --min_tss_enrichment is %s, --min_frip is %s)"
                          % (n, min_tss_enrichment, min_frip))

    def ratio(v, k):
        return b"NA" if v is None or np.isnan(v[k]) else b"%.4f" % v[k]

    def count(v, k):
        return b"NA" if v is None else b"%d" % int(v[k])

    rows = [HEADER]
    for k, b in enumerate(barcodes):
        rows.append(b"%s\t%d\t%s\t%s\t%s\t%s\t%s\t%d\n" % (b, int(fragments[k]), count(tss_center, k), count(tss_flank, k), ratio(enrich, k),
                                                            count(in_peaks, k), ratio(frip, k), int(ok[k])))
    texts = {".cellqc.tsv": b"".join(rows),
             ".cellqc.cells.tsv": b"".join([b + b"\n" for b, o in zip(barcodes, ok.tolist()) if o])}
    if profile is not None:
        texts[".cellqc.tss_profile.txt"] = "".join(["%d\t%d\n" % (j - flank, v) for j, v in enumerate(np.asarray(profile).tolist())]).encode("ascii")
    texts[".cellqc.txt"] = ("barcodes_listed\t%d\nbarcodes_seen\t%d\ndata_lines\t%d\nunassigned_lines\t%d\nsites\t%d\npeak_intervals\t%d\n"
                            "passing\t%d\n" % (n, int(np.count_nonzero(fragments)), int(fragments.sum()) + n_unassigned, n_unassigned,
                                               n_sites, n_peaks, int(ok.sum()))).encode("ascii")
    return ok, texts


def get_cellqc(args, timing=None):
    """`pyatac cellqc`: writes BASE.cellqc.tsv, .cellqc.cells.tsv, .cellqc.txt and, with --tss, .cellqc.tss_profile.txt; returns
    (passing, texts)"""
    from .cellgroups import CellGroupError, default_base, read_groups
    from .fragments import FragmentStore
    check_args(args)
    base = args.out if args.out else default_base(args.fragments)
    t = timing if timing is not None else {}
    for path in (args.cells, args.tss, args.peaks, args.fragments):
        if path is not None and not os.path.exists(path):
            raise CellGroupError("%s: no such file" % path)
    barcodes = read_groups(args.cells, header=args.header).barcodes
    sites = peaks = None
    n_sites = n_peaks = 0
    if args.tss is not None:
        names, chrom, start, end, minus = read_bed_columns(args.tss, strand_col=args.strand)
        sites = sites_by_chrom(names, chrom, start, end, minus)
        n_sites = len(start)
    if args.peaks is not None:
        names, chrom, start, end, _ = read_bed_columns(args.peaks)
        peaks = peaks_by_chrom(names, chrom, start, end)
        n_peaks = sum(len(p[0]) for p in peaks.values())
    t0 = time.perf_counter()
    store, bc_count, n_unassigned = FragmentStore.from_fragments_cells(args.fragments, barcodes)
    t["read_s"] = time.perf_counter() - t0
    tc, tf, ip, prof = cell_qc(store, len(barcodes), sites, peaks, args.flank, args.center, args.edge, timing=t)
    if sites is None:
        tc = tf = prof = None
    if peaks is None:
        ip = None
    ok, texts = finish(barcodes, bc_count, tc, tf, ip, prof, args.flank, args.center, args.edge, args.min_tss_enrichment, args.min_frip,
                       n_unassigned, n_sites, n_peaks)
    for suffix, text in texts.items():
        with open(base + suffix, "wb") as fh:
            fh.write(text)
    return ok, texts
