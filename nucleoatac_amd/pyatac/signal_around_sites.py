"""`pyatac signal`: the per-base value of a tabix-indexed bedGraph around a set of sites, per site and summed over the sites (the
reference's pyatac/signal_around_sites.py).

The reference opens the track once per site set and reads, pads, transforms and adds one window at a time in Python.  Here the sites
are read as columns, their windows are worked out on the host, and the sites go to the device in BED order in batches: the windows
of a batch are merged per chromosome into disjoint spans, the spans are read in one natac_tbx_read_regions call into one buffer, and
one natac_site_signal call gathers every window from it, transforms the rows and sums the columns.

The site rule (Python-2 integer division): centre c = start + len // 2 on plus, end - len // 2 - 1 on minus ("-" is minus, every other
strand value and no --strand is plus).  K = up + down + 1 columns.  With up and down both non-zero the window is [max(0, c - up),
min(size, c + 1 + down)) on plus and [max(0, c - down), min(size, c + 1 + up)) on minus, `size` from --sizes; with up == down == 0 it
is [c, c + 1) and --sizes is not consulted.  A base without a record is NaN, a base under several records has the value of the last
one in file order, a chromosome that is not in the track's index is all NaN.  A window shorter than K is padded with zeros (not NaN):
on the left if the clipped window starts at 0, else on the right -- decided before a minus-strand row is reversed, so a window clipped
at both ends of a short chromosome is padded on the left only.  Then, per row: reverse on minus; --exp: exp(row), padding becomes 1,
NaN stays; --positive: values below 0 become 0, NaN and -0.0 stay; --scale: NaN becomes 0 in the row itself and the row is divided
by S + (S == 0), S = the sum of its absolute values.  The aggregate is the column sum of the rows with NaN as 0; --norm divides it by
the number of sites kept.  Rows of length zero in the BED are dropped, as ChunkList.read does.

Summation order: the device adds a column over segments of _lib.SIGNAL_SEG consecutive sites, then the segment sums in order; the
batches' aggregates are added here in batch order.  The same inputs give the same bits; the reference's own order (site by site, or
np.sum over the matrix with --all) differs from it in the last bits.

TWO DELIBERATE DEVIATIONS.  (1) With exactly one of --up / --down zero the reference does not extend the centre at all and then
broadcasts its one-base read over K columns -- an accident of `up != 0 and down != 0`; that combination is refused with SignalError.
(2) Where the reference ends in a traceback -- a BED chromosome that is not in --sizes (KeyError), a site whose clipped window has
negative length because it starts past the chromosome's end (np.ones of a negative size), no site at all -- SignalError names the BED
row before any device work, and nothing is written.  No .eps plot is made.
"""
import gzip
import os
import time

import numpy as np

from .chunk import read_bed_columns
from .get_nucleotide import site_centers
from .utils import read_chrom_sizes

BATCH_VALUES = 1 << 25          # columns (n sites x K) of one device call: 256 MB of float64 rows, and at most as many track values
TEXT_ROWS = 256                 # matrix rows formatted by one % operation


class SignalError(Exception):
    """`pyatac signal` cannot run on these arguments or sites (nothing is written)"""


def site_windows(names, chrom, start, end, minus, sizes, up, down):
    """(win_start, win_end, lead, K) per site (columns of read_bed_columns): the clipped window [win_start, win_end) in genomic
    coordinates and the number of zero columns before it in genomic orientation.  Raises SignalError naming the row."""
    if up < 0 or down < 0:
        raise SignalError("--up (%d) and --down (%d) must not be negative" % (up, down))
    if (up == 0) != (down == 0):
        raise SignalError("--up %d --down %d: with exactly one of them 0 the reference reads one base and repeats it over %d columns; "
                          "give both, or 0 for both" % (up, down, up + down + 1))
    K = up + down + 1
    c = site_centers(start, end, minus)
    if K == 1:
        return c, c + 1, np.zeros(len(c), np.int32), K
    missing = [k for k, name in enumerate(names) if name not in sizes]
    if missing:
        i = int(np.flatnonzero(np.isin(chrom, missing))[0])
        raise SignalError("row %d (%s:%d-%d): chromosome %s is not in the --sizes file" % (i + 1, names[chrom[i]], start[i], end[i],
                                                                                           names[chrom[i]]))
    size = np.array([sizes[name] for name in names], np.int64)[chrom] if len(names) else np.zeros(0, np.int64)
    ws = np.maximum(0, c - np.where(minus, down, up))
    we = np.minimum(size, c + 1 + np.where(minus, up, down))
    bad = np.flatnonzero(we < ws)
    if len(bad):
        i = int(bad[0])
        raise SignalError("row %d (%s:%d-%d): its window starts at %d, past the end of %s (%d bases)" % (
            i + 1, names[chrom[i]], start[i], end[i], ws[i], names[chrom[i]], size[i]))
    lead = np.where(ws == 0, K - (we - ws), 0).astype(np.int32)
    return ws, we, lead, K


def merge_spans(chrom, ws, we):
    """the windows of one batch merged per chromosome into disjoint spans: (span_chrom, span_start, span_end, span_off, src) with the
    spans sorted by (chromosome index, start), span_off their offsets in one value buffer (one more entry: its length) and src[i] the
    offset of window i's first base in it"""
    order = np.lexsort((ws, chrom))
    c, s, e = chrom[order], ws[order], we[order]
    reach = np.maximum.accumulate(e + (c.astype(np.int64) << 42)) - (c.astype(np.int64) << 42)     # furthest end so far, per chromosome
    first = np.ones(len(order), bool)
    first[1:] = (c[1:] != c[:-1]) | (s[1:] > reach[:-1])
    head = np.flatnonzero(first)
    span_chrom, span_start = c[head], s[head]
    span_end = reach[np.append(head[1:] - 1, len(order) - 1)] if len(order) else reach[:0]
    span_off = np.concatenate(([0], np.cumsum(span_end - span_start))).astype(np.int64)
    key = (chrom.astype(np.int64) << 42) + ws
    k = np.searchsorted((span_chrom.astype(np.int64) << 42) + span_start, key, side="right") - 1
    src = span_off[k] + (ws - span_start[k]) if len(order) else np.zeros(0, np.int64)
    return span_chrom, span_start, span_end, span_off, src


def tracks_text(mat):
    """np.savetxt(mat, delimiter=",", fmt="%1.5g") as bytes, TEXT_ROWS rows per % operation"""
    n, K = mat.shape
    row = ",".join(["%1.5g"] * K) + "\n"
    out = []
    for i in range(0, n, TEXT_ROWS):
        block = mat[i:i + TEXT_ROWS]
        out.append(((row * len(block)) % tuple(block.ravel().tolist())).encode("latin1"))
    return b"".join(out)


def agg_text(result):
    """np.savetxt(result, delimiter="\\t") of the 1-d aggregate: one '%.18e' value per line"""
    return "".join("%.18e\n" % v for v in result.tolist())


def get_signal(args, timing=None):
    """`pyatac signal` (signal_around_sites.py:88-118): writes <out>.tracks.txt.gz (--all) and <out>.agg.track.txt (unless --no_agg);
    returns (aggregate float64[K], matrix float64[n, K] or None) at full precision"""
    if not args.out:
        args.out = ".".join(os.path.basename(args.bed).split(".")[0:-1])
    t = timing if timing is not None else {}
    for k in ("read_s", "device_s", "kernel_ms"):
        t.setdefault(k, 0.0)
    t0 = time.perf_counter()
    sizes = read_chrom_sizes(args.sizes)
    names, chrom, start, end, minus = read_bed_columns(args.bed, strand_col=args.strand)
    t["bed_s"] = time.perf_counter() - t0
    ws, we, lead, K = site_windows(names, chrom, start, end, minus, sizes, args.up, args.down)
    n = len(start)
    if n == 0:
        raise SignalError("%s has no site of at least one base" % args.bed)
    length = (we - ws).astype(np.int32)
    from .. import get_context
    from ..tabix import NativeTabix
    ctx = get_context()
    tbx = NativeTabix(args.bg)
    agg = np.zeros(K)
    mat = np.empty((n, K)) if args.all else None
    per = max(1, BATCH_VALUES // K)
    try:
        for a in range(0, n, per):
            b = min(n, a + per)
            t0 = time.perf_counter()
            sc, ss, se, off, src = merge_spans(chrom[a:b], ws[a:b], we[a:b])
            vals, _ = tbx.read_regions([names[k] for k in sc.tolist()], ss, se, empty=np.nan, value_col=4)
            t["read_s"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            part, m, ms = ctx.site_signal(vals, src, length[a:b], lead[a:b], minus[a:b], K, exp=args.exp, positive=args.positive,
                                          scale=args.scale, want_matrix=args.all, with_kernel_ms=True)
            t["device_s"] += time.perf_counter() - t0
            t["kernel_ms"] += ms
            agg += part
            if args.all:
                mat[a:b] = m
    finally:
        tbx.close()
    t0 = time.perf_counter()
    if args.all:
        with gzip.open(args.out + ".tracks.txt.gz", "wb") as f:
            for i in range(0, n, 64 * TEXT_ROWS):
                f.write(tracks_text(mat[i:i + 64 * TEXT_ROWS]))
    result = agg
    if not args.no_agg:
        if args.norm:
            result = agg / n
        with open(args.out + ".agg.track.txt", "w") as f:
            f.write(agg_text(result))
    t["text_s"] = time.perf_counter() - t0
    return result, mat
