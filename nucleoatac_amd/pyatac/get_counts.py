"""`pyatac counts`: fragment counts per BED window (the reference's pyatac/get_counts.py).

The reference re-fetches the BAM for every window and tests every read in Python.  Here the BAM is decoded once (FragmentStore), the
windows are grouped by chromosome, and one natac_region_counts call per chromosome uploads that chromosome's records once, finds
every window's contiguous range of candidate records on the device and counts them there.  The counts are exact integers, so the
decompressed <out>.counts.txt.gz equals the reference's text.

The counting rule, per window [s, e), over EVERY kept record (forward read of a proper pair) of the window's chromosome:
l = pos + 4, ilen = |tlen| - 8 (--not_atac: l = pos, ilen = |tlen|), r = l + ilen - 1; the record counts once if
lower <= ilen < upper and (s <= l < e or s <= r < e).  ilen == 0 gives r = l - 1 and is counted by the same rule.  The reference
looks only at the reads of fetch(chrom, max(0, s - upper), e + upper); that is a superset filter: a fragment that passes the size
filter with an end in the window always has its forward read overlapping that interval unless the read is shorter than 3 bases, and
the store keeps no read lengths -- so "every kept record" is the rule here.  Overlapping, repeated and unsorted windows are counted
independently; windows with end - start < 1 are dropped like ChunkList.read drops them.
"""
import gzip
import os
import time

import numpy as np

from .chunk import read_bed_columns
from .fragments import FragmentStore


class CountsError(Exception):
    """`pyatac counts` cannot run on these arguments (nothing is written)"""


def count_regions(names, chrom, start, end, bam, lower=0, upper=500, atac=True, timing=None):
    """int64 count of every region (columns of read_bed_columns), in their order: one natac_region_counts call per chromosome.
    timing (a dict) gets the seconds of the device calls and the kernels' device ms."""
    from .. import get_context
    st = FragmentStore.open(bam)
    missing = [c for c in names if c not in st.pos]
    if missing:
        raise CountsError("chromosome %s of the bed file is not in %s" % (", ".join(missing), bam))
    t = timing if timing is not None else {}
    t.setdefault("device_s", 0.0)
    t.setdefault("kernel_ms", 0.0)
    out = np.zeros(len(start), np.int64)
    for k, c in enumerate(names):
        idx = np.flatnonzero(chrom == k)
        t0 = time.perf_counter()
        cnt, ms = get_context().region_counts(st.pos[c], st.tlen[c], start[idx], end[idx], lower, upper, atac, with_kernel_ms=True)
        t["device_s"] += time.perf_counter() - t0
        t["kernel_ms"] += ms
        out[idx] = cnt
    return out


def get_counts(args, timing=None):
    """`pyatac counts` (get_counts.py:20-47): writes <out>.counts.txt.gz, one integer per line in BED order, and returns the counts"""
    if args.out is None:
        args.out = ".".join(os.path.basename(args.bed).split(".")[0:-1])
    if args.upper <= args.lower:
        raise CountsError("--upper (%d) must be larger than --lower (%d)" % (args.upper, args.lower))
    t = timing if timing is not None else {}
    FragmentStore.prefetch(args.bam)
    t0 = time.perf_counter()
    names, chrom, start, end, _ = read_bed_columns(args.bed)
    t["bed_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    FragmentStore.open(args.bam)
    t["decode_s"] = time.perf_counter() - t0
    mat = count_regions(names, chrom, start, end, args.bam, args.lower, args.upper, args.atac, timing=t)
    t0 = time.perf_counter()
    text = "\n".join(map(str, mat.tolist()))
    with gzip.open(args.out + ".counts.txt.gz", "wb") as f:          # np.savetxt(fmt='%i', delimiter="\n"): a newline after every value
        f.write((text + "\n").encode("ascii") if len(mat) else b"")
    t["text_s"] = time.perf_counter() - t0
    return mat
