"""`pyatac pwm`: fit the Tn5 insertion PWM of a BAM (the reference's pyatac/get_pwm.py).

The reference walks the genome in 1-kb chunks on a process pool and, per chunk, re-reads the BAM, builds the insertion track and
adds the one-hot sequence window of every base, weighted by its insertion count (get_pwm.py:21-40, tracks.py:179-201).  Here the
BAM is decoded once (FragmentStore), the regions are packed in sub-batches of about SUB_BATCH_BP bases (natac_pack_chunks) and each
sub-batch is one launch of natac_insertion_seq_counts, which gives the exact int64 window counts.  Only the finish -- normalise by
the insertion count and the background frequencies, symmetrise -- runs on the host, in float64 and in the reference's order, so the
fitted matrix is bit-identical to the reference's.
"""
import os
import time

import numpy as np

from .bias import PWM
from .chunk import Chunk, ChunkList
from .fragments import FragmentStore
from .seq import ACGT, FastaStore, getNucFreqs, getNucFreqsFromChunkList
from .utils import read_chrom_sizes_from_fasta

# genome-wide regions are cut into tiles of this many bases instead of the reference's 1-kb chunks: every insertion lies in exactly one
# tile either way, so the counts are the same, and a tile carries its fragments once instead of ~5 times (1 kb chunk, 2 kb margin)
TILE_BP = 1 << 22
# bases per sub-batch (one pack + one kernel launch): the device holds the sub-batch's sequence windows and its fragments
SUB_BATCH_BP = 1 << 26


class PWMFitError(Exception):
    """the fit has nothing to count (no insertion passed the filters)"""


def genome_regions(chrs, flank, tile=TILE_BP):
    """[flank, L - flank) of every chromosome, sorted by name like ChunkList.convertChromSizes, cut into tiles of `tile` bases;
    chromosomes with L <= 2 * flank contribute nothing"""
    out = ChunkList()
    for c in sorted(chrs.keys()):
        a, b = flank, chrs[c] - flank
        for s in range(a, b, tile):
            list.append(out, Chunk(c, s, min(s + tile, b)))
    return out


def bed_regions(bed, chrs, flank):
    """ChunkList.read(bed, chromDict=chrs, min_offset=flank) (get_pwm.py:66): regions on chromosomes missing from the FASTA are dropped
    with a warning, clipped to [flank, L - flank) and dropped when empty; not merged.  With flank 0 the reference does not clip, and
    fails on a region that reaches past the chromosome's end; here such a region is clipped to the chromosome."""
    chunks = ChunkList.read(bed, chromDict=chrs, min_offset=flank)
    if not flank:
        for ch in chunks:
            ch.start, ch.end = max(ch.start, 0), min(ch.end, chrs[ch.chrom])
        chunks[:] = [ch for ch in chunks if ch.end - ch.start >= 1]
    return chunks


def _split_bases(chunks, target_bp):
    out, a, bp = [], 0, 0
    for i, c in enumerate(chunks):
        n = c.end - c.start
        if i > a and bp + n > target_bp:
            out.append(chunks[a:i])
            a, bp = i, 0
        bp += n
    if len(chunks) > a:
        out.append(chunks[a:len(chunks)])
    return out


def pack_windows(chunks, st, fs, flank, lower, upper, atac):
    """(chunk_len, frag_off, lpos, ilen, seq_off, seq) of a list of regions: the fragments through natac_pack_chunks with a margin
    that holds every fragment one of whose ends can fall in a region, the sequence windows [start - flank, end + flank) end to end"""
    from ..pipeline import _pack_fragments
    chroms = [c.chrom for c in chunks]
    starts = np.array([c.start for c in chunks], np.int64)
    ends = np.array([c.end for c in chunks], np.int64)
    margin = max(int(upper), 1) + max(0, -int(lower)) + 1
    offs, lpos, ilen = _pack_fragments(st, chroms, starts, ends, margin, atac)
    a, b = starts - flank, ends + flank
    seq_off = np.zeros(len(chunks) + 1, np.int64)
    np.cumsum(b - a, out=seq_off[1:])
    seq = np.empty(int(seq_off[-1]), np.uint8)
    for k, c in enumerate(chroms):
        s = fs.seqs[c]
        if a[k] < 0 or b[k] > len(s):
            raise ValueError("region %s:%d-%d: its window of %d bases reaches past the chromosome" % (c, starts[k], ends[k], flank))
        seq[seq_off[k]:seq_off[k + 1]] = s[a[k]:b[k]]
    return (ends - starts).astype(np.int32), offs, lpos, ilen, seq_off, seq


def count_windows(chunks, bam, fasta, flank, lower=0, upper=2000, atac=True, sym=True, sub_bp=SUB_BATCH_BP, timing=None,
                  prefetch=True):
    """summed window counts (M int64[4, 2*flank+1], rows A C G T; n counted insertions) of the regions, one natac_insertion_seq_counts
    launch per sub-batch.  timing (a dict) gets the seconds of packing and of the device calls and the kernels' device ms."""
    from .. import get_context
    from ..pipeline import prefetch_map
    ctx = get_context()
    st = FragmentStore.open(bam)
    fs = FastaStore.open(fasta)
    M = np.zeros((4, 2 * flank + 1), np.int64)
    n = 0
    t = timing if timing is not None else {}
    for k in ("pack_s", "device_s", "kernel_ms"):
        t.setdefault(k, 0.0)
    t.setdefault("sub_batches", 0)

    def pack(sub):
        t0 = time.perf_counter()
        out = pack_windows(sub, st, fs, flank, lower, upper, atac)
        return out, time.perf_counter() - t0

    subs = _split_bases(chunks, sub_bp)
    for (arrs, dt) in (prefetch_map(pack, subs) if prefetch else map(pack, subs)):
        t["pack_s"] += dt
        t0 = time.perf_counter()
        m, nn, ms = ctx.insertion_seq_counts(*arrs, flank, lower, upper, sym=sym, with_kernel_ms=True)
        t["device_s"] += time.perf_counter() - t0
        t["kernel_ms"] += ms
        t["sub_batches"] += 1
        M += m
        n += nn
    return M, n


def finish_pwm(M, n, normfreqs, flank, sym):
    """the reference's finish in its order (get_pwm.py:80-93): M / n, each row divided by its background frequency, then unless
    no_sym the average of the matrix and its reverse complement, mirrored about the centre column"""
    result = np.asarray(M, dtype=np.float64) / float(n)
    result = result / np.reshape(np.repeat(np.asarray(normfreqs, dtype=np.float64), result.shape[1]), result.shape)
    if sym:
        left = result[:, 0:(flank + 1)]
        right = result[:, flank:]
        rightflipped = np.fliplr(np.flipud(right))
        combined = (left + rightflipped) / 2
        result = np.hstack((combined, np.fliplr(np.flipud(combined[:, 0:flank]))))
    return result


def get_pwm(args, timing=None):
    """`pyatac pwm` (get_pwm.py:55-93): writes <out>.PWM.txt.  Raises PWMFitError (and writes nothing) when no insertion is counted,
    where the reference writes a matrix of NaN."""
    if not args.out:
        args.out = ".".join(os.path.basename(args.bam).split(".")[0:-1])
    flank = int(args.flank)
    if flank < 0 or flank > 1000:
        raise ValueError("--flank must be in [0, 1000] (got %d)" % flank)
    if args.upper <= args.lower:
        raise ValueError("--upper (%d) must be larger than --lower (%d)" % (args.upper, args.lower))
    FragmentStore.prefetch(args.bam)
    chrs = read_chrom_sizes_from_fasta(args.fasta)
    chunks = genome_regions(chrs, flank) if args.bed is None else bed_regions(args.bed, chrs, flank)
    M, n = count_windows(chunks, args.bam, args.fasta, flank, args.lower, args.upper, args.atac, args.sym, timing=timing)
    if n == 0:
        raise PWMFitError("no insertion with %d <= insert size < %d falls in the %s: nothing to fit a PWM to (no file written)" % (
            args.lower, args.upper, "regions of the bed file" if args.bed else "genome"))
    t0 = time.perf_counter()
    normfreqs = getNucFreqsFromChunkList(chunks, args.fasta, ACGT) if args.bed else getNucFreqs(args.fasta, ACGT)
    if timing is not None:
        timing["background_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    result = finish_pwm(M, n, normfreqs, flank, args.sym)
    PWM(result, flank, flank, list(ACGT)).save(args.out + ".PWM.txt", py2_floats=True)
    if timing is not None:
        timing["finish_s"] = time.perf_counter() - t0
        timing["n_insertions"] = int(n)
    return result

