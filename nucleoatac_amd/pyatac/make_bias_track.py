"""`pyatac bias`: the genome-wide (or per-region) log Tn5 preference track of a FASTA under a PWM (the reference's
pyatac/make_bias_track.py), written as <out>.Scores.bedgraph.gz + .tbi.

Regions are the reference's: without --bed the 1-kb chunks of every chromosome, chromosomes by name; with --bed the BED regions,
those on chromosomes the FASTA lacks dropped with a warning (checkChroms; `ins` / `cov` fail there, like the reference), then merged.
Per region [s, e) on a chromosome of length L, InsertionBiasTrack.computeBias (pyatac/bias.py:85-92) slops to [max(0, s - up),
min(L, e + down)), scores every full PWM window and trims, so the region's track is [max(0, s - up) + up, min(L, e + down) - down):
a chromosome's first track starts at `up`, its last ends at L - down, interior chunks abut.  Every region stays a chunk of its own, so
lines break at region boundaries like the reference's.

Here the sequence windows are cut from the FastaStore on the prefetch threads, natac_run_pwm_track scores them straight into a
per-base track in HBM, and the device writer turns that into BGZF members and tabix records (trackfiles.write_packed_track_file): no
score crosses PCIe.

A deliberate divergence: where the trimmed interval is empty or negative (a last chunk of at most `down` bases, a chromosome shorter
than up + down + 1, a BED region starting at or past L) the reference raises inside Track.write_track ("Inconsistency between length
of values and start/end values") and leaves a broken run.  Here such a region writes no line, the run goes on, and one warning on
stderr names the regions.

k-mer PWMs (row words longer than one letter) are not supported, as in Context.pwm_bias: BiasTrackError, no file.
"""
import os
import sys
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..packing import PackedChunks
from .bias import PWM
from .chunk import Chunk, ChunkList
from .seq import FastaStore
from .utils import read_chrom_sizes_from_fasta


class BiasTrackError(Exception):
    """the PWM cannot be scored on the device"""


@dataclass
class SeqTrackChunks(PackedChunks):
    """a fragment-free batch whose chunks are trimmed track intervals, with the bases under each: track_seq[track_seq_off[i] :
    track_seq_off[i + 1]] = the chunk_len[i] + K - 1 bases of [start_i - up, end_i + down)"""
    track_seq_off: Optional[np.ndarray] = None
    track_seq: Optional[np.ndarray] = None


def default_out(args):
    """the basename of the BED file without its last extension, else of the FASTA (make_bias_track.py:61-65)"""
    if args.out:
        return args.out
    src = args.fasta if args.bed is None else args.bed
    return ".".join(os.path.basename(src).split(".")[0:-1])


def bias_regions(chrs, up, down, bed=None, splitsize=1000):
    """(tracks, empty): the trimmed track interval of every region, in the reference's order, as a ChunkList, and the regions
    (untrimmed Chunks) whose trimmed interval is empty or negative, which write nothing.  chrs: {chromosome: length} of the FASTA."""
    if bed is None:
        chunks = ChunkList.convertChromSizes(chrs, splitsize=splitsize)
    else:
        chunks = ChunkList.read(bed)
        chunks.checkChroms(list(chrs.keys()))
        chunks.merge()
    tracks, empty = ChunkList(), []
    for c in chunks:
        n = chrs[c.chrom]
        a = max(0, c.start - up) + up
        b = min(n, c.end + down) - down
        if b > a:
            list.append(tracks, Chunk(c.chrom, a, b))
        else:
            empty.append(c)
    return tracks, empty


def _warn_empty(empty, up, down):
    shown = ", ".join("%s:%d-%d" % (c.chrom, c.start, c.end) for c in empty[:20])
    more = " and %d more" % (len(empty) - 20) if len(empty) > 20 else ""
    sys.stderr.write("pyatac bias: warning: %d region%s too close to a chromosome end to hold one PWM window (%d up, %d down) wrote "
                     "no lines: %s%s\n" % (len(empty), "s" if len(empty) > 1 else "", up, down, shown, more))


def pack_seq_windows(sub, fs, up, down):
    """SeqTrackChunks of the trimmed intervals `sub`: no fragments, the sequence windows laid end to end"""
    nc = len(sub)
    starts = np.fromiter((c.start for c in sub), np.int64, nc)
    ends = np.fromiter((c.end for c in sub), np.int64, nc)
    segs = [fs.seqs[c.chrom][c.start - up:c.end + down] for c in sub]
    off = np.zeros(nc + 1, np.int64)
    np.cumsum(ends - starts + (up + down), out=off[1:])
    seq = np.concatenate(segs) if segs else np.zeros(0, np.uint8)
    if seq.shape[0] != off[-1]:
        raise ValueError("a track interval reaches past its chromosome in the FASTA")
    return SeqTrackChunks(chunk_start=starts, chunk_len=(ends - starts).astype(np.int32), frag_off=np.zeros(nc + 1, np.int64),
                          frag_lpos=np.zeros(0, np.int32), frag_ilen=np.zeros(0, np.int32), bias_off=None, bias_log=None,
                          chroms=[c.chrom for c in sub], track_seq_off=off, track_seq=seq)


def make_bias_track(args, timing=None, max_chunks=None):
    """writes <out>.Scores.bedgraph.gz and its .tbi (make_bias_track.py:57-95).  timing (a dict) also gets fasta_s, the wait for the
    FASTA to be loaded."""
    from .. import _lib as L
    from .trackfiles import write_packed_track_file
    args.out = default_out(args)
    pwm = PWM.open(args.pwm)
    lens = set(len(x) for x in pwm.nucleotides)
    if lens != {1}:
        raise BiasTrackError("k-mer PWMs (row words of %s letters) are not supported: single-nucleotide PWMs only (no file written)"
                             % "/".join(str(x) for x in sorted(lens)))
    logp = np.log(np.asarray(pwm.mat, dtype=np.float64))
    nucs = np.frombuffer("".join(pwm.nucleotides).encode("ascii"), dtype=np.uint8)
    if logp.shape != (len(pwm.nucleotides), pwm.up + pwm.down + 1):
        raise BiasTrackError("PWM matrix is %s, not (rows, up + down + 1) = (%d, %d) (no file written)" % (
            logp.shape, len(pwm.nucleotides), pwm.up + pwm.down + 1))
    FastaStore.prefetch(args.fasta)            # loads while the regions are formed
    tracks, empty = bias_regions(read_chrom_sizes_from_fasta(args.fasta), pwm.up, pwm.down, args.bed)
    if empty:
        _warn_empty(empty, pwm.up, pwm.down)
    t0 = time.perf_counter()
    fs = FastaStore.open(args.fasta)
    if timing is not None:
        timing["fasta_s"] = time.perf_counter() - t0

    def run(b):
        b.run_pwm_track(b.packed.track_seq_off, b.packed.track_seq, logp, nucs)
        return L.T_BIAS
    return write_packed_track_file(args.out + ".Scores.bedgraph.gz", tracks, lambda sub: pack_seq_windows(sub, fs, pwm.up, pwm.down), run,
                                   max_chunks=max_chunks, timing=timing)
