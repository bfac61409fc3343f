"""The driver behind `pyatac ins`, `pyatac cov` and (write_packed_track_file) `pyatac bias`: regions -> packed sub-batches -> one track
kernel per sub-batch -> bedGraph.gz + .tbi.

The reference maps every 1-kb chunk (or merged BED region) on a process pool, re-reads the BAM per chunk and writes every region with
its own Track.write_track into a text file that it then compresses and indexes (get_ins.py:49-85, get_cov.py:40-76).  Here the BAM is
decoded once (FragmentStore), the regions are packed in sub-batches (pipeline.sub_batches, natac_pack_chunks) on a small thread pool
ahead of the device, and per sub-batch one kernel fills the track and the device writer turns it into BGZF members and tabix records
(natac_batch_format_track, writer.TrackFile).  Each region stays a chunk of its own, so lines break at every region boundary like the
reference's.
"""
import os
import time

import numpy as np

from .chunk import ChunkList
from .fragments import FragmentStore
from .utils import read_chrom_sizes_from_bam

MAX_CHUNKS = 4096       # regions per sub-batch (pipeline.sub_batches also caps its bases)


class MissingChromosomeError(Exception):
    """a BED region lies on a chromosome that the BAM does not have"""


def default_out(args):
    """the basename of the BAM without its last extension, or of the BED file when one is given (get_ins.py:66-70)"""
    if args.out:
        return args.out
    src = args.bam if args.bed is None else args.bed
    return ".".join(os.path.basename(src).split(".")[0:-1])


def track_regions(bam, bed=None, splitsize=1000):
    """the reference's regions: ChunkList.convertChromSizes(read_chrom_sizes_from_bam(bam), splitsize) -- chromosomes by name, 1-kb
    chunks, the last one of each chromosome cut short -- or ChunkList.read(bed) merged, not clipped to the chromosomes.  A region on a
    chromosome the BAM lacks raises MissingChromosomeError (the reference fails on it)."""
    chrs = read_chrom_sizes_from_bam(bam)
    if bed is None:
        return ChunkList.convertChromSizes(chrs, splitsize=splitsize)
    chunks = ChunkList.read(bed)
    chunks.merge()
    bad = sorted(set(c.chrom for c in chunks if c.chrom not in chrs))
    if bad:
        raise MissingChromosomeError("chromosome%s %s of %s not in the BAM file (no file written)" % (
            "s" if len(bad) > 1 else "", ", ".join(bad), bed))
    return chunks


def gaussian_window(smooth):
    """(w, wsum) of utils.smooth(..., window="gaussian", norm=True) for window_len = smooth (pyatac/utils.py:23-52): an even length gets
    one more tap and sd = (M - 1) / 6.0 of that M; wsum is the 'valid' normaliser of a signal without NaN"""
    from scipy import signal
    M = int(smooth) + (1 - int(smooth) % 2)
    w = np.asarray(signal.windows.gaussian(M, (M - 1) / 6.0), dtype=np.float64)
    return w, float(np.convolve(w, np.ones(M), mode="valid")[0])


def _pack(chunks, st, margin, atac):
    from ..packing import PackedChunks
    from ..pipeline import _pack_fragments
    chroms = [c.chrom for c in chunks]
    starts = np.array([c.start for c in chunks], np.int64)
    ends = np.array([c.end for c in chunks], np.int64)
    offs, lpos, ilen = _pack_fragments(st, chroms, starts, ends, margin, atac)
    return PackedChunks(chunk_start=starts, chunk_len=(ends - starts).astype(np.int32), frag_off=offs, frag_lpos=lpos, frag_ilen=ilen,
                        bias_off=None, bias_log=None, chroms=chroms)


def write_track_file(path, chunks, bam, run, halo, lower, upper, atac, max_chunks=None, timing=None):
    """run(batch) -> track id, for every sub-batch of `chunks`; writes `path` (BGZF) and `path`.tbi.  `halo`: how far past a region
    the kernel reads fragment ends or centres (the packing margin covers it).  timing (a dict) gets the seconds of packing, of the
    device calls and of the writer, and the sub-batch count."""
    st = FragmentStore.open(bam)
    margin = max(int(upper), 1) + max(0, -int(lower)) + int(halo) + 2
    return write_packed_track_file(path, chunks, lambda sub: _pack(sub, st, margin, atac), run, max_chunks=max_chunks, timing=timing)


def write_packed_track_file(path, chunks, pack_chunks, run, max_chunks=None, timing=None):
    """write_track_file for any packer: pack_chunks(sub) -> the PackedChunks of a sub-batch (called on the prefetch threads), run(batch)
    -> the id of the track it filled (the batch's PackedChunks is batch.packed)."""
    from .. import get_context
    from ..pipeline import prefetch_map, sub_batches
    from ..writer import TrackFile, write_track_index
    ctx = get_context()
    t = timing if timing is not None else {}
    for k in ("pack_s", "device_s", "writer_s"):
        t.setdefault(k, 0.0)
    t.setdefault("sub_batches", 0)

    def pack(sub):
        t0 = time.perf_counter()
        pk = pack_chunks(sub)
        return pk, time.perf_counter() - t0

    out = TrackFile(path)
    for pk, dt in prefetch_map(pack, sub_batches(chunks, max_chunks=max_chunks or MAX_CHUNKS)):
        t["pack_s"] += dt
        t0 = time.perf_counter()
        b = ctx.upload(pk)
        try:
            tid = run(b)
            ctx.sync()
            t1 = time.perf_counter()
            t["device_s"] += t1 - t0
            z, info = b.format_track(tid, pk.chroms, pk.chunk_start, compress=True)
            if info["hard"]:        # values the device formatter leaves to the host (e.g. a huge --scale)
                out.append_values(pk.chroms, pk.chunk_start, pk.out_off, b.track(tid).astype(np.float64))
            else:
                out.append_members(z, info["index"])
            t["writer_s"] += time.perf_counter() - t1
        finally:
            b.free()
        t["sub_batches"] += 1
    t0 = time.perf_counter()
    out.close()
    write_track_index(path, [out.log()])
    t["writer_s"] += time.perf_counter() - t0
    return path

