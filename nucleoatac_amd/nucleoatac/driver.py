"""What the `occ`, `nuc` and `nfr` drivers share: the input prefetch, the phase clock, the writer thread behind the pipelined
executor and the gathering of its track files' record logs."""
import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor, wait

import numpy as np

from ..shard import env_rank_world, gather_in_chunk_order

# Track.write_track + bgzip on the GPU (natac_batch_format_track); NATAC_DEVICE_WRITER=0: the native host writer formats the tracks
DEVICE_WRITER = os.environ.get("NATAC_DEVICE_WRITER", "1") != "0"


class Phases(object):
    """wall-clock seconds per named phase (cheap: two perf_counter calls per phase)"""

    def __init__(self, store):
        self.store, self.clock = store, time.perf_counter
        store.clear()
        self.t = self.clock()

    def mark(self, name):
        now = self.clock()
        self.store[name] = round(self.store.get(name, 0.0) + now - self.t, 3)
        self.t = now


def prefetch_inputs(args):
    """start the loads that can run next to the FASTA index / BED reads of a driver's prologue"""
    if env_rank_world()[2] == 0 and isinstance(args.bam, str):      # the node's publishing rank
        from ..pyatac.fragments import FragmentStore
        FragmentStore.prefetch(args.bam)       # it decodes (shard.shared_fragment_store)
    if getattr(args, "fasta", None):
        from ..pyatac.seq import FastaStore
        FastaStore.prefetch(args.fasta)        # the genome loads on its own thread; the BED file only needs the record lengths


def chrom_ids(part):
    """(names, id of every chunk's chromosome in names) of a sub-batch, as writer.write_bed_rows takes them"""
    names = sorted(set(c.chrom for c in part))
    idx = {c: i for i, c in enumerate(names)}
    return names, np.array([idx[c.chrom] for c in part], dtype=np.int32)


class TrackWriter(threading.Thread):
    """consumes finished sub-batches in order on its own thread (run_occ.py:41-59 are the reference's writer processes): every
    track is appended to its writer.TrackFile -- finished BGZF members when Track.write_track + bgzip ran on the device, else through
    the native host writer --, then `extra(result)`, then the result's pinned buffers go back to the executor."""

    def __init__(self, files, track_of, extra):
        """files: name -> TrackFile, track_of: name -> track id.
        extra: a function of the result, or a pair (start, finish): start(result) -> state runs next to the result's file appends
        and before its buffers are released, finish(state) for sub-batch k only after start of sub-batch k + 1 (still in result
        order) -- whatever start handed to a worker pool has company before the writer waits for it"""
        threading.Thread.__init__(self, daemon=True)
        self.files, self.track_of, self.extra = files, track_of, extra
        self.two_phase = isinstance(extra, tuple)
        self._pending = None
        self.q = queue.Queue(maxsize=2)
        self.err = None
        self.seconds = 0.0
        self.seconds_files = 0.0
        self.pool = ThreadPoolExecutor(max(1, len(files)) + 1, thread_name_prefix="natac-track-file")

    def run(self):
        while True:
            r = self.q.get()
            if r is None:
                return
            try:
                if self.err is None:
                    t0 = time.perf_counter()
                    part = r.tag
                    chroms, starts = [c.chrom for c in part], [c.start for c in part]

                    def write_one(name):
                        t = self.track_of[name]
                        z = r.text.get(t) if r.text else None
                        if z is not None:
                            self.files[name].append_members(z, r.text_index[t])
                        else:
                            self.files[name].append_values(chroms, starts, r.packed.out_off, r.tracks[t])

                    # one file per track: the appends run side by side (write() releases the GIL), every file still in order; the
                    # per-result extra work (peak rows / calls of THIS result, in result order) runs next to them
                    jobs = [self.pool.submit(write_one, n) for n in self.files]
                    more = self.pool.submit(self.extra[0] if self.two_phase else self.extra, r)
                    try:
                        for j in jobs:
                            j.result()
                        self.seconds_files += time.perf_counter() - t0
                    finally:                 # the result's buffers are released below: nothing may still be reading them
                        wait(jobs + [more])
                    state = more.result()
                    if self.two_phase:
                        r.release()          # start() has copied what finish() needs: the slot goes back before the wait
                        prev, self._pending = self._pending, state
                        if prev is not None:
                            self.extra[1](prev)
                    self.seconds += time.perf_counter() - t0
            except BaseException as e:      # noqa: BLE001 -- re-raised on the main thread
                self.err = e
            finally:
                r.release()

    def put(self, r):
        if self.err is not None:
            raise self.err
        self.q.put(r)

    def finish(self):
        self.q.put(None)
        self.join()
        self.pool.shutdown()
        if self.err is None and self._pending is not None:      # the last sub-batch's second half
            t0 = time.perf_counter()
            prev, self._pending = self._pending, None
            self.extra[1](prev)
            self.seconds += time.perf_counter() - t0
        if self.err is not None:
            raise self.err


def finish_tracks(files):
    """close this rank's track files (name -> TrackFile) and gather their logs: on rank 0 name -> [TrackFile.log() of rank 0, 1, ...],
    which is what writer.write_track_index takes once rank 0 has assembled the file; None on the other ranks"""
    for f in files.values():
        f.close()
    logs = gather_in_chunk_order([{n: f.log() for n, f in files.items()}], dst=0)
    return logs and {n: [l[n] for l in logs] for n in files}
