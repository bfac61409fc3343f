"""Throughput of the native BAM extractor (csrc/natac_bam.hpp: natac_bam_open decodes every record, keeps the forward reads of
proper pairs) on a synthetic coordinate-sorted BAM of N paired-end records with realistic record sizes (50-base reads, names of
~20 characters, one 50M cigar; BGZF members of 0xff00 bytes at zlib level 6 like samtools):  python tools/bench_bam.py 4000000
With --fragments, after the BAM run: the fragment file of the same BAM's kept reads (chrom, start, end, a 16-base barcode, a count; the
same members and level) through natac_frag_open_device and through natac_frag_open at 16 and at 4 threads, on the same box.
With --split, after the BAM run: the same kept reads as a single-cell fragment file (barcodes drawn from a pool of 10,000 cells, 90 % of
them listed, assigned round-robin to G = 1, 16 and 255 groups) through natac_frag_split_device, natac_frag_split at 16 and at 4 threads,
and the plain device decode of that same file, in the same run.
With --cells, after the BAM run: that same single-cell file (10,000 cells) through natac_frag_cells_device, natac_frag_cells at 16 and at
4 threads, and the plain device decode of the same file, in the same run."""
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_bam(path, n, n_refs=4, ref_len=50_000_000, seed=0):
    rng = np.random.default_rng(seed)
    text = b"@HD\tVN:1.0\tSO:coordinate\n"
    head = [b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_refs)]
    for r in range(n_refs):
        nm = ("chr%d" % (r + 1)).encode() + b"\0"
        head.append(struct.pack("<i", len(nm)) + nm + struct.pack("<i", ref_len))
    seq_len, name_len = 50, 20
    rec = np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("lname", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("ncig", "<u2"),
                    ("flag", "<u2"), ("lseq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4"), ("name", "S%d" % name_len),
                    ("cigar", "<u4"), ("seq", "u1", (seq_len + 1) // 2), ("qual", "u1", seq_len)])
    a = np.zeros(n, dtype=rec)
    a["bs"] = rec.itemsize - 4
    a["ref"] = np.sort(rng.integers(0, n_refs, n))
    pos = rng.integers(0, ref_len - 1000, n)
    order = np.lexsort((pos, a["ref"]))
    a["pos"] = pos[order]
    a["lname"], a["mapq"], a["ncig"], a["lseq"] = name_len, 30, 1, seq_len
    fwd = rng.random(n) < 0.5
    a["flag"] = np.where(fwd, 99, 147)                    # proper pair, first forward / second reverse
    a["nref"] = a["ref"]
    tl = rng.integers(40, 600, n)
    a["tlen"] = np.where(fwd, tl, -tl)
    a["npos"] = np.maximum(a["pos"] + np.where(fwd, tl - seq_len, -(tl - seq_len)), 0)
    a["name"] = np.char.add(b"read", np.arange(n).astype("S15"))
    a["cigar"] = seq_len << 4
    a["seq"] = rng.integers(0, 256, (n, (seq_len + 1) // 2), dtype=np.uint8)
    a["qual"] = rng.integers(20, 41, (n, seq_len), dtype=np.uint8)
    bgzf_write(path, b"".join(head) + a.tobytes())
    return a.nbytes + sum(len(h) for h in head), int(fwd.sum())


def bgzf_write(path, data):
    def member(o):
        chunk = data[o:o + 0xff00]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        return (bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(comp) + 8 - 1) + comp +
                struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk)))
    with ThreadPoolExecutor(os.cpu_count() or 4) as pool, open(path, "wb") as f:
        for m in pool.map(member, range(0, len(data), 0xff00)):
            f.write(m)
        f.write(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))


def bench_fragments(d, store):
    """the fragment file of `store` (what the BAM run decoded): device twice (the first call pays the first launches), host at 16 and 4"""
    from nucleoatac_amd.device import Context
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    rng = np.random.default_rng(1)
    parts = [b"# id=bench\n"]
    for c in store.references:
        start, end = (store.pos[c] + 4).tolist(), (store.pos[c] + store.tlen[c] - 4).tolist()
        bc = rng.integers(0, 4, (len(start), 16), dtype=np.uint8)
        bc = np.frombuffer(b"ACGT", dtype=np.uint8)[bc].view("S16").ravel().tolist()
        row = c.encode() + b"\t%d\t%d\t%s-1\t1\n"
        parts.append(b"".join([row % t for t in zip(start, end, bc)]))
    text = b"".join(parts)
    path = os.path.join(d, "fragments.tsv.gz")
    bgzf_write(path, text)
    size, n = os.path.getsize(path), sum(len(store.pos[c]) for c in store.references)
    print("fragment file: %d lines, %.0f MB of text, %.0f MB compressed" % (n, len(text) / 1e6, size / 1e6))
    modes = ([(0, True), (0, True)] if Context.device_count() > 0 else []) + [(16, False), (4, False)]
    for threads, device in modes:
        t0 = time.perf_counter()
        st = FragmentStore.from_fragments(path, n_threads=threads, device=device)
        dt = time.perf_counter() - t0
        if device:
            threads = "device" if FragmentStore.last_frag_on_device else "device->host"
        same = all(np.array_equal(st.pos[c], store.pos[c]) and np.array_equal(st.tlen[c], store.tlen[c]) for c in st.references)
        print("fragments threads=%s  %d lines (same arrays as the BAM: %s): %.2f s = %.1f M lines/s, %.0f MB/s compressed, %.0f MB/s inflated"
              % (threads, n, same, dt, n / dt / 1e6, size / dt / 1e6, len(text) / dt / 1e6))


def single_cell_file(d, store):
    """the kept reads of `store` as a single-cell fragment file -> (path, lines, cells, the 90 % of them a split lists)"""
    rng = np.random.default_rng(2)
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (10000, 16), dtype=np.uint8)].view("S16").ravel()
    pool = np.unique(pool)
    cells = [c + b"-1" for c in pool.tolist()]
    listed = cells[:len(cells) * 9 // 10]
    parts = [b"# id=bench\n"]
    for c in store.references:
        start, end = (store.pos[c] + 4).tolist(), (store.pos[c] + store.tlen[c] - 4).tolist()
        bc = pool[rng.integers(0, len(pool), len(start))].tolist()
        row = c.encode() + b"\t%d\t%d\t%s-1\t1\n"
        parts.append(b"".join([row % t for t in zip(start, end, bc)]))
    text = b"".join(parts)
    path = os.path.join(d, "cells.tsv.gz")
    bgzf_write(path, text)
    size, n = os.path.getsize(path), sum(len(store.pos[c]) for c in store.references)
    print("single-cell fragment file: %d lines, %d cells (%d listed), %.0f MB of text, %.0f MB compressed" % (n, len(cells), len(listed), len(text) / 1e6, size / 1e6))
    return path, n, cells, listed


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def bench_cells(d, store):
    """device discovery twice (the first call pays the first launches), host discovery at 16 and at 4 threads, the plain device decode"""
    from nucleoatac_amd.device import Context
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    path, n, cells, _ = single_cell_file(d, store)
    gpu = Context.device_count() > 0
    if gpu:
        FragmentStore.from_fragments(path, device=True)          # (the first call pays the first launches)
    row, ref = [], None
    for threads, device in ([(0, True), (0, True)] if gpu else []) + [(16, False), (4, False)]:
        table, dt = timed(lambda: FragmentStore.discover_cells(path, n_threads=threads, device=device))
        tag = ("device" if FragmentStore.last_frag_on_device else "device->host") if device else "host %d threads" % threads
        sig = (table.barcodes, table.n_frag.tolist(), table.n_nfr.tolist(), table.n_mono.tolist(), table.n_data, table.n_unassigned)
        ref = ref or sig
        row.append("%s %.3f s%s" % (tag, dt, "" if sig == ref else " (DIFFERS)"))
    if gpu:
        _, dt = timed(lambda: FragmentStore.from_fragments(path, device=True))
        row.append("plain device decode %.3f s" % dt)
    print("cells  %d lines, %d cells found (%d in the pool), %d unassigned: %s" % (n, len(ref[0]), len(cells), ref[5], ", ".join(row)))


def bench_split(d, store):
    """per G four times: device split, host split at 16 and at 4 threads, the plain device decode of the same file"""
    from nucleoatac_amd.device import Context
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    path, n, cells, listed = single_cell_file(d, store)
    gpu = Context.device_count() > 0
    if gpu:
        FragmentStore.from_fragments(path, device=True)          # (the first call pays the first launches)
    for G in (1, 16, 255):
        group_of = [k % G for k in range(len(listed))]
        row, ref = [], None
        for threads, device in ([(0, True)] if gpu else []) + [(16, False), (4, False)]:
            (stores, bc_count, n_un), dt = timed(lambda: FragmentStore.split_fragments(path, listed, group_of, G, n_threads=threads, device=device))
            tag = ("device" if FragmentStore.last_frag_on_device else "device->host") if device else "host %d threads" % threads
            sig = (n_un, int(bc_count.sum()), [sum(int(st.pos[c].sum()) for c in st.references) for st in stores])
            ref = ref or sig
            row.append("%s %.3f s%s" % (tag, dt, "" if sig == ref else " (DIFFERS)"))
        if gpu:
            _, dt = timed(lambda: FragmentStore.from_fragments(path, device=True))
            row.append("plain device decode %.3f s" % dt)
        print("split G=%d  %d lines, %d unassigned: %s" % (G, n, ref[0], ", ".join(row)))


def main():
    args = [a for a in sys.argv[1:] if a not in ("--fragments", "--split", "--cells")]
    n = int(args[0]) if args else 4_000_000
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    d = tempfile.mkdtemp(prefix="natac_bam_")
    path = os.path.join(d, "synth.bam")
    try:
        raw, kept = synth_bam(path, n)
        size = os.path.getsize(path)
        from nucleoatac_amd.device import Context
        modes = [(1, False), (4, False), (0, False)] + ([(0, True), (0, True)] if Context.device_count() > 0 else [])
        for threads, device in modes:
            t0 = time.perf_counter()
            st = FragmentStore.from_bam(path, n_threads=threads, device=device)
            dt = time.perf_counter() - t0
            if device:
                threads = "device" if FragmentStore.last_bam_on_device else "device->host"
                import ctypes as C
                from nucleoatac_amd import _lib as L, get_context
                h = C.c_void_p()
                t1 = time.perf_counter()
                L.check(L.load().natac_bam_open_device(get_context()._h, path.encode(), C.byref(h), None))
                print("   natac_bam_open_device alone: %.2f s" % (time.perf_counter() - t1))
                L.load().natac_bam_close(h)
            total = sum(len(st.pos[c]) for c in st.pos) if hasattr(st, "pos") else -1
            print("threads=%s  %d records, %d kept (expected %d): %.2f s = %.1f M records/s, %.0f MB/s compressed, %.0f MB/s inflated"
                  % (threads or "auto", n, total, kept, dt, n / dt / 1e6, size / dt / 1e6, raw / dt / 1e6))
        if "--fragments" in sys.argv:
            bench_fragments(d, st)
        if "--split" in sys.argv:
            bench_split(d, st)
        if "--cells" in sys.argv:
            bench_cells(d, st)
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
