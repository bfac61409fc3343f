"""Fragment access + the four extractor functions of the reference's Cython module pyatac/fragments.pyx.

The reference re-opens the BAM and iterates `AlignmentFile.fetch` inside every call (fragments.pyx:21-25).
Here the alignment file is decoded ONCE into a FragmentStore (per chromosome: sorted leftmost positions and
template lengths of the forward proper-pair reads, which are the only reads the reference keeps,
fragments.pyx:25); the extractor functions keep the reference's names and argument order -- `bamfile` may be a
FragmentStore or a path (.bam / .npz, or a fragment file: .tsv / .tsv.gz / .bed / .bed.gz) -- and run on the GPU through the
C-ABI.
"""
import gzip
import os
import struct

import numpy as np

_CACHE = {}
_PENDING = {}     # src -> (thread, result box) of FragmentStore.prefetch
FRAGMENT_SUFFIXES = (".tsv", ".tsv.gz", ".bed", ".bed.gz")      # names FragmentStore._load reads as fragment files
# the fixed reason per cause of a malformed fragment line (csrc/natac_fragfile.hpp: reason_text)
_FRAG_REASONS = dict(fields="fewer than three tab-separated fields", empty="empty chromosome name",
                     long="chromosome name longer than 255 bytes", number="start / end is not a number",
                     range="start / end out of range (more than 2147483647)", order="end before start",
                     barcode="no barcode field")      # (only when splitting by barcode)


class CellTable(object):
    """the cells of a fragment file in order of first appearance (FragmentStore.discover_cells): barcodes (list of bytes), n_frag / n_nfr /
    n_mono (int64 arrays, one entry per cell), n_data (the file's data lines) and n_unassigned (those of no cell)"""

    def __init__(self, barcodes, n_frag, n_nfr, n_mono, n_data, n_unassigned):
        self.barcodes = list(barcodes)
        self.n_frag, self.n_nfr, self.n_mono = (np.ascontiguousarray(a, dtype=np.int64) for a in (n_frag, n_nfr, n_mono))
        self.n_data, self.n_unassigned = int(n_data), int(n_unassigned)

    def __len__(self):
        return len(self.barcodes)


class FragmentStore(object):
    """per-chromosome arrays of forward proper-pair reads: pos (leftmost coordinate, sorted), tlen (|template length|)"""

    def __init__(self, chroms, lengths, pos, tlen, trusted=False, cell=None):
        self.references = list(chroms)
        self.lengths = [int(x) for x in lengths]
        self.cell = None         # a cell-tagged store (from_fragments_cells): cell[chrom] int32, the cell of every record
        if cell is not None:
            if trusted:
                raise ValueError("a cell-tagged store is built from unsorted arrays")
            self.cell = {c: np.ascontiguousarray(cell[c], dtype=np.int32) for c in self.references}
        if trusted:      # arrays published by another FragmentStore (shard.shared_fragment_store): already int64, |tlen|, sorted
            self.pos = {c: pos[c] for c in self.references}
            self.tlen = {c: tlen[c] for c in self.references}
            self.max_tlen = max([int(t.max()) for t in self.tlen.values() if len(t)] + [0])
            return
        self.pos = {c: np.ascontiguousarray(pos[c], dtype=np.int64) for c in self.references}
        self.tlen = {c: np.ascontiguousarray(np.abs(tlen[c]), dtype=np.int64) for c in self.references}
        for c in self.references:
            if len(self.pos[c]) > 1 and np.any(np.diff(self.pos[c]) < 0):
                o = np.argsort(self.pos[c], kind="stable")
                self.pos[c], self.tlen[c] = self.pos[c][o], self.tlen[c][o]
                if self.cell is not None:
                    self.cell[c] = self.cell[c][o]
        self.max_tlen = max([int(t.max()) for t in self.tlen.values() if len(t)] + [0])

    def chrom_sizes(self):
        return dict(zip(self.references, self.lengths))

    @staticmethod
    def prefetch(src):
        """start decoding `src` on a thread (the drivers call this first thing: the BAM decode -- native code, GIL released --
        runs while the main thread reads the FASTA index and the BED file); FragmentStore.open(src) waits for it"""
        if isinstance(src, FragmentStore) or src in _CACHE or src in _PENDING:
            return
        import threading
        if os.environ.get("NATAC_DEVICE_BAM", "1") != "0" and str(src).endswith((".bam",) + FRAGMENT_SUFFIXES):
            from .. import get_context
            from ..device import Context
            if Context.device_count() > 0:
                get_context()               # the process-wide context is created on the caller's thread, not raced for
        box = {}

        def work():
            try:
                box["store"] = FragmentStore._load(src)
            except BaseException as e:      # noqa: BLE001 -- re-raised by open() on the caller's thread
                box["error"] = e
        t = threading.Thread(target=work, name="natac-bam-prefetch", daemon=True)
        _PENDING[src] = (t, box)
        t.start()

    @staticmethod
    def open(src):
        if isinstance(src, FragmentStore):
            return src
        if src in _PENDING:
            t, box = _PENDING.pop(src)
            t.join()
            if "error" in box:
                raise box["error"]
            _CACHE[src] = box["store"]
        if src in _CACHE:
            return _CACHE[src]
        _CACHE[src] = st = FragmentStore._load(src)
        return st

    @staticmethod
    def _load(src):
        if src.endswith(".npz"):
            st = FragmentStore.from_npz(src)
        elif src.endswith(".bam"):
            st = FragmentStore.from_bam(src)
        elif src.endswith(FRAGMENT_SUFFIXES):
            st = FragmentStore.from_fragments(src)
        else:
            raise ValueError("unsupported alignment source %r (expected FragmentStore, .bam, .npz or a fragment file: %s)"
                             % (src, ", ".join(FRAGMENT_SUFFIXES)))
        return st

    @staticmethod
    def register(src, store):
        """make FragmentStore.open(src) return `store` (a store built elsewhere, e.g. mapped from shared memory)"""
        _CACHE[src] = store

    @staticmethod
    def from_npz(path):
        d = np.load(path, allow_pickle=False)
        chroms = [str(x) for x in d["chrom_names"]]
        tagged = bool(chroms) and all("cell_" + c in d.files for c in chroms)      # written by a cell-tagged store
        return FragmentStore(chroms, d["chrom_lengths"], {c: d["pos_" + c] for c in chroms},
                             {c: d["tlen_" + c] for c in chroms}, cell={c: d["cell_" + c] for c in chroms} if tagged else None)

    def save_npz(self, path):
        arrs = dict(chrom_names=np.array(self.references), chrom_lengths=np.array(self.lengths))
        for c in self.references:
            arrs["pos_" + c] = self.pos[c]
            arrs["tlen_" + c] = self.tlen[c]
            if self.cell is not None:
                arrs["cell_" + c] = self.cell[c]
        np.savez_compressed(path, **arrs)

    @staticmethod
    def from_bam(path, n_threads=0, device=None):
        """native decoder in libnatac_hip.so.  On a GPU box: natac_bam_open_device (csrc/natac_bam_dev.hpp on the
        window stream of csrc/natac_bgzf_dev.hpp) -- the file goes to the
        device through two pinned staging buffers, every lane of the chip inflates BGZF members from a queue while the rest of
        the file is still being read, the records are walked on the device and the chain of record starts is confirmed link by
        link.  Without a GPU, or with device=False / NATAC_DEVICE_BAM=0: natac_bam_open, parallel inflate + record walk on the
        host cores.  Both give the same arrays.  Measured on the MI355X box (tools/bench_bam.py, 60 M records, 4.6 GB): device
        0.72 s; host 1.64 s with its 64 threads, 6.1 s with 4."""
        import ctypes as C
        from .. import _lib as L
        lib = L.load()
        h = C.c_void_p()
        if device is None:
            from ..device import Context
            device = os.environ.get("NATAC_DEVICE_BAM", "1") != "0" and Context.device_count() > 0
        if device:
            from .. import get_context
            on_dev = C.c_int(0)
            L.check(lib.natac_bam_open_device(get_context()._h, str(path).encode(), C.byref(h), C.byref(on_dev)))
            FragmentStore.last_bam_on_device = bool(on_dev.value)
        else:
            L.check(lib.natac_bam_open(str(path).encode(), int(n_threads), C.byref(h)))
            FragmentStore.last_bam_on_device = False
        return FragmentStore._from_handle(lib, h)

    @staticmethod
    def _from_handle(lib, h, cells=False):
        """the per-reference arrays of a natac_bam handle (natac_bam_open* / natac_frag_open*); closes the handle.  cells: the handle
        of a cell-tagged read, whose cell indices come along"""
        import ctypes as C
        from .. import _lib as L
        try:
            nref = C.c_int32(0)
            L.check(lib.natac_bam_counts(h, C.byref(nref), None, None))
            names, lens, pos, tl, ce = [], [], {}, {}, {}
            for r in range(nref.value):
                name = C.create_string_buffer(512)
                ln, nr = C.c_int64(0), C.c_int64(0)
                L.check(lib.natac_bam_ref_info(h, r, name, 512, C.byref(ln), C.byref(nr)))
                c = name.value.decode()
                if c in pos:
                    raise ValueError("two chromosomes read as %r" % (c,))      # (fragment-file names that differ only behind a NUL byte)
                p = np.empty(nr.value, dtype=np.int64)
                t = np.empty(nr.value, dtype=np.int64)
                L.check(lib.natac_bam_ref_reads(h, r, p.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), nr.value))
                if cells:
                    ce[c] = np.empty(nr.value, dtype=np.int32)
                    L.check(lib.natac_bam_ref_cells(h, r, ce[c].ctypes.data_as(C.c_void_p)))
                names.append(c)
                lens.append(ln.value)
                pos[c], tl[c] = p, t
        finally:
            lib.natac_bam_close(h)
        return FragmentStore(names, lens, pos, tl, cell=ce if cells else None)

    @staticmethod
    def from_fragments(path, n_threads=0, device=None, barcodes=None):
        """A fragment file (fragments.tsv.gz of Cell Ranger ATAC, the ENCODE pipeline, chromap, sinto, SnapATAC / ArchR) read by the
        native decoder.  The format rule (include/natac.h states it, csrc/natac_fragfile.hpp: parse_line is it):

        - lines end in "\\n", a "\\r" directly before it is dropped, a last line without "\\n" is a line; empty lines and lines
          whose first byte is "#" (the 10x header) are skipped;
        - every other line is a data line: TAB-separated, at least three fields, fields after the third ignored whatever they hold
          (barcode, duplicate count: one line is one fragment, identical lines are separate fragments); chrom is 1-255 bytes, start
          and end are 1-10 ASCII digits without sign or blanks, at most 2**31 - 1, end >= start;
        - [start, end) is taken as the insertion-to-insertion interval the reference's ATAC offsets produce
          (pyatac/fragments.pyx:26-31: l = start, ilen = end - start): the stored record is pos = start - 4 (may be negative),
          tlen = end - start + 8; end == start is kept.  Files written with the +4/-5 convention are one base shorter at the right
          end than the reference's +4/-4 reading of the same BAM; nothing is corrected, because the writer's convention is not
          recorded in the file;
        - chromosomes are numbered in order of first appearance (one that comes back later keeps its id); there is no sequence
          dictionary, so a chromosome's length is the largest end on it (commands given --fasta take sizes from the FASTA);
        - a malformed data line raises "<path>: line <N>: <reason>" (N 1-based, counting skipped lines), nothing is returned.

        The container goes by magic bytes: BGZF, any other gzip, plain text.  On a GPU box a BGZF file goes through
        natac_frag_open_device (csrc/natac_fragfile_dev.hpp, PlainJob): the members are staged and inflated by the BAM path's window
        stream (csrc/natac_bgzf_dev.hpp), then the text is split
        into lines, parsed and compacted on the device; FragmentStore.last_frag_on_device tells whether the device answered (the host
        decoder answers inside the call for another container, a malformed line, a damaged file, a line longer than a window, more
        than 65,536 chromosome runs in a window).  Without a GPU, or with device=False / NATAC_DEVICE_BAM=0: natac_frag_open, parallel
        inflate and parse over line-aligned slices on the host cores.  Both give the same arrays.
        Measured on the MI355X box (tools/bench_bam.py 20000000 --fragments, one box): a 20 M-record BAM's 10.0 M kept reads as a fragment
        file (436 MB of text, 129 MB BGZF): device 0.15 s; host 0.26 s with 16 threads, 0.50 s with 4; the device decode of the BAM itself
        (1.25 GB) 0.28 s.

        With `barcodes` (an iterable of cell barcodes) only the lines of those cells are kept: the one-group case of split_fragments,
        under its rule (every data line then needs a fourth field)."""
        if barcodes is not None:
            barcodes = list(barcodes)
            return FragmentStore.split_fragments(path, barcodes, [0] * len(barcodes), 1, n_threads=n_threads, device=device)[0][0]
        import ctypes as C
        from .. import _lib as L
        lib = L.load()
        h = C.c_void_p()
        if device is None:
            from ..device import Context
            device = os.environ.get("NATAC_DEVICE_BAM", "1") != "0" and Context.device_count() > 0
        if device:
            from .. import get_context
            on_dev = C.c_int(0)
            L.check(lib.natac_frag_open_device(get_context()._h, str(path).encode(), C.byref(h), C.byref(on_dev)))
            FragmentStore.last_frag_on_device = bool(on_dev.value)
        else:
            L.check(lib.natac_frag_open(str(path).encode(), int(n_threads), C.byref(h)))
            FragmentStore.last_frag_on_device = False
        return FragmentStore._from_handle(lib, h)

    @staticmethod
    def split_fragments(path, barcodes, group_of, n_groups, n_threads=0, device=None):
        """One pass over a fragment file that yields one FragmentStore per cell group (a cluster, a sample, a QC whitelist): per-cluster
        pseudo-bulk without filtering the text once per cluster.  barcodes[k] (bytes or str, 1-255 bytes, distinct) belongs to group
        group_of[k] in [0, n_groups).  Returns (stores, bc_count, n_unassigned): n_groups stores, the data lines per listed barcode
        (int64) and the data lines in no group.  The split rule (include/natac.h states it, csrc/natac_fragfile.hpp: split_line is it):

        - every line is validated exactly as by from_fragments; a data line with fewer than four fields is malformed as well
          ("no barcode field", checked last);
        - the barcode is the fourth field, compared byte for byte (no trimming, no case folding, a "-1" suffix is part of it); a line
          whose barcode is empty, longer than 255 bytes or not listed is unassigned: validated, counted, in no group, no error;
        - every store has the same chromosome list (first appearance over ALL data lines) and the same lengths (largest end over all
          data lines), so groups are comparable; a chromosome on which a group has nothing is present and empty;
        - a group's records are its lines in file order within each chromosome (then sorted stably by the FragmentStore, like any).

        On a GPU box a BGZF file goes through natac_frag_split_device (csrc/natac_fragfile_dev.hpp, SplitJob): the barcode of every data
        line is
        hashed, looked up and counted on the device and each window's assigned lines are partitioned by group there;
        FragmentStore.last_frag_on_device tells whether the device answered (the host path answers inside the call for everything
        from_fragments hands over, a line without a barcode field, a table of more than 4,194,304 barcodes and more than 1,048,576
        groups x chromosome runs in a window).  Both paths give the same arrays.
        Measured on the MI355X box (tools/bench_bam.py 20000000 --split, one run): 10.0 M lines, 9,000 of 10,000 cells listed, 127 MB BGZF,
        into 1 / 16 / 255 groups: device 0.20 / 0.16 / 0.15 s; host 0.51 / 0.48 / 0.53 s with 16 threads, 1.06 / 1.17 / 1.27 s with 4; the
        plain device decode of the same file 0.15 / 0.15 / 0.13 s."""
        import ctypes as C
        from .. import _lib as L
        lib = L.load()
        bcs = [b.encode() if isinstance(b, str) else bytes(b) for b in barcodes]
        group_of = np.ascontiguousarray(group_of, dtype=np.int32)
        n_groups = int(n_groups)
        if len(group_of) != len(bcs):
            raise ValueError("barcodes and group_of differ in length")
        if not 1 <= n_groups <= 255:                              # NATAC_SPLIT_MAX_GROUPS: the handle array below is sized by it
            raise ValueError("n_groups must be in [1, 255]")
        off = np.zeros(len(bcs) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in bcs], out=off[1:])
        blob = np.frombuffer(b"".join(bcs) + b"\0", dtype=np.uint8)
        handles = (C.c_void_p * n_groups)()
        bc_count = np.zeros(len(bcs), dtype=np.int64)
        n_un = C.c_int64(0)
        table = (len(bcs), blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), group_of.ctypes.data_as(C.c_void_p), n_groups,
                 C.cast(handles, C.c_void_p), bc_count.ctypes.data_as(C.c_void_p), C.cast(C.pointer(n_un), C.c_void_p))
        if device is None:
            from ..device import Context
            device = os.environ.get("NATAC_DEVICE_BAM", "1") != "0" and Context.device_count() > 0
        if device:
            from .. import get_context
            on_dev = C.c_int(0)
            L.check(lib.natac_frag_split_device(get_context()._h, str(path).encode(), *table, C.byref(on_dev)))
            FragmentStore.last_frag_on_device = bool(on_dev.value)
        else:
            L.check(lib.natac_frag_split(str(path).encode(), int(n_threads), *table))
            FragmentStore.last_frag_on_device = False
        stores, failed = [], None
        for g in range(n_groups):                                 # (_from_handle closes its handle, also when it raises)
            try:
                stores.append(FragmentStore._from_handle(lib, C.c_void_p(handles[g])))
            except BaseException as e:      # noqa: BLE001 -- the other handles are still closed, then it is raised
                failed = failed or e
        if failed is not None:
            raise failed
        return stores, bc_count, int(n_un.value)

    @staticmethod
    def _barcode_table(barcodes):
        """(barcodes as bytes, the ctypes arguments n_barcodes, bc_bytes, bc_off, and the arrays that keep them alive)"""
        import ctypes as C
        bcs = [b.encode() if isinstance(b, str) else bytes(b) for b in barcodes]
        off = np.zeros(len(bcs) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in bcs], out=off[1:])
        blob = np.frombuffer(b"".join(bcs) + b"\0", dtype=np.uint8)
        return bcs, (len(bcs), blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p)), (blob, off)

    @staticmethod
    def from_fragments_cells(path, barcodes, n_threads=0):
        """A cell-tagged read of a fragment file: the one-group case of split_fragments, under its rule, that also keeps which cell
        every kept record belongs to.  Returns (store, bc_count, n_unassigned): store.cell[chrom] (int32) holds, per record, the index
        of its barcode in `barcodes` (bytes or str, 1-255 bytes, distinct), permuted together with pos and tlen by the store's stable
        sort; the chromosome list and lengths come from ALL data lines; bc_count / n_unassigned as split_fragments.  What
        Context.region_cell_counts and `pyatac cellcounts` read.
        The host decoder answers (natac_frag_open_cells): it reads 10 M lines in 0.26-0.5 s by the figures of from_fragments, and a
        device variant of this read is not part of the package.  A tagged store is not registered with FragmentStore.open."""
        import ctypes as C
        from .. import _lib as L
        lib = L.load()
        bcs, table, _keep = FragmentStore._barcode_table(barcodes)
        h = C.c_void_p()
        bc_count = np.zeros(len(bcs), dtype=np.int64)
        n_un = C.c_int64(0)
        L.check(lib.natac_frag_open_cells(str(path).encode(), int(n_threads), *table, C.byref(h), bc_count.ctypes.data_as(C.c_void_p),
                                          C.cast(C.pointer(n_un), C.c_void_p)))
        return FragmentStore._from_handle(lib, h, cells=True), bc_count, int(n_un.value)

    @staticmethod
    def cells_fragments_python(path, barcodes):
        """pure-Python restatement of from_fragments_cells, kept as an independent check of the native path"""
        bcs = [b.encode() if isinstance(b, str) else bytes(b) for b in barcodes]
        index = {b: k for k, b in enumerate(bcs)}
        if len(index) != len(bcs):
            raise ValueError("a barcode is listed twice")
        names, length, pos, tl, cell = [], {}, {}, {}, {}
        bc_count = np.zeros(len(bcs), dtype=np.int64)
        n_unassigned = 0
        for c, start, end, bc in FragmentStore._python_lines(path, need_barcode=True):
            if c not in length:
                names.append(c)
                length[c], pos[c], tl[c], cell[c] = 0, [], [], []
            length[c] = max(length[c], end)
            k = index.get(bc)
            if k is None:
                n_unassigned += 1
                continue
            bc_count[k] += 1
            pos[c].append(start - 4)
            tl[c].append(end - start + 8)
            cell[c].append(k)
        store = FragmentStore(names, [length[c] for c in names], {c: np.array(pos[c], np.int64) for c in names},
                              {c: np.array(tl[c], np.int64) for c in names}, cell={c: np.array(cell[c], np.int32) for c in names})
        return store, bc_count, n_unassigned

    @staticmethod
    def _python_lines(path, need_barcode=False):
        """the data lines of a fragment file by the format rule, restated in pure Python: (chrom, start, end, barcode) per data line;
        barcode is None unless need_barcode (the split rule: a data line then needs a fourth field, checked last)"""
        with open(path, "rb") as fh:
            zipped = fh.read(2) == b"\x1f\x8b"
        with (gzip.open if zipped else open)(path, "rb") as fh:
            lines = fh.read().split(b"\n")
        open_end = lines[-1] != b""          # the last line has no "\n" (and keeps a "\r")
        if not open_end:
            lines.pop()

        def bad(no, why):
            return ValueError("%s: line %d: %s" % (path, no, _FRAG_REASONS[why]))

        def coord(no, b):
            if not b or not b.isdigit():
                raise bad(no, "number")
            if len(b) > 10 or int(b) > 2 ** 31 - 1:
                raise bad(no, "range")
            return int(b)
        for no, line in enumerate(lines, 1):
            if line.endswith(b"\r") and not (open_end and no == len(lines)):
                line = line[:-1]
            if not line or line[:1] == b"#":
                continue
            f = line.split(b"\t")
            if len(f) < 3:
                raise bad(no, "fields")
            if not f[0]:
                raise bad(no, "empty")
            if len(f[0]) > 255:
                raise bad(no, "long")
            start = coord(no, f[1])
            end = coord(no, f[2])
            if end < start:
                raise bad(no, "order")
            if need_barcode and len(f) < 4:
                raise bad(no, "barcode")
            yield f[0].decode(), start, end, f[3] if need_barcode else None

    @staticmethod
    def from_fragments_python(path):
        """pure-Python restatement of the format rule of from_fragments, kept as an independent check of the native decoders"""
        names, pos, tl, length = [], {}, {}, {}
        for c, start, end, _ in FragmentStore._python_lines(path):
            if c not in pos:
                names.append(c)
                pos[c], tl[c], length[c] = [], [], 0
            pos[c].append(start - 4)
            tl[c].append(end - start + 8)
            length[c] = max(length[c], end)
        return FragmentStore(names, [length[c] for c in names], {c: np.array(pos[c], np.int64) for c in names},
                             {c: np.array(tl[c], np.int64) for c in names})

    @staticmethod
    def split_fragments_python(path, barcodes, group_of, n_groups):
        """pure-Python restatement of the split rule of split_fragments, kept as an independent check of the native paths"""
        bcs = [b.encode() if isinstance(b, str) else bytes(b) for b in barcodes]
        index = {b: k for k, b in enumerate(bcs)}
        if len(index) != len(bcs):
            raise ValueError("a barcode is listed twice")
        names, length = [], {}
        pos = [{} for _ in range(n_groups)]
        tl = [{} for _ in range(n_groups)]
        bc_count = np.zeros(len(bcs), dtype=np.int64)
        n_unassigned = 0
        for c, start, end, bc in FragmentStore._python_lines(path, need_barcode=True):
            if c not in length:
                names.append(c)
                length[c] = 0
            length[c] = max(length[c], end)
            k = index.get(bc)              # (an empty barcode and one longer than 255 bytes cannot be listed)
            if k is None:
                n_unassigned += 1
                continue
            bc_count[k] += 1
            g = int(group_of[k])
            pos[g].setdefault(c, []).append(start - 4)
            tl[g].setdefault(c, []).append(end - start + 8)
        stores = [FragmentStore(names, [length[c] for c in names], {c: np.array(pos[g].get(c, []), np.int64) for c in names},
                                {c: np.array(tl[g].get(c, []), np.int64) for c in names}) for g in range(n_groups)]
        return stores, bc_count, n_unassigned

    @staticmethod
    def discover_cells(path, nfr_upper=147, mono_upper=294, n_threads=0, device=None):
        """Which cells a fragment file holds, with per-cell QC counts, in one pass: the barcode table that split_fragments and
        from_fragments_cells take, built from the file itself.  Returns a CellTable.  The cells rule (include/natac.h states it,
        csrc/natac_fragfile.hpp: barcode_line is it):

        - every line is validated exactly as by split_fragments (the same checks, order, reasons and line numbers, "no barcode field"
          checked last), and the barcode is the fourth field as the split rule defines it, byte for byte;
        - a data line whose barcode is 1-255 bytes long belongs to the cell of that barcode; cells are numbered in order of first
          appearance over the file's data lines (file order, not hash or thread order); a data line whose barcode is empty or longer
          than 255 bytes is unassigned: validated, counted in n_unassigned, no error;
        - with ilen = end - start, cell k has three exact int64 counters: n_frag[k] its data lines, n_nfr[k] those with
          ilen < nfr_upper, n_mono[k] those with nfr_upper <= ilen < mono_upper; 0 < nfr_upper < mono_upper (the defaults, 147 and
          294, are the usual nucleosome-free and mono-nucleosome classes of single-cell ATAC QC: defaults of a flag, not measured
          values); one line is one fragment whatever its fifth column says;
        - more than 8,388,608 distinct barcodes fail the call with a message naming the line at which the limit was passed;
        - the result is a function of the file's bytes and the two bounds only: not of n_threads, the windows, the BGZF member size, the
          container, or which path answered.

        With device=True a BGZF file goes through natac_frag_cells_device (csrc/natac_fragfile_dev.hpp, CellsJob): the text is inflated and
        split
        into lines on the device, and the table is built there from the file itself -- an open-addressing table of FIXED size (8,388,608
        slots, at most half of them taken) in device memory that lives across windows; a slot is claimed by the smallest line of a window
        and only matches after the bytes compared equal.  FragmentStore.last_frag_on_device tells whether the device answered (the host
        path answers inside the call for everything from_fragments hands over, a line without a barcode field, a full table -- more
        than 4,194,304 barcodes --, more than 268,435,455 lines in a window and a HIP failure).  Both paths give the same table.
        Measured on the MI355X box (tools/bench_bam.py 20000000 --cells, one box, one run): the 10.0 M lines and 10,000 cells of the
        split's file, 127 MB BGZF: device 0.094 s and, called again, 0.088 s; host 0.47 s with 16 threads, 0.76 s with 4; the plain
        device decode of the same file 0.13 s (it brings every record back, this call only the table).  The device is the faster
        path there, so device=None takes it on a GPU box as split_fragments does (NATAC_DEVICE_BAM=0: the host)."""
        import ctypes as C
        from .. import _lib as L
        lib = L.load()
        h = C.c_void_p()
        if device is None:
            from ..device import Context
            device = os.environ.get("NATAC_DEVICE_BAM", "1") != "0" and Context.device_count() > 0
        if device:
            from .. import get_context
            on_dev = C.c_int(0)
            L.check(lib.natac_frag_cells_device(get_context()._h, str(path).encode(), int(nfr_upper), int(mono_upper), C.byref(h), C.byref(on_dev)))
            FragmentStore.last_frag_on_device = bool(on_dev.value)
        else:
            L.check(lib.natac_frag_cells(str(path).encode(), int(n_threads), int(nfr_upper), int(mono_upper), C.byref(h)))
            FragmentStore.last_frag_on_device = False
        try:
            n, nb, nd, nu = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
            L.check(lib.natac_cells_counts(h, C.byref(n), C.byref(nb), C.byref(nd), C.byref(nu)))
            blob = np.zeros(nb.value + 1, dtype=np.uint8)
            off = np.zeros(n.value + 1, dtype=np.int64)
            counts = [np.zeros(n.value, dtype=np.int64) for _ in range(3)]
            L.check(lib.natac_cells_read(h, n.value, nb.value, blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                         *[a.ctypes.data_as(C.c_void_p) for a in counts]))
        finally:
            lib.natac_cells_close(h)
        raw, o = blob.tobytes(), off.tolist()
        return CellTable([raw[a:b] for a, b in zip(o[:-1], o[1:])], counts[0], counts[1], counts[2], nd.value, nu.value)

    @staticmethod
    def discover_cells_python(path, nfr_upper=147, mono_upper=294):
        """pure-Python restatement of the cells rule of discover_cells, kept as an independent check of the native paths"""
        if not 0 < nfr_upper < mono_upper:
            raise ValueError("0 < nfr_upper < mono_upper does not hold")
        index, counts = {}, []
        n_data = n_unassigned = 0
        for _, start, end, bc in FragmentStore._python_lines(path, need_barcode=True):
            n_data += 1
            if not 1 <= len(bc) <= 255:
                n_unassigned += 1
                continue
            k = index.setdefault(bc, len(counts))
            if k == len(counts):
                counts.append([0, 0, 0])
            ilen = end - start
            counts[k][0] += 1
            if ilen < nfr_upper:
                counts[k][1] += 1
            elif ilen < mono_upper:
                counts[k][2] += 1
        c = np.array(counts, dtype=np.int64).reshape(-1, 3)
        return CellTable(list(index), c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(), n_data, n_unassigned)

    def save_fragments(self, path):
        """write the store as a fragment file (chrom, start = pos + 4, end = pos + tlen - 4 per line, in the store's order: chromosome
        by chromosome, sorted by start), BGZF-compressed by natac_bgzip_file with its .tbi by natac_tabix_index: a BAM converted once
        reads back as the same pos / tlen arrays through from_fragments"""
        from ..writer import bgzip_file, tabix_index
        tmp = str(path) + ".tmp"
        with open(tmp, "w") as fh:
            for c in self.references:
                start, end = self.pos[c] + 4, self.pos[c] + self.tlen[c] - 4
                if len(start) and (int(start.min()) < 0 or bool(np.any(end < start)) or int(end.max()) > 2 ** 31 - 1):
                    os.remove(tmp)
                    raise ValueError("%s holds a read a fragment line cannot carry (pos < -4, |tlen| < 8 or an end beyond 2**31 - 1)" % c)
                row = c + "\t%d\t%d\n"
                for o in range(0, len(start), 1 << 16):
                    fh.write("".join([row % se for se in zip(start[o:o + (1 << 16)].tolist(), end[o:o + (1 << 16)].tolist())]))
        bgzip_file(tmp, str(path))
        tabix_index(str(path))
        return str(path)

    @staticmethod
    def from_bam_python(path):
        """pure-Python BGZF/BAM decoder (SAM spec section 4), kept as an independent check of the native one:
        keeps FLAG & 0x2 (proper pair) and not FLAG & 0x10 (reverse)"""
        with gzip.open(path, "rb") as fh:
            b = fh.read()
        if b[:4] != b"BAM\x01":
            raise ValueError("%s is not a BAM file" % path)
        o = 8 + struct.unpack_from("<i", b, 4)[0]
        n_ref = struct.unpack_from("<i", b, o)[0]
        o += 4
        names, lens = [], []
        for _ in range(n_ref):
            ln = struct.unpack_from("<i", b, o)[0]
            names.append(b[o + 4:o + 3 + ln].decode())
            lens.append(struct.unpack_from("<i", b, o + 4 + ln)[0])
            o += 8 + ln
        pos = {c: [] for c in names}
        tl = {c: [] for c in names}
        nb = len(b)
        while o + 36 <= nb:
            bs, ref_id, p = struct.unpack_from("<iii", b, o)
            flag = struct.unpack_from("<H", b, o + 18)[0]
            tlen = struct.unpack_from("<i", b, o + 32)[0]
            if ref_id >= 0 and (flag & 0x2) and not (flag & 0x10):
                pos[names[ref_id]].append(p)
                tl[names[ref_id]].append(tlen)
            o += 4 + bs
        return FragmentStore(names, lens, {c: np.array(pos[c], np.int64) for c in names},
                             {c: np.array(tl[c], np.int64) for c in names})

    @staticmethod
    def from_arrays(chrom_sizes, l, n, atac=True):
        """build from already shifted fragments (l = pos+4, n = |tlen|-8 when atac)"""
        sh, d = (4, 8) if atac else (0, 0)
        chroms = list(chrom_sizes.keys())
        return FragmentStore(chroms, [chrom_sizes[c] for c in chroms],
                             {c: np.asarray(l.get(c, []), np.int64) - sh for c in chroms},
                             {c: np.asarray(n.get(c, []), np.int64) + d for c in chroms})

    def fetch(self, chrom, start, end, atac=1):
        """(l, n) of every read that can matter for [start, end): superset of htslib's overlap fetch
        (fragments.pyx:24); l = pos+4, n = |tlen|-8 when atac (fragments.pyx:26-34)"""
        if chrom not in self.pos:
            return np.zeros(0, np.int64), np.zeros(0, np.int32)
        p = self.pos[chrom]
        a = int(np.searchsorted(p, start - 1024, "left"))
        b = int(np.searchsorted(p, end, "left"))
        if atac:
            return p[a:b] + 4, (self.tlen[chrom][a:b] - 8).astype(np.int32)
        return p[a:b].copy(), self.tlen[chrom][a:b].astype(np.int32)

    def all_fragments(self, chrom, atac=1):
        return self.fetch(chrom, -(1 << 40), 1 << 40, atac)


def _ctx():
    from .. import get_context
    return get_context()


def makeFragmentMat(bamfile, chrom, start, end, lower, upper, atac=1):
    """V-plot count matrix (upper-lower) x (end-start) -- pyatac/fragments.pyx:17-40"""
    l, n = FragmentStore.open(bamfile).fetch(chrom, max(0, start - upper), end + upper, atac)
    return _ctx().make_fragment_mat(l, n, start, end, lower, upper)


def getInsertions(bamfile, chrom, start, end, lower, upper, atac=1):
    """per-base Tn5 insertion counts -- pyatac/fragments.pyx:43-67"""
    l, n = FragmentStore.open(bamfile).fetch(chrom, max(0, start - upper), end + upper, atac)
    return _ctx().get_insertions(l, n, start, end, lower, upper)


def getStrandedInsertions(bamfile, chrom, start, end, lower, upper, atac=1):
    """(plus, minus) = insertions at the left / right fragment ends -- pyatac/fragments.pyx:71-97"""
    l, n = FragmentStore.open(bamfile).fetch(chrom, max(0, start - upper), end + upper, atac)
    return _ctx().get_stranded_insertions(l, n, start, end, lower, upper)


def getAllFragmentSizes(bamfile, lower, upper, atac=1):
    """insert-size histogram of the whole file -- pyatac/fragments.pyx:101-119"""
    st = FragmentStore.open(bamfile)
    sizes = np.zeros(upper - lower, dtype=np.float64)
    for c, ln in zip(st.references, st.lengths):
        l, n = st.all_fragments(c, atac)
        if len(l):
            big = 1 << 40
            sizes += _ctx().fragment_sizes(l, n, [-big], [big], lower, upper)
    return sizes


def getFragmentSizesFromChunkList(chunks, bamfile, lower, upper, atac=1):
    """insert-size histogram of fragments centred in the chunks -- pyatac/fragments.pyx:123-145
    (a fragment counts once per chunk that contains its centre)"""
    st = FragmentStore.open(bamfile)
    sizes = np.zeros(upper - lower, dtype=np.float64)
    by_chrom = {}
    for ch in chunks:
        by_chrom.setdefault(ch.chrom, []).append((ch.start, ch.end))
    for c, iv in by_chrom.items():
        iv.sort()
        lo, hi = iv[0][0], max(e for _, e in iv)
        l, n = st.fetch(c, max(0, lo - upper), hi + upper, atac)
        if len(l):
            sizes += _ctx().fragment_sizes(l, n, [s for s, _ in iv], [e for _, e in iv], lower, upper)
    return sizes
