"""Thin object layer over the C-ABI: one Context per GPU, DeviceBatch = packed chunks resident in HBM.

All numerics run in libnatac_hip.so (HIP, gfx950).  numpy is only used for the host buffers
that cross the boundary.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib as L
from .packing import PackedChunks


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class _PinnedOwner(object):
    """keeps a hipHostMalloc block alive for the numpy arrays that view it"""

    def __init__(self, nbytes):
        self._lib = L.load()
        p = C.c_void_p()
        L.check(self._lib.natac_host_alloc(int(nbytes), C.byref(p)))
        self.ptr, self.nbytes = p.value, int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                self._lib.natac_host_free(C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64):
    """numpy array in page-locked host memory (natac_host_alloc): PCIe transfers to / from it run at full rate.  The block
    is released when the last array viewing it dies: numpy collapses `.base` chains to the buffer exporter, so the owner is
    attached to that exporter (the ctypes array), not to an ndarray subclass."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if not np.isscalar(shape) else int(shape)
    owner = _PinnedOwner(max(1, n * dt.itemsize))
    buf = (C.c_char * owner.nbytes).from_address(owner.ptr)
    buf._natac_owner = owner
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)


def pinned_copy(a):
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


def pool_trim():
    L.check(L.load().natac_pool_trim())


def peaks_plan(max_len, order):
    """how the peak searches launch for a batch whose longest chunk has max_len bases (natac_peaks_plan; needs no GPU): dict of
    kernel ("reg" / "seg"), bt, nj (None for seg), mask ("registers" / "two_phase" / "direct", None for seg), global_lists,
    forms_smooth, pk_cap, lds_bytes and lds_bytes_smooth"""
    v = [C.c_int32() for _ in range(7)]
    lds = (C.c_int64 * 2)()
    L.check(L.load().natac_peaks_plan(int(max_len), int(order), *[C.byref(x) for x in v], lds))
    kernel, bt, nj, mask, gl, fs, cap = [x.value for x in v]
    seg = kernel == 1
    return dict(kernel="seg" if seg else "reg", bt=bt, nj=None if seg else nj, mask=None if seg else ("registers", "two_phase", "direct")[mask],
                global_lists=bool(gl), forms_smooth=bool(fs), pk_cap=cap, lds_bytes=lds[0], lds_bytes_smooth=lds[1])


def motif_deviations_plan(n_windows, n_cells, nnz, n_motifs, max_set, max_count, n_cu=256):
    """how motif_deviations launches for a matrix of n_windows x n_cells with nnz entries, n_motifs motifs the largest of max_set windows
    and the largest count max_count, on n_cu compute units (natac_motif_deviations_plan; needs no GPU, reads NATAC_DEVIATIONS_CELL_TILE as
    the call does): dict of tile, n_tiles, lanes, wide (64-bit counters) and lds_bytes"""
    tile, lanes, wide = C.c_int32(), C.c_int32(), C.c_int32()
    n_tiles, lds = C.c_int64(), C.c_int64()
    L.check(L.load().natac_motif_deviations_plan(int(n_windows), int(n_cells), int(nnz), int(n_motifs), int(max_set), int(max_count), int(n_cu),
                                                 C.byref(tile), C.byref(n_tiles), C.byref(lanes), C.byref(wide), C.byref(lds)))
    return dict(tile=tile.value, n_tiles=n_tiles.value, lanes=lanes.value, wide=bool(wide.value), lds_bytes=lds.value)


def group_rank_sums_plan(n_windows, n_cells, nnz, longest_row, n_groups, n_cu=256):
    """how group_rank_sums launches for a matrix of n_windows x n_cells with nnz entries whose longest row has longest_row entries, with
    n_groups groups on n_cu compute units (natac_group_rank_sums_plan; needs no GPU, reads NATAC_MARKERS_SHORT_MAX / NATAC_MARKERS_BLOCK_MAX
    as the call does): dict of short_max, block_max, lanes, chunk, and per arm ("short", "block", "long") wg and lds_bytes, and grid
    for the short and the block arm"""
    v = [C.c_int32() for _ in range(4)]
    wg, lds, grid = (C.c_int32 * 3)(), (C.c_int64 * 3)(), (C.c_int32 * 2)()
    L.check(L.load().natac_group_rank_sums_plan(int(n_windows), int(n_cells), int(nnz), int(longest_row), int(n_groups), int(n_cu),
                                                *[C.byref(x) for x in v], wg, lds, grid))
    arms = ("short", "block", "long")
    return dict(short_max=v[0].value, block_max=v[1].value, lanes=v[2].value, chunk=v[3].value, wg=dict(zip(arms, list(wg))),
                lds_bytes=dict(zip(arms, list(lds))), grid=dict(zip(arms, list(grid))))


def window_pair_sums_plan(n_windows, n_cells, nnz, n_listed, listed_entries, n_cu=256):
    """how window_pair_sums launches for a matrix of n_windows x n_cells with nnz entries of which n_listed windows are listed, with
    listed_entries entries between them, on n_cu compute units (natac_window_pair_sums_plan; needs no GPU, reads NATAC_COACCESS_TABLE_MAX /
    NATAC_COACCESS_CHUNK as the call does): dict of arm ("table" / "search"), table_max, lanes, chunk, wg, lds_bytes and grid"""
    v = [C.c_int32() for _ in range(5)]
    lds, grid = C.c_int64(), C.c_int32()
    L.check(L.load().natac_window_pair_sums_plan(int(n_windows), int(n_cells), int(nnz), int(n_listed), int(listed_entries), int(n_cu),
                                                 *([C.byref(x) for x in v] + [C.byref(lds), C.byref(grid)])))
    return dict(arm=("table", "search")[v[0].value], table_max=v[1].value, lanes=v[2].value, chunk=v[3].value, wg=v[4].value,
                lds_bytes=lds.value, grid=grid.value)


def gene_cell_scores_plan(n_genes, n_cells, table_rows, n_cu=256):
    """how gene_cell_scores launches for n_genes genes and n_cells cells of which table_rows rows take the table arm, on n_cu compute
    units (natac_gene_cell_scores_plan; needs no GPU, reads NATAC_GENESCORES_SHORT_MAX / NATAC_GENESCORES_TILE as the call does): dict of
    short_max, tile, n_tiles, wg, lds_bytes and grid"""
    v = [C.c_int32() for _ in range(4)]
    lds, grid = C.c_int64(), C.c_int32()
    L.check(L.load().natac_gene_cell_scores_plan(int(n_genes), int(n_cells), int(table_rows), int(n_cu),
                                                 *([C.byref(x) for x in v] + [C.byref(lds), C.byref(grid)])))
    return dict(short_max=v[0].value, tile=v[1].value, n_tiles=v[2].value, wg=v[3].value, lds_bytes=lds.value, grid=grid.value)


def knn_plan(nq, nr, dim, k, n_cu=256):
    """how knn launches for nq queries against nr references of dim columns with k neighbours on n_cu compute units (natac_knn_plan; needs
    no GPU, reads NATAC_KNN_WAVE_K_MAX / NATAC_KNN_QUERY_TILE / NATAC_KNN_REF_TILE as the call does): dict of arm ("wave" / "lds"),
    wave_k_max, query_tile, ref_tile, capacity, wg, lds_bytes and grid"""
    v = [C.c_int32() for _ in range(6)]
    lds, grid = C.c_int64(), C.c_int32()
    L.check(L.load().natac_knn_plan(int(nq), int(nr), int(dim), int(k), int(n_cu), *([C.byref(x) for x in v] + [C.byref(lds), C.byref(grid)])))
    return dict(arm=("wave", "lds")[v[0].value], wave_k_max=v[1].value, query_tile=v[2].value, ref_tile=v[3].value, capacity=v[4].value,
                wg=v[5].value, lds_bytes=lds.value, grid=grid.value)


class TrackStore(object):
    """device-resident copies of batch tracks as their .bedgraph file shows them (natac_store_*; see occstore.py)"""

    def __init__(self):
        self._lib = L.load()
        self._h = C.c_void_p()
        L.check(self._lib.natac_store_create(C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.natac_store_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001
            pass

    def set_budget(self, max_bytes=-1, min_free_bytes=-1):
        """HBM budget (natac_store_set_budget): the store stays below max_bytes and leaves min_free_bytes of the device to the
        pipeline's batches (defaults: no cap / a quarter of the device); the first refusal closes the store"""
        L.check(self._lib.natac_store_set_budget(self._h, int(max_bytes), int(min_free_bytes)))

    def adopt(self, batch, tracks, write_zero=True, keep_runs_before_nan=False):
        """copy `tracks` of `batch` into the store; returns the segment id, or None when a value cannot be rounded exactly on the
        device or the store's HBM budget declines the segment (nothing is kept then; the caller reads the files)"""
        t = np.ascontiguousarray(tracks, dtype=np.int32)
        seg, hard = C.c_int64(-1), C.c_int32(0)
        try:
            L.check(self._lib.natac_store_adopt(self._h, batch._h, len(t), _ptr(t), (1 if write_zero else 0) | (2 if keep_runs_before_nan else 0),
                                                C.byref(seg), C.byref(hard)))
        except L.NatacError as e:
            if e.code == -4:        # NATAC_E_NOMEM: HBM is full (24 bytes per base add up on a large genome) -- the files are there
                return None
            raise
        return None if seg.value < 0 else int(seg.value)

    def read(self, ctx, segment, offset, length, slot):
        sg, of, ln = (np.ascontiguousarray(a, dtype=np.int64) for a in (segment, offset, length))
        out = np.empty(int(ln.sum()), dtype=np.float64)
        L.check(self._lib.natac_store_read(self._h, ctx._h, len(sg), _ptr(sg), _ptr(of), _ptr(ln), int(slot), _ptr(out), out.size))
        return out

    def info(self):
        n, by = C.c_int64(0), C.c_int64(0)
        L.check(self._lib.natac_store_info(self._h, C.byref(n), C.byref(by)))
        d = C.c_int64(0)
        L.check(self._lib.natac_store_declined(self._h, C.byref(d)))
        return dict(segments=n.value, bytes=by.value, declined=d.value)


class Context(object):
    """one HIP device + stream (natac_ctx)"""

    def __init__(self, device_id=0):
        self._lib = L.load()
        h = C.c_void_p()
        L.check(self._lib.natac_ctx_create(int(device_id), C.byref(h)))
        self._h = h
        self.device_id = int(device_id)
        self.vmat_shape = None
        self.occ_step = None
        self._batches = weakref.WeakSet()

    def close(self):
        """destroy the context; batches that are still alive are freed first (they hold a pointer to it)"""
        if getattr(self, "_h", None):
            for b in list(self._batches):
                b.free()
            self._lib.natac_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def device_count():
        n = C.c_int(0)
        L.load().natac_device_count(C.byref(n))
        return n.value

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu = C.c_int(0)
        mem = C.c_size_t(0)
        L.check(self._lib.natac_ctx_device_info(self._h, name, 256, C.byref(ncu), C.byref(mem)))
        return dict(name=name.value.decode(), n_cu=ncu.value, mem_bytes=mem.value)

    def device_ids(self):
        """(HIP device ordinal, PCI bus id) of the GPU this context computes on"""
        dev = C.c_int(-1)
        buf = C.create_string_buffer(64)
        L.check(self._lib.natac_ctx_device_ids(self._h, C.byref(dev), buf, 64))
        return dev.value, buf.value.decode()

    def sync(self):
        L.check(self._lib.natac_ctx_sync(self._h))

    # ---- constants -------------------------------------------------------------------------
    def set_vmat(self, mat, lower, upper):
        """VMat template: mat (upper-lower, 2w+1) for insert sizes [lower, upper) (pyatac/VMat.py:24-37)."""
        mat = _f64(mat)
        if mat.ndim != 2 or mat.shape[0] != upper - lower or mat.shape[1] % 2 != 1:
            raise ValueError("mat shape is not consistent with insert limits")
        L.check(self._lib.natac_set_vmat(self._h, _ptr(mat), int(lower), int(upper), mat.shape[1] // 2))
        self.vmat_shape = mat.shape

    def bg_tiling(self, chunk_len):
        """(tiles, extended tiles among them) of the background stage for a chunk of this length with the V-plot that is set
        (natac_bg_tiling)."""
        nt, ex = C.c_int32(0), C.c_int32(0)
        L.check(self._lib.natac_bg_tiling(self._h, int(chunk_len), C.byref(nt), C.byref(ex)))
        return nt.value, ex.value

    def set_sizes(self, sizes):
        """global insert-size distribution over [0, len(sizes)) (pyatac/chunkmat2d.py:154-156)."""
        sizes = _f64(sizes)
        L.check(self._lib.natac_set_sizes(self._h, _ptr(sizes), sizes.shape[0]))

    def set_occ_model(self, nuc_probs, nfr_probs, alphas=None, cutoff=None, step=5, flank=60):
        """OccupancyCalcParams / OccupancyParameters (nucleoatac/Occupancy.py:89-102, 175-193)."""
        nuc_probs, nfr_probs = _f64(nuc_probs), _f64(nfr_probs)
        if nuc_probs.shape != nfr_probs.shape:
            raise ValueError("nuc_probs / nfr_probs shape mismatch")
        if alphas is None:
            alphas = np.linspace(0, 1, 101)
        alphas = _f64(alphas)
        if cutoff is None:
            from scipy import stats
            cutoff = float(stats.chi2.ppf(0.9, 1))
        L.check(self._lib.natac_set_occ_model(self._h, _ptr(nuc_probs), _ptr(nfr_probs), nuc_probs.shape[0],
                                              _ptr(alphas), alphas.shape[0], float(cutoff), int(step), int(flank)))
        step = int(step)
        self.occ_step = step - 1 if step % 2 == 0 else step
        self.occ_upper = nuc_probs.shape[0]

    def occ_route(self):
        """(fast, rn, zero_flags) of the last set_occ_model (natac_ctx_occ_route): whether natac_occ_decide runs, its renormalisation
        period (16 or 4; 0 when the general kernel takes everything) and its zero-probability flags."""
        fast, rn, zf = C.c_int32(), C.c_int32(), C.c_int32()
        L.check(self._lib.natac_ctx_occ_route(self._h, C.byref(fast), C.byref(rn), C.byref(zf)))
        return bool(fast.value), rn.value, zf.value

    # ---- Cython-function drop-ins ------------------------------------------------------------
    def make_fragment_mat(self, l, n, start, end, lower, upper):
        """makeFragmentMat (pyatac/fragments.pyx:17-40) on packed fragments (l = pos+4, n = |tlen|-8)."""
        l = np.ascontiguousarray(l, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        mat = np.empty((upper - lower, end - start), dtype=np.float64)
        L.check(self._lib.natac_make_fragment_mat(self._h, l.shape[0], _ptr(l), _ptr(n), int(start), int(end),
                                                  int(lower), int(upper), _ptr(mat)))
        return mat

    def get_insertions(self, l, n, start, end, lower=0, upper=2000):
        """getInsertions (pyatac/fragments.pyx:43-67)."""
        l = np.ascontiguousarray(l, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        out = np.empty(end - start, dtype=np.float64)
        L.check(self._lib.natac_get_insertions(self._h, l.shape[0], _ptr(l), _ptr(n), int(start), int(end),
                                               int(lower), int(upper), _ptr(out)))
        return out

    def get_stranded_insertions(self, l, n, start, end, lower=0, upper=2000):
        """getStrandedInsertions (pyatac/fragments.pyx:71-97): (plus, minus)."""
        l = np.ascontiguousarray(l, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        plus, minus = np.empty(end - start, dtype=np.float64), np.empty(end - start, dtype=np.float64)
        L.check(self._lib.natac_get_stranded_insertions(self._h, l.shape[0], _ptr(l), _ptr(n), int(start), int(end),
                                                        int(lower), int(upper), _ptr(plus), _ptr(minus)))
        return plus, minus

    def fragment_sizes(self, l, n, chunk_starts, chunk_ends, lower, upper):
        """getFragmentSizesFromChunkList (pyatac/fragments.pyx:123-145), one chromosome."""
        l = np.ascontiguousarray(l, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int32)
        cs = np.ascontiguousarray(chunk_starts, dtype=np.int64)
        ce = np.ascontiguousarray(chunk_ends, dtype=np.int64)
        out = np.empty(upper - lower, dtype=np.float64)
        L.check(self._lib.natac_fragment_sizes(self._h, l.shape[0], _ptr(l), _ptr(n), cs.shape[0], _ptr(cs), _ptr(ce),
                                               int(lower), int(upper), _ptr(out)))
        return out

    def calculate_cov(self, p, v, r, literal=False):
        """calculateCov (nucleoatac/multinomial_cov.pyx:20-31); raises ValueError on a shape mismatch (:21-22)."""
        p, v = _f64(p), _f64(v)
        if p.ndim != 1 or v.ndim != 1 or p.shape[0] != v.shape[0]:
            raise ValueError("p and v must be same shape")
        out = C.c_double(0)
        L.check(self._lib.natac_calculate_cov(self._h, _ptr(p), _ptr(v), p.shape[0], int(r), 1 if literal else 0,
                                              C.byref(out)))
        return out.value

    # ---- operator-level entry points ------------------------------------------------------------
    def smooth(self, sig, window_len, window="flat", sd=None, mode="valid", norm=True):
        """utils.smooth (pyatac/utils.py:23-52) on the GPU."""
        import warnings
        if window not in ("flat", "gaussian"):
            raise Exception("Incorrect window input for smooth. Options are flat, gaussian")
        if mode not in ("valid", "same"):
            raise Exception("mode must be 'valid' or 'same'")
        if window_len % 2 != 1:
            warnings.warn("Window length is even number.  Needs to be odd so adding 1.")
            window_len += 1
        if window == "gaussian":
            if sd is None:
                sd = (window_len - 1) / 6.0
            nn = np.arange(window_len) - (window_len - 1) / 2.0
            w = np.exp(-0.5 * (nn / sd) ** 2)     # scipy.signal.gaussian
        else:
            w = np.ones(window_len)
        sig = _f64(sig)
        w = _f64(w)
        out = np.empty(sig.shape[0] - window_len + 1 if mode == "valid" else sig.shape[0], dtype=np.float64)
        L.check(self._lib.natac_smooth(self._h, _ptr(sig), sig.shape[0], _ptr(w), int(window_len),
                                       0 if mode == "valid" else 1, 1 if norm else 0, _ptr(out)))
        return out

    def make_bias_mat(self, bias_log, track_start, start, end, lower, upper):
        """BiasMat2D.makeBiasMat (pyatac/chunkmat2d.py:140-153) for a log-scale bias track."""
        b = _f64(bias_log)
        mat = np.empty((upper - lower, end - start), dtype=np.float64)
        L.check(self._lib.natac_make_bias_mat(self._h, _ptr(b), b.shape[0], int(track_start), int(start), int(end),
                                              int(lower), int(upper), _ptr(mat)))
        return mat

    def pwm_bias(self, sequence, pwm_mat, nucleotides):
        """InsertionBiasTrack.computeBias (pyatac/bias.py:85-92): log-bias of every position of `sequence`."""
        if isinstance(sequence, np.ndarray) and sequence.dtype == np.uint8:
            seq = np.ascontiguousarray(sequence)              # already upper-case ASCII codes (FastaStore)
        else:
            seq = np.frombuffer(sequence.encode("ascii") if isinstance(sequence, str) else bytes(sequence), dtype=np.uint8)
        logp = _f64(np.log(np.asarray(pwm_mat, dtype=np.float64)))
        lens = set(len(x) for x in nucleotides)
        if len(lens) != 1:     # the reference's seq_to_mat check (pyatac/seq.py:39-41)
            raise Exception("Usage Error! Nucleotides must all be of same length! No mixing single nucleotides with dinucleotides, etc")
        if lens != {1}:
            raise NotImplementedError("k-mer PWMs (words of %d letters) are not supported by natac_pwm_bias: single-"
                                      "nucleotide PWMs only (every PWM shipped with the reference is one)" % lens.pop())
        nucs = np.frombuffer("".join(nucleotides).encode("ascii"), dtype=np.uint8)
        out = np.empty(len(seq) - logp.shape[1] + 1, dtype=np.float64)
        L.check(self._lib.natac_pwm_bias(self._h, _ptr(seq), len(seq), _ptr(logp), _ptr(nucs), logp.shape[0],
                                         logp.shape[1], _ptr(out)))
        return out

    def insertion_seq_counts(self, chunk_len, frag_off, frag_lpos, frag_ilen, seq_off, seq, flank, lower=0, upper=2000, sym=True,
                             with_kernel_ms=False):
        """window counts of `pyatac pwm` over a packed chunk list (_pwmHelper, pyatac/get_pwm.py:21-40): (M int64[4, 2*flank+1] with
        rows A C G T, n = counted insertions), exact.  seq[seq_off[k]:seq_off[k+1]] = the bases of [start_k - flank, end_k + flank).
        with_kernel_ms: also return the counting kernel's device time in ms."""
        cl = np.ascontiguousarray(chunk_len, dtype=np.int32)
        fo = np.ascontiguousarray(frag_off, dtype=np.int64)
        fl = np.ascontiguousarray(frag_lpos, dtype=np.int32)
        fi = np.ascontiguousarray(frag_ilen, dtype=np.int32)
        so = np.ascontiguousarray(seq_off, dtype=np.int64)
        sq = np.ascontiguousarray(seq, dtype=np.uint8)
        if fo.shape[0] != cl.shape[0] + 1 or so.shape[0] != cl.shape[0] + 1:
            raise ValueError("frag_off and seq_off need n_chunks + 1 entries")
        if fl.shape != fi.shape or (cl.shape[0] and (fo[-1] != fl.shape[0] or so[-1] != sq.shape[0])):
            raise ValueError("frag_off / seq_off do not match the fragment and sequence arrays")
        K = 2 * int(flank) + 1
        counts = np.zeros((4, max(K, 1)), dtype=np.int64)
        n = C.c_int64(0)
        ms = C.c_double(0)
        L.check(self._lib.natac_insertion_seq_counts(self._h, cl.shape[0], _ptr(cl), _ptr(fo), _ptr(fl), _ptr(fi), _ptr(so), _ptr(sq),
                                                     int(flank), int(lower), int(upper), 1 if sym else 0, _ptr(counts), C.byref(n),
                                                     C.byref(ms)))
        return (counts, n.value, ms.value) if with_kernel_ms else (counts, n.value)

    def base_counts(self, seq, starts=None, ends=None, per_range=False):
        """int64[4]: the A, C, G, T bases of seq[starts[i]:ends[i]] summed over the ranges (default: the whole array); the numerators of
        seq.getNucFreqs / getNucFreqsFromChunkList (pyatac/seq.py:47-72).  per_range: int64[n_ranges, 4], every range on its own
        (natac_window_base_counts), by the same rule."""
        sq = np.ascontiguousarray(seq, dtype=np.uint8)
        st = np.ascontiguousarray([0] if starts is None else starts, dtype=np.int64)
        en = np.ascontiguousarray([sq.shape[0]] if ends is None else ends, dtype=np.int64)
        if st.shape != en.shape:
            raise ValueError("starts and ends differ in length")
        if per_range:
            if st.ndim != 1:
                raise ValueError("starts and ends must be 1-d")
            out = np.zeros((st.shape[0], 4), dtype=np.int64)
            L.check(self._lib.natac_window_base_counts(self._h, _ptr(sq), sq.shape[0], st.shape[0], _ptr(st), _ptr(en), _ptr(out)))
            return out
        out = np.zeros(4, dtype=np.int64)
        L.check(self._lib.natac_base_counts(self._h, _ptr(sq), sq.shape[0], st.shape[0], _ptr(st), _ptr(en), _ptr(out)))
        return out

    def region_counts(self, pos, tlen, starts, ends, lower=0, upper=500, atac=True, with_kernel_ms=False):
        """fragment counts of `pyatac counts` (pyatac/get_counts.py:30-45) for regions of one chromosome: int64[n_regions], exact.
        pos (sorted) / tlen are the chromosome's records as the FragmentStore holds them; a record counts for [start, end) if
        lower <= ilen < upper and its left or its right end lies in it.  with_kernel_ms: also return the kernels' device time."""
        p = np.ascontiguousarray(pos, dtype=np.int64)
        t = np.ascontiguousarray(tlen, dtype=np.int64)
        st = np.ascontiguousarray(starts, dtype=np.int64)
        en = np.ascontiguousarray(ends, dtype=np.int64)
        if p.ndim != 1 or p.shape != t.shape or st.ndim != 1 or st.shape != en.shape:
            raise ValueError("pos / tlen and starts / ends must be pairs of 1-d arrays of one length")
        out = np.zeros(st.shape[0], dtype=np.int64)
        ms = C.c_double(0)
        L.check(self._lib.natac_region_counts(self._h, p.shape[0], _ptr(p), _ptr(t), st.shape[0], _ptr(st), _ptr(en), int(lower),
                                              int(upper), 1 if atac else 0, _ptr(out), C.byref(ms)))
        return (out, ms.value) if with_kernel_ms else out

    def region_cell_counts(self, pos, tlen, cell, n_cells, starts, ends, lower=0, upper=500, atac=True, with_kernel_ms=False):
        """the cell-by-region count matrix of one chromosome (natac_region_cell_counts) as CSR with one row per region, in the given
        order: (indptr int64[n_regions + 1], indices int32[nnz], data int32[nnz]); within a row the cell indices ascend, data is the
        number of records of that cell that count for the region by region_counts' rule, exact.  pos (sorted) / tlen / cell are the
        chromosome's records as a cell-tagged FragmentStore holds them (FragmentStore.from_fragments_cells), cell in [0, n_cells).
        with_kernel_ms: also return the device time of the call's kernels."""
        p = np.ascontiguousarray(pos, dtype=np.int64)
        t = np.ascontiguousarray(tlen, dtype=np.int64)
        ce = np.ascontiguousarray(cell, dtype=np.int32)
        st = np.ascontiguousarray(starts, dtype=np.int64)
        en = np.ascontiguousarray(ends, dtype=np.int64)
        if p.ndim != 1 or p.shape != t.shape or p.shape != ce.shape or st.ndim != 1 or st.shape != en.shape:
            raise ValueError("pos / tlen / cell and starts / ends must be 1-d arrays of one length each")
        # room for the entries: a row has at most as many as it has candidate records (the kernels' own search, natac_region_ranges:
        # every record that can count lies in that range of the sorted pos) and at most n_cells
        shift = 4 if atac else 0
        a = np.searchsorted(p, st - max(int(upper), 1) - shift, "right")
        b = np.searchsorted(p, en + max(0, 1 - int(lower)) - shift, "left")
        cap = int(np.minimum(np.maximum(b - a, 0), max(int(n_cells), 1)).sum())
        indptr = np.zeros(st.shape[0] + 1, dtype=np.int64)
        col = np.empty(max(cap, 1), dtype=np.int32)
        val = np.empty(max(cap, 1), dtype=np.int32)
        ms = C.c_double(0)
        L.check(self._lib.natac_region_cell_counts(self._h, p.shape[0], _ptr(p), _ptr(t), _ptr(ce), int(n_cells), st.shape[0], _ptr(st),
                                                   _ptr(en), int(lower), int(upper), 1 if atac else 0, _ptr(indptr), col.shape[0],
                                                   _ptr(col), _ptr(val), C.byref(ms)))
        nnz = int(indptr[-1])
        out = (indptr, col[:nnz].copy(), val[:nnz].copy())
        return out + (ms.value,) if with_kernel_ms else out

    def gene_cell_scores(self, pos, tlen, cell, n_cells, win_lo, win_hi, body_lo, body_hi, weight, lower, upper, with_hits=False,
                         with_arm_rows=False, with_kernel_ms=False):
        """the device part of `pyatac genescores` for one chromosome (natac_gene_cell_scores; include/natac.h states the rule): CSR with
        one row per gene in the given order, (indptr int64[n_genes + 1], indices int32[nnz], data int32[nnz]); within a row the cell
        indices ascend, data is the exact sum of weight[d] over the cell's insertions in [win_lo, win_hi), d the distance to
        [body_lo, body_hi).  pos (sorted) / tlen / cell as region_cell_counts takes them; weight int32[n_w], every element in
        [1, NATAC_GENESCORES_MAX_WEIGHT].  A sizing call, then the filling call.  with_hits: also int64[n_genes], the insertions that
        counted per gene; with_arm_rows: also int64[2], the non-empty rows the short and the table arm took; with_kernel_ms: also the
        kernels' device time of both calls.  A refused operand raises before anything is returned."""
        p = np.ascontiguousarray(pos, dtype=np.int64)
        t = np.ascontiguousarray(tlen, dtype=np.int64)
        ce = np.ascontiguousarray(cell, dtype=np.int32)
        g = [np.ascontiguousarray(a, dtype=np.int64) for a in (win_lo, win_hi, body_lo, body_hi)]
        w = np.ascontiguousarray(weight, dtype=np.int32)
        if p.ndim != 1 or p.shape != t.shape or p.shape != ce.shape or g[0].ndim != 1 or any(a.shape != g[0].shape for a in g) or w.ndim != 1:
            raise ValueError("pos / tlen / cell, the four gene arrays and weight must be 1-d arrays of one length each")
        ng = g[0].shape[0]
        indptr = np.zeros(ng + 1, dtype=np.int64)
        hits, arms = np.zeros(ng, dtype=np.int64), np.zeros(2, dtype=np.int64)
        ms, ms_all = C.c_double(0), 0.0

        def call(cap, col, val):
            L.check(self._lib.natac_gene_cell_scores(self._h, p.shape[0], _ptr(p), _ptr(t), _ptr(ce), int(n_cells), ng, _ptr(g[0]), _ptr(g[1]),
                                                     _ptr(g[2]), _ptr(g[3]), w.shape[0], _ptr(w), int(lower), int(upper), _ptr(indptr), cap,
                                                     _ptr(col), _ptr(val), _ptr(hits), _ptr(arms), C.byref(ms)))
            return ms.value

        ms_all += call(0, None, None)
        nnz = int(indptr[-1])
        col, val = np.empty(nnz, dtype=np.int32), np.empty(nnz, dtype=np.int32)
        if nnz:
            ms_all += call(nnz, col, val)
        res = (indptr, col, val)
        if with_hits:
            res += (hits,)
        if with_arm_rows:
            res += (arms,)
        return res + (ms_all,) if with_kernel_ms else res

    def knn(self, points, k, queries=None, self_offset=None, max_out=None, with_arm_queries=False, with_kernel_ms=False):
        """exact k nearest neighbours (natac_knn; include/natac.h states the rule): (idx int32[nq, k], dist2 float64[nq, k]), row i the k
        smallest references by (d2, index) ascending, d2 the plain column-ordered sum of squared differences in fp64; where fewer than k
        references are available the tail is -1 / +inf.  points float64[nr, dim] are the references.  queries=None: every point queries
        all points with itself excluded.  Otherwise queries float64[nq, dim], and self_offset (None or -1: nothing excluded) says that
        query i is reference i + self_offset and is left out of its own row.  The queries are cut into blocks of at most max_out // k
        rows (default and most NATAC_KNN_MAX_OUT); the result does not depend on the cut.  with_arm_queries: also int64[2], the queries
        the wave and the lds arm took; with_kernel_ms: also the kernels' device time.  A refused operand raises before anything is
        returned."""
        x = _f64(points)
        if x.ndim != 2:
            raise ValueError("points must be a 2-d array [nr, dim]")
        if queries is None:
            q, so = x, 0
        else:
            q, so = _f64(queries), -1 if self_offset is None else int(self_offset)
            if q.ndim != 2 or q.shape[1] != x.shape[1]:
                raise ValueError("queries must be a 2-d array with the columns of points")
        k = int(k)
        if not 1 <= k <= L.KNN_MAX_K:       # before it sizes the outputs
            raise ValueError("k must be in [1, %d] (got %d)" % (L.KNN_MAX_K, k))
        max_out = L.KNN_MAX_OUT if max_out is None else min(int(max_out), L.KNN_MAX_OUT)
        block = max(max_out // k, 1)
        nq, nr, dim = q.shape[0], x.shape[0], x.shape[1]
        idx, d2 = np.empty((nq, k), dtype=np.int32), np.empty((nq, k), dtype=np.float64)
        arms, arms_all = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64)
        ms, ms_all = C.c_double(0), 0.0
        for lo in range(0, max(nq, 1), block):
            n = min(block, nq - lo)
            qb, ib, db = q[lo:lo + n], idx[lo:lo + n], d2[lo:lo + n]
            L.check(self._lib.natac_knn(self._h, n, nr, dim, _ptr(qb), _ptr(x), so + lo if so >= 0 else -1, k, _ptr(ib), _ptr(db), _ptr(arms),
                                        C.byref(ms)))
            arms_all += arms
            ms_all += ms.value
        res = (idx, d2)
        if with_arm_queries:
            res += (arms_all,)
        return res + (ms_all,) if with_kernel_ms else res

    def sparse_lsi(self, indptr, indices, data, n_cells, row_weight, col_scale, r, n_iter, q0, scale=1e4, transform="log", binarize=False,
                   with_kernel_ms=False):
        """the r leading singular triplets of the weighted cell-by-window matrix (natac_sparse_lsi; include/natac.h states the
        algorithm): (sigma float64[r] descending, U float64[n_cells, r], V float64[n_windows, r]).  indptr / indices / data are the CSR
        arrays of region_cell_counts (rows the windows, indices the cells, ascending within a row, data >= 1).  The entry of count a in
        window w and cell c is t = a' * col_scale[c] * row_weight[w] (a' = 1 with binarize) or, with transform "log", log1p(t * scale); a
        zero weight or scale drops the window or the cell, whose vector is then zero.  q0 float64[n_windows, r] starts the n_iter rounds of
        subspace iteration.  Every component's sign is fixed here: the entry of largest magnitude in its column of U (the lowest index
        among equals) is positive, the column of V is flipped with it.  ValueError("rank") when the matrix has fewer than r independent
        directions.  ValueError("range") when the size of the weights or of q0 takes a Gram matrix of the iteration out of fp64's range
        (singular values above about 1e154 or below about 1e-146 / sqrt(r); natac.h has the rule) -- inside it a power of two in the
        weights or in q0 changes no bit of U and V.  with_kernel_ms: also return the device time of the call's kernels."""
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        da = np.ascontiguousarray(data, dtype=np.int32)
        rw = _f64(row_weight)
        cs = _f64(col_scale)
        q = _f64(q0)
        r, n, m = int(r), int(n_cells), ip.shape[0] - 1
        if ip.ndim != 1 or m < 0 or ix.ndim != 1 or ix.shape != da.shape or rw.shape != (m,) or cs.shape != (max(n, 0),):
            raise ValueError("indptr / indices / data must be CSR arrays, row_weight one per row and col_scale one per cell")
        if transform not in ("log", "linear"):
            raise ValueError("transform must be 'log' or 'linear' (got %r)" % (transform,))
        if not 1 <= r <= L.LSI_MAX_R:       # before it sizes the outputs
            raise ValueError("r must be in [1, %d] (got %d)" % (L.LSI_MAX_R, r))
        if q.shape != (m, r):
            raise ValueError("q0 must have one row per window and r columns")
        if m and int(ip[-1]) > ix.shape[0]:
            raise ValueError("indptr points past the %d entries given" % ix.shape[0])
        sigma = np.zeros(r, dtype=np.float64)
        U = np.zeros((n, r), dtype=np.float64)
        V = np.zeros((m, r), dtype=np.float64)
        status, ms = C.c_int32(0), C.c_double(0)
        L.check(self._lib.natac_sparse_lsi(self._h, m, n, _ptr(ip), _ptr(ix), _ptr(da), _ptr(rw), _ptr(cs), float(scale),
                                           1 if transform == "log" else 0, 1 if binarize else 0, r, int(n_iter), _ptr(q), _ptr(sigma),
                                           _ptr(U), _ptr(V), C.byref(status), C.byref(ms)))
        if status.value:
            raise ValueError("range" if status.value == 2 else "rank")
        top = np.argmax(np.abs(U), axis=0)
        flip = np.where(U[top, np.arange(r)] < 0, -1.0, 1.0)
        U *= flip
        V *= flip
        return (sigma, U, V, ms.value) if with_kernel_ms else (sigma, U, V)

    def motif_deviations(self, indptr, indices, data, n_cells, hit_indptr, hit_indices, n_motifs, bg, with_kernel_ms=False, with_sums=False):
        """the device part of `pyatac deviations` (natac_motif_deviations; include/natac.h states the rule): (raw, bg_mean, bg_m2), each
        float64[n_motifs, n_cells].  indptr / indices / data are the CSR arrays of region_cell_counts after the dropping (rows the windows,
        every window and every cell with an entry, data >= 1, the total below 2^31); hit_indptr / hit_indices the CSR pattern of the
        window-by-motif hit matrix over the same windows (motifs ascending within a row; the values are not needed) -- it is turned
        motif-major here with a stable sort by motif, so every motif's windows ascend; bg int32[B, n_windows] the background sets 1 .. B.
        with_sums: also (O int64[B + 1, n_motifs, n_cells], E int64[B + 1, n_motifs]), the testing output.  with_kernel_ms: also the
        kernel's device time.  The returned arrays are filled only by a call that succeeds."""
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        da = np.ascontiguousarray(data, dtype=np.int32)
        hp = np.ascontiguousarray(hit_indptr, dtype=np.int64)
        hx = np.ascontiguousarray(hit_indices, dtype=np.int64)
        bgm = np.ascontiguousarray(bg, dtype=np.int32)
        n, M, m = int(n_cells), int(n_motifs), ip.shape[0] - 1
        if ip.ndim != 1 or m < 0 or ix.ndim != 1 or ix.shape != da.shape or hp.shape != (m + 1,) or hx.ndim != 1:
            raise ValueError("indptr / indices / data and hit_indptr / hit_indices must be CSR arrays over the same windows")
        if m and int(ip[-1]) > ix.shape[0]:
            raise ValueError("indptr points past the %d entries given" % ix.shape[0])
        if m and (int(hp[0]) != 0 or int(hp[-1]) != hx.shape[0] or np.any(np.diff(hp) < 0)):
            raise ValueError("hit_indptr does not describe the %d hit entries given" % hx.shape[0])
        if not 0 <= M <= 2147483647 or not 0 <= n <= 2147483647:
            raise ValueError("n_motifs and n_cells must be in [0, 2^31)")
        if len(hx) and (hx.min() < 0 or hx.max() >= M):
            raise ValueError("hit_indices holds a motif outside [0, %d)" % M)
        if bgm.ndim != 2 or bgm.shape[1] != m:
            raise ValueError("bg must have one column per window")
        B = bgm.shape[0]
        # motif-major: a stable sort of the (window, motif) pairs by motif keeps the windows ascending
        mot_ptr = np.zeros(M + 1, dtype=np.int64)
        np.cumsum(np.bincount(hx, minlength=M), out=mot_ptr[1:])
        win = np.repeat(np.arange(m, dtype=np.int32), np.diff(hp)) if m else np.zeros(0, np.int32)
        mot_win = np.ascontiguousarray(win[np.argsort(hx, kind="stable")], dtype=np.int32)
        out = [np.zeros((M, n), dtype=np.float64) for _ in range(3)]
        sums = [np.zeros((B + 1, M, n), dtype=np.int64), np.zeros((B + 1, M), dtype=np.int64)] if with_sums else None
        ms = C.c_double(0)
        L.check(self._lib.natac_motif_deviations(self._h, m, n, _ptr(ip), _ptr(ix), _ptr(da), M, _ptr(mot_ptr), _ptr(mot_win), B, _ptr(bgm),
                                                 _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(sums[0]) if sums else None,
                                                 _ptr(sums[1]) if sums else None, C.byref(ms)))
        res = tuple(out)
        if with_sums:
            res += tuple(sums)
        return res + (ms.value,) if with_kernel_ms else res

    def group_rank_sums(self, indptr, indices, data, n_cells, depth, group, n_groups, with_kernel_ms=False, with_arm_rows=False, max_out=None):
        """the device part of `pyatac markers` (natac_group_rank_sums; include/natac.h states the rule): (detected int32, total int64,
        rank2 int64, each [n_windows, n_groups], ties int64[n_windows]).  indptr / indices / data are the CSR arrays of
        region_cell_counts restricted to the kept cells (rows the windows, empty rows allowed, indices ascending within a row, data >= 1);
        depth[n_cells] in [1, 2^31) and group[n_cells] in [0, n_groups) belong to the cells.  The rows go to the device in blocks of at
        most max_out // n_groups (max_out defaults to NATAC_MARKERS_MAX_OUT and may only be lowered); the result does not depend on the
        cut.  with_arm_rows: also int64[3], the rows the short, block and long arm took; with_kernel_ms: also the kernels' device time.
        The returned arrays are filled only by blocks that succeed; a refused operand raises before anything is returned."""
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        da = np.ascontiguousarray(data, dtype=np.int32)
        dp = np.ascontiguousarray(depth, dtype=np.int64)
        gr = np.ascontiguousarray(group, dtype=np.int32)
        n, G, m = int(n_cells), int(n_groups), ip.shape[0] - 1
        if ip.ndim != 1 or m < 0 or ix.ndim != 1 or ix.shape != da.shape or dp.shape != (max(n, 0),) or gr.shape != dp.shape:
            raise ValueError("indptr / indices / data must be CSR arrays, depth and group one per cell")
        if m and int(ip[-1]) > ix.shape[0]:
            raise ValueError("indptr points past the %d entries given" % ix.shape[0])
        cap = L.MARKERS_MAX_OUT if max_out is None else int(max_out)
        if not 1 <= cap <= L.MARKERS_MAX_OUT:
            raise ValueError("max_out must be in [1, %d] (got %d)" % (L.MARKERS_MAX_OUT, cap))
        step = max(1, cap // max(G, 1))
        detected = np.zeros((m, max(G, 0)), dtype=np.int32)
        total = np.zeros((m, max(G, 0)), dtype=np.int64)
        rank2 = np.zeros((m, max(G, 0)), dtype=np.int64)
        ties = np.zeros(m, dtype=np.int64)
        arms, ms_all = np.zeros(3, dtype=np.int64), 0.0
        for r0 in range(0, max(m, 1), step):          # m == 0 still makes the one call that checks the operands
            r1 = min(m, r0 + step)
            part, ms = np.zeros(3, dtype=np.int64), C.c_double(0)
            L.check(self._lib.natac_group_rank_sums(self._h, r1 - r0, n, _ptr(ip[r0:r1 + 1]), _ptr(ix), _ptr(da), _ptr(dp), _ptr(gr), G,
                                                    _ptr(detected[r0:r1]), _ptr(total[r0:r1]), _ptr(rank2[r0:r1]), _ptr(ties[r0:r1]),
                                                    _ptr(part), C.byref(ms)))
            arms += part
            ms_all += ms.value
        res = (detected, total, rank2, ties)
        if with_arm_rows:
            res += (arms,)
        return res + (ms_all,) if with_kernel_ms else res

    def window_pair_sums(self, indptr, indices, data, n_cells, order, hi, with_arm_owners=False, with_kernel_ms=False, max_pairs=None):
        """the device part of `pyatac coaccess` (natac_window_pair_sums; include/natac.h states the rule): (sxy int64, both int32), one
        element per pair.  indptr / indices / data are the CSR arrays of region_cell_counts (rows the windows, empty rows allowed, indices
        ascending within a row, data >= 1).  order[k] lists rows in rank sequence; owner i is paired with order[i + 1 .. hi[i]),
        i < hi[i] <= k, and its pairs follow those of owner i - 1.  The owners go to the device in consecutive blocks of at most
        max_pairs pairs (max_pairs defaults to NATAC_COACCESS_MAX_PAIRS and may only be lowered; ValueError if one owner alone has more),
        one call per block with the slice of `order` its partners need; the result does not depend on the cut.  ValueError as well for
        an hi outside its range and where N * a_max^2 * L_max reaches 2^62 (n_cells, the largest count, the longest listed row).
        with_arm_owners: also int64[2], the owners with a partner that the table and the search arm took; with_kernel_ms: also the
        kernels' device time.  A refused operand raises before anything is returned."""
        ip = np.ascontiguousarray(indptr, dtype=np.int64)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        da = np.ascontiguousarray(data, dtype=np.int32)
        od = np.ascontiguousarray(order, dtype=np.int32)
        h = np.ascontiguousarray(hi, dtype=np.int64)
        n, m, k = int(n_cells), ip.shape[0] - 1, od.shape[0]
        if ip.ndim != 1 or m < 0 or ix.ndim != 1 or ix.shape != da.shape or od.ndim != 1 or h.shape != od.shape:
            raise ValueError("indptr / indices / data must be CSR arrays, order and hi one per listed window")
        if m and int(ip[-1]) > ix.shape[0]:
            raise ValueError("indptr points past the %d entries given" % ix.shape[0])
        cap = L.COACCESS_MAX_PAIRS if max_pairs is None else int(max_pairs)
        if not 1 <= cap <= L.COACCESS_MAX_PAIRS:
            raise ValueError("max_pairs must be in [1, %d] (got %d)" % (L.COACCESS_MAX_PAIRS, cap))
        own = np.arange(k, dtype=np.int64)
        bad = np.flatnonzero((h <= own) | (h > k))
        if len(bad):
            raise ValueError("hi[%d] = %d outside (%d, %d]" % (bad[0], h[bad[0]], bad[0], k))
        if k and m and ((od < 0) | (od >= m)).any():
            w = int(np.flatnonzero((od < 0) | (od >= m))[0])
            raise ValueError("order[%d] = %d outside [0, %d)" % (w, od[w], m))
        if k and m and len(da):
            a_max, l_max = int(da.max()), int(np.diff(ip)[od].max())
            if n * a_max * a_max * l_max >= 1 << 62:
                raise ValueError("N * a_max^2 * L_max must be below 2^62: N = %d cells, a_max = %d the largest count, L_max = %d the longest "
                                 "listed row" % (n, a_max, l_max))
        n_part = h - own - 1
        if k and int(n_part.max()) > cap:
            w = int(np.argmax(n_part > cap))
            raise ValueError("owner %d alone has %d partners, more than max_pairs = %d" % (w, n_part[w], cap))
        ptr = np.zeros(k + 1, dtype=np.int64)
        np.cumsum(n_part, out=ptr[1:])
        sxy, both = np.zeros(int(ptr[-1]), dtype=np.int64), np.zeros(int(ptr[-1]), dtype=np.int32)
        arms, ms_all = np.zeros(2, dtype=np.int64), 0.0
        i0 = 0
        while True:                                   # k == 0 still makes the one call that checks the operands
            i1 = min(k, max(i0 + 1, int(np.searchsorted(ptr, ptr[i0] + cap, side="right")) - 1))
            end = int(h[i0:i1].max()) if i1 > i0 else i0                   # the block's partners reach order[end - 1]
            # the partners past the block's owners are listed without partners of their own
            h_blk = np.concatenate([h[i0:i1] - i0, np.arange(i1 - i0 + 1, end - i0 + 1, dtype=np.int64)])
            p_blk = np.concatenate([ptr[i0:i1 + 1] - ptr[i0], np.full(end - i1, ptr[i1] - ptr[i0], dtype=np.int64)])
            o_blk = np.ascontiguousarray(od[i0:end])
            part, ms = np.zeros(2, dtype=np.int64), C.c_double(0)
            L.check(self._lib.natac_window_pair_sums(self._h, m, n, _ptr(ip), _ptr(ix), _ptr(da), end - i0, _ptr(o_blk), _ptr(h_blk), _ptr(p_blk),
                                                     _ptr(sxy[ptr[i0]:ptr[i1]]), _ptr(both[ptr[i0]:ptr[i1]]), _ptr(part), C.byref(ms)))
            arms += part
            ms_all += ms.value
            i0 = i1
            if i0 >= k:
                break
        res = (sxy, both)
        if with_arm_owners:
            res += (arms,)
        return res + (ms_all,) if with_kernel_ms else res

    def cell_site_qc(self, pos, tlen, cell, n_cells, site_center=None, site_minus=None, flank=1000, center=500, edge=100, peak_start=None,
                     peak_end=None, with_kernel_ms=False):
        """per-cell TSS counts, the aggregate TSS profile and per-cell fragments in peaks of one chromosome (natac_cell_site_qc):
        (tss_center int64[n_cells], tss_flank int64[n_cells], in_peaks int64[n_cells], profile int64[2 * flank + 1]), exact.  pos (sorted) /
        tlen / cell as region_cell_counts takes them; every record counts with its two insertions l = pos + 4 and r = pos + tlen - 5.
        site_center must be ascending (site_minus, or None for all plus, carried along); a pair of an insertion and a site with
        |d| <= flank adds to profile[d + flank], to tss_center of the cell if |d| <= center and to tss_flank if |d| > flank - edge.
        peak_start / peak_end are disjoint ascending intervals; a record with l or r in one adds 1 to in_peaks of its cell.  None for the
        sites or for the peaks skips that part.  with_kernel_ms: also return the device time of the call's kernels."""
        p = np.ascontiguousarray(pos, dtype=np.int64)
        t = np.ascontiguousarray(tlen, dtype=np.int64)
        ce = np.ascontiguousarray(cell, dtype=np.int32)
        sc = np.ascontiguousarray([] if site_center is None else site_center, dtype=np.int64)
        sm = None if site_minus is None else np.ascontiguousarray(site_minus, dtype=np.uint8)
        ps = np.ascontiguousarray([] if peak_start is None else peak_start, dtype=np.int64)
        pe = np.ascontiguousarray([] if peak_end is None else peak_end, dtype=np.int64)
        if p.ndim != 1 or p.shape != t.shape or p.shape != ce.shape or sc.ndim != 1 or ps.ndim != 1 or ps.shape != pe.shape or \
                (sm is not None and sm.shape != sc.shape):
            raise ValueError("pos / tlen / cell, site_center / site_minus and peak_start / peak_end must be 1-d arrays of one length each")
        n_cells, flank = int(n_cells), int(flank)
        if not 1 <= n_cells <= L.SPLIT_MAX_BARCODES:      # before it sizes the outputs and is narrowed to the int32 of the C call
            raise ValueError("n_cells must be in [1, %d] (got %d)" % (L.SPLIT_MAX_BARCODES, n_cells))
        out = [np.zeros(n_cells, dtype=np.int64) for _ in range(3)]
        profile = np.zeros(2 * min(max(flank, 0), L.CELLQC_MAX_FLANK) + 1, dtype=np.int64)
        ms = C.c_double(0)
        L.check(self._lib.natac_cell_site_qc(self._h, p.shape[0], _ptr(p), _ptr(t), _ptr(ce), n_cells, sc.shape[0], _ptr(sc),
                                             None if sm is None else _ptr(sm), flank, int(center), int(edge), ps.shape[0], _ptr(ps), _ptr(pe),
                                             _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(profile), C.byref(ms)))
        res = (out[0], out[1], out[2], profile)
        return res + (ms.value,) if with_kernel_ms else res

    def enriched_regions(self, pos, tlen, chrom_len, thr_small, thr_large, min_pileup, half_width=75, small=500, large=5000, max_gap=75,
                         min_length=150, capacity=None, with_kernel_ms=False, with_counts=False):
        """the enriched regions of one chromosome (natac_enriched_regions; include/natac.h states the rule): (start, end, summit int64,
        pileup, n_small, n_large int32) of the kept regions in ascending order, exact.  pos (sorted) / tlen as region_counts takes them;
        every record counts with its two insertions l = pos + 4 and r = pos + tlen - 5, each dropped on its own outside [0, chrom_len).
        A base is significant when its pileup p (insertions within half_width) is at least min_pileup and its counts within small and
        large are at most thr_small[k] and thr_large[k], k = min(p, len(thr_small) - 1); significant bases at most max_gap apart are one
        region, one shorter than min_length is dropped.  capacity: the room of the first call (default 4096); a call that finds more
        is made again with room for all.  with_counts: also (regions before the length rule, significant bases); with_kernel_ms: also
        the device time of the calls' kernels."""
        p = np.ascontiguousarray(pos, dtype=np.int64)
        t = np.ascontiguousarray(tlen, dtype=np.int64)
        ts = np.ascontiguousarray(thr_small, dtype=np.int32)
        tl = np.ascontiguousarray(thr_large, dtype=np.int32)
        if p.ndim != 1 or p.shape != t.shape or ts.ndim != 1 or ts.shape != tl.shape:
            raise ValueError("pos / tlen and thr_small / thr_large must be 1-d arrays of one length each")
        cap = 4096 if capacity is None else max(int(capacity), 0)
        n, found, nsig, ms, total_ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0), 0.0
        while True:
            out = [np.zeros(max(cap, 1), dtype=np.int64) for _ in range(3)] + [np.zeros(max(cap, 1), dtype=np.int32) for _ in range(3)]
            L.check(self._lib.natac_enriched_regions(self._h, p.shape[0], _ptr(p), _ptr(t), int(chrom_len), int(half_width), int(small),
                                                     int(large), int(max_gap), int(min_length), int(min_pileup), ts.shape[0], _ptr(ts),
                                                     _ptr(tl), C.byref(n), cap, *[_ptr(o) for o in out], C.byref(found), C.byref(nsig),
                                                     C.byref(ms)))
            total_ms += ms.value
            if n.value <= cap:
                break
            cap = int(n.value)
        res = tuple(o[:n.value].copy() for o in out)
        if with_counts:
            res += (int(found.value), int(nsig.value))
        return res + (total_ms,) if with_kernel_ms else res

    def motif_scan(self, seq, starts, ends, widths, scores, thresholds, with_kernel_ms=False, capacity=None):
        """the sites of integer position weight matrices in one chromosome (natac_motif_scan; include/natac.h states the rule):
        (motif int32, start int64, strand uint8, score int32, counts int32[n_windows, n_motifs]), the hits sorted by (motif, start,
        strand) on the device, exact.  seq: the chromosome's bytes, case as in the FASTA; starts / ends: the windows (None: the whole
        chromosome); widths[n_motifs]; scores: int32[sum of widths, 4], the motifs' columns one after the other, bases A C G T;
        thresholds[n_motifs].  A window start x is a `+` hit of a motif when its forward score reaches the threshold, a `-` hit when the
        reverse complement's does; counts[i, m] = the hits of motif m that lie inside window i.  capacity: the room of the first call
        (default NATAC_MOTIF_FIRST_CAPACITY, or the environment's value of that name); a call that finds more is made again with room
        for all.  with_kernel_ms: also the device time of the calls' kernels."""
        sq = np.ascontiguousarray(seq, dtype=np.uint8)
        st = np.ascontiguousarray([0] if starts is None else starts, dtype=np.int64)
        en = np.ascontiguousarray([sq.shape[0]] if ends is None else ends, dtype=np.int64)
        wd = np.ascontiguousarray(widths, dtype=np.int32)
        sc = np.ascontiguousarray(scores, dtype=np.int32)
        th = np.ascontiguousarray(thresholds, dtype=np.int32)
        if sq.ndim != 1 or st.ndim != 1 or st.shape != en.shape or wd.ndim != 1 or th.shape != wd.shape:
            raise ValueError("seq, starts / ends and widths / thresholds must be 1-d arrays, each pair of one length")
        if sc.size != 4 * int(np.maximum(wd, 0).sum(dtype=np.int64)):
            raise ValueError("scores must hold four numbers for every column of every motif")
        if capacity is None:
            capacity = int(os.environ.get("NATAC_MOTIF_FIRST_CAPACITY", L.MOTIF_FIRST_CAPACITY))
        cap = max(int(capacity), 0)
        counts = np.zeros((st.shape[0], wd.shape[0]), dtype=np.int32)
        n, ms, total_ms = C.c_int64(0), C.c_double(0), 0.0
        while True:
            out = [np.empty(max(cap, 1), dtype=dt) for dt in (np.int32, np.int64, np.uint8, np.int32)]
            L.check(self._lib.natac_motif_scan(self._h, _ptr(sq), sq.shape[0], st.shape[0], _ptr(st), _ptr(en), wd.shape[0], _ptr(wd),
                                               _ptr(sc), _ptr(th), C.byref(n), cap, *[_ptr(o) for o in out], _ptr(counts), C.byref(ms)))
            total_ms += ms.value
            if n.value <= cap:
                break
            cap = int(n.value)
        res = tuple(o[:n.value].copy() for o in out) + (counts,)
        return res + (total_ms,) if with_kernel_ms else res

    def site_seq_counts(self, seq, centers, minus, up, down, word=1, with_kernel_ms=False):
        """word counts of `pyatac nucleotide` (_nucleotideHelper, pyatac/get_nucleotide.py:19-38) around the sites of one chromosome:
        (M int64[4 or 16, up + down + 1], n = the sites whose window lies inside the chromosome), exact.  seq: the chromosome's bytes,
        case as in the FASTA; centers in [0, len(seq)); minus: per-site flags or None (all plus); word 1 (rows A C G T) or 2 (rows
        itertools.product("CGAT", repeat=2)).  with_kernel_ms: also return the kernel's device time."""
        sq = np.ascontiguousarray(seq, dtype=np.uint8)
        ce = np.ascontiguousarray(centers, dtype=np.int64)
        mi = None if minus is None else np.ascontiguousarray(minus, dtype=np.uint8)
        if sq.ndim != 1 or ce.ndim != 1 or (mi is not None and mi.shape != ce.shape):
            raise ValueError("seq and centers must be 1-d, minus as long as centers")
        rows = 16 if int(word) == 2 else 4
        counts = np.zeros((rows, max(int(up) + int(down) + 1, 1)), dtype=np.int64)
        n = C.c_int64(0)
        ms = C.c_double(0)
        L.check(self._lib.natac_site_seq_counts(self._h, _ptr(sq), sq.shape[0], ce.shape[0], _ptr(ce), None if mi is None else _ptr(mi),
                                                int(up), int(down), int(word), _ptr(counts), C.byref(n), C.byref(ms)))
        return (counts, n.value, ms.value) if with_kernel_ms else (counts, n.value)

    def site_signal(self, vals, src, length, lead, minus, K, exp=False, positive=False, scale=False, want_matrix=False, with_kernel_ms=False):
        """rows and aggregate of `pyatac signal` (_signalHelper, pyatac/signal_around_sites.py:24-74): (agg float64[K], mat float64[n, K]
        or None).  vals: the per-base track values the sites need, NaN where there is no record; site i is lead[i] zeros, the length[i]
        values from vals[src[i]], zeros up to K, reversed where minus[i] (None: all plus); then exp, positive (negatives to 0) and scale
        (NaN to 0, row / (sum |row| or 1)).  agg is the column sum with NaN as 0, added in the fixed order of natac.h (segments of
        _lib.SIGNAL_SEG sites): two calls give the same bits.  with_kernel_ms: also return the kernels' device time."""
        v = np.ascontiguousarray(vals, dtype=np.float64)
        sr = np.ascontiguousarray(src, dtype=np.int64)
        ln = np.ascontiguousarray(length, dtype=np.int32)
        ld = np.ascontiguousarray(lead, dtype=np.int32)
        mi = None if minus is None else np.ascontiguousarray(minus, dtype=np.uint8)
        if v.ndim != 1 or sr.ndim != 1 or ln.shape != sr.shape or ld.shape != sr.shape or (mi is not None and mi.shape != sr.shape):
            raise ValueError("vals and src must be 1-d; length, lead and minus as long as src")
        K = int(K)
        agg = np.zeros(max(K, 1), dtype=np.float64)
        mat = np.empty((sr.shape[0], max(K, 1)), dtype=np.float64) if want_matrix else None
        ms = C.c_double(0)
        flags = (1 if exp else 0) | (2 if positive else 0) | (4 if scale else 0)
        L.check(self._lib.natac_site_signal(self._h, _ptr(v), v.shape[0], sr.shape[0], _ptr(sr), _ptr(ln), _ptr(ld),
                                            None if mi is None else _ptr(mi), K, flags, None if mat is None else _ptr(mat), _ptr(agg),
                                            C.byref(ms)))
        return (agg, mat, ms.value) if with_kernel_ms else (agg, mat)

    def correlate_valid(self, sub, vmat):
        """signal.correlate(sub, vmat, mode='valid')[0] (nucleoatac/NucleosomeCalling.py:34-36)."""
        sub, vmat = _f64(sub), _f64(vmat)
        if sub.ndim != 2 or vmat.ndim != 2 or sub.shape[0] != vmat.shape[0]:
            raise ValueError("sub and vmat must have the same number of rows")
        out = np.empty(sub.shape[1] - vmat.shape[1] + 1, dtype=np.float64)
        L.check(self._lib.natac_correlate_valid(self._h, _ptr(sub), sub.shape[1], _ptr(vmat), vmat.shape[0],
                                                vmat.shape[1], _ptr(out)))
        return out

    def calculate_occupancy(self, inserts, bias):
        """calculateOccupancy (nucleoatac/Occupancy.py:104-120) with the model of set_occ_model."""
        ins, b = _f64(inserts), _f64(bias)
        upper = getattr(self, "occ_upper", None)
        if upper is not None and (ins.shape != (upper,) or b.shape != (upper,)):    # the C entry reads occ_upper values of each
            raise ValueError("inserts and bias must each hold the model's %d values (got %s and %s)" % (upper, ins.shape, b.shape))
        out = np.empty(3, dtype=np.float64)
        rc = self._lib.natac_calculate_occupancy(self._h, _ptr(ins), _ptr(b), _ptr(out))
        if rc == -1 and b"likelihood-ratio" in self._lib.natac_last_error():
            raise ValueError("min() arg is an empty sequence")   # what the reference raises (Occupancy.py:118)
        L.check(rc)
        return float(out[0]), float(out[1]), float(out[2])

    def format_doubles(self, vals):
        """python-2 str(float) of every value, formatted ON THE DEVICE (natac_format_doubles; validation of the track writer's
        '%.12g' arithmetic).  Returns (list of str, number of undecidable values)."""
        v = _f64(np.ravel(vals))
        n = v.shape[0]
        out = np.empty(24 * n, dtype=np.uint8)
        off = np.empty(n + 1, dtype=np.int64)
        hard = C.c_int32(0)
        L.check(self._lib.natac_format_doubles(self._h, _ptr(v), n, _ptr(out), out.nbytes, _ptr(off), C.byref(hard)))
        raw = out.tobytes()
        return [raw[off[i]:off[i + 1]].decode("ascii") for i in range(n)], hard.value

    # ---- profiling ---------------------------------------------------------------------------
    def profile_enable(self, on=True):
        L.check(self._lib.natac_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        L.check(self._lib.natac_profile_reset(self._h))

    def profile(self):
        """{kernel name: (total ms, launches)} from HIP events on the context's stream"""
        out = {}
        for k, name in enumerate(L.KERNEL_NAMES):
            ms, n = C.c_double(0), C.c_int64(0)
            L.check(self._lib.natac_profile_get(self._h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def clock_trace_start(self, max_samples=20000, interval_us=100):
        """start the one-wave shader-clock sampler (natac_clock_trace_start); profile_enable(True) makes the launches that follow
        appear as intervals on its time axis"""
        L.check(self._lib.natac_clock_trace_start(self._h, int(max_samples), int(interval_us)))

    def clock_trace_stop(self):
        """-> dict(t_ms, ghz: clock between consecutive samples; per_kernel: {kernel name: mean GHz over its launches' intervals,
        weighted by time}; intervals: [(kernel name, t0_ms, t1_ms)])"""
        ns, ni = C.c_int64(0), C.c_int64(0)
        L.check(self._lib.natac_clock_trace_stop(self._h, C.byref(ns), C.byref(ni)))
        t, cyc = np.empty(ns.value, np.float64), np.empty(ns.value, np.float64)
        ik, i0, i1 = np.empty(ni.value, np.int32), np.empty(ni.value, np.float64), np.empty(ni.value, np.float64)
        L.check(self._lib.natac_clock_trace_fetch(self._h, ns.value, _ptr(t), _ptr(cyc), ni.value, _ptr(ik), _ptr(i0), _ptr(i1)))
        dt = np.diff(t)
        ghz = np.where(dt > 0, np.diff(cyc) / np.maximum(dt, 1e-12) / 1e6, np.nan)     # cycles per ms / 1e6 = GHz
        if len(dt):      # the two counters are read a few cycles apart: a slope over a very short interval (or a wrapped counter) is noise
            ghz[(dt < 0.25 * np.median(dt)) | ~(ghz > 0) | (ghz > 10.0)] = np.nan
        mid = 0.5 * (t[1:] + t[:-1])
        per, w = {}, {}
        for k, a, b in zip(ik, i0, i1):
            m = (mid >= a) & (mid <= b) & np.isfinite(ghz)
            if m.any():
                name = L.KERNEL_NAMES[int(k)]
                per[name] = per.get(name, 0.0) + float(np.sum(ghz[m] * dt[m]))
                w[name] = w.get(name, 0.0) + float(np.sum(dt[m]))
        return dict(t_ms=t, ghz=ghz, per_kernel={k: per[k] / w[k] for k in per},
                    intervals=[(L.KERNEL_NAMES[int(k)], float(a), float(b)) for k, a, b in zip(ik, i0, i1)])

    def timer_start(self):
        L.check(self._lib.natac_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_double(0)
        L.check(self._lib.natac_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def upload(self, packed):
        return DeviceBatch(self, packed)


class DeviceBatch(object):
    """a PackedChunks batch resident in HBM (natac_batch) and its per-base output tracks"""

    def __init__(self, ctx, packed):
        if not isinstance(packed, PackedChunks):
            raise TypeError("expected PackedChunks")
        self.ctx = ctx
        self._lib = ctx._lib
        self.packed = packed
        h = C.c_void_p()
        if getattr(packed, "seq", None) is not None:        # Tn5 bias scored on the device from the sequence windows
            L.check(self._lib.natac_batch_create_from_seq(
                ctx._h, packed.n_chunks, _ptr(packed.chunk_len), _ptr(packed.frag_off), _ptr(packed.frag_lpos), _ptr(packed.frag_ilen),
                _ptr(packed.seq_off), _ptr(packed.seq), _ptr(packed.pwm_log), _ptr(packed.pwm_nucs), packed.pwm_log.shape[0],
                packed.pwm_log.shape[1], int(packed.bias_left), int(packed.bias_right), C.byref(h)))
        else:
            L.check(self._lib.natac_batch_create(
                ctx._h, packed.n_chunks, _ptr(packed.chunk_len), _ptr(packed.frag_off), _ptr(packed.frag_lpos),
                _ptr(packed.frag_ilen), _ptr(packed.bias_off) if packed.bias_log is not None else None,
                _ptr(packed.bias_log), int(packed.bias_left), int(packed.bias_right), C.byref(h)))
        self._h = h
        self.total_bp = packed.total_bp
        ctx._batches.add(self)

    def free(self):
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):       # never touch a batch whose context is gone
                self._lib.natac_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def release_outputs(self):
        """free every output array of the batch, keep the packed inputs in HBM (natac_batch_release_outputs)"""
        L.check(self._lib.natac_batch_release_outputs(self._h))

    def run_nuc(self, smooth_sd=10):
        L.check(self._lib.natac_run_nuc(self._h, float(smooth_sd)))

    def run_occ(self):
        L.check(self._lib.natac_run_occ(self._h))

    def run_ins(self, lower=0, upper=2000):
        L.check(self._lib.natac_run_ins(self._h, int(lower), int(upper)))

    def run_ins_smooth(self, w, lower=0, upper=2000, wsum=None):
        """`pyatac ins --smooth` for every chunk (natac_run_ins_smooth): the insertions of [start - M//2, end + M//2) smoothed by the
        odd-length window w and divided by wsum (default: np.convolve(w, ones(M), 'valid')[0], utils.smooth's norm=True).  The batch
        must be packed with a margin that holds every fragment with an end within M//2 of a chunk.  Fills T_INS_SMOOTH."""
        w = _f64(w)
        if wsum is None:
            wsum = float(np.convolve(w, np.ones(w.shape[0]), "valid")[0]) if w.shape[0] else 0.0
        L.check(self._lib.natac_run_ins_smooth(self._h, int(lower), int(upper), _ptr(w), w.shape[0], float(wsum)))

    def run_center_cov(self, window, mult, lower=0, upper=2000):
        """`pyatac cov` for every chunk (natac_run_center_cov): fragment centres within window//2 of every base times mult
        (scale / float(window)).  Fills T_CENTER_COV."""
        L.check(self._lib.natac_run_center_cov(self._h, int(lower), int(upper), int(window), float(mult)))

    def run_pwm_track(self, seq_off, seq, pwm_log, nucleotides):
        """`pyatac bias` for every chunk (natac_run_pwm_track): seq[seq_off[i]:seq_off[i+1]] = the chunk_len[i] + K - 1 bases under
        chunk i's track (uint8, any case), pwm_log = log(PWM.mat) of shape (nrow, K), nucleotides = its row letters (a uint8 array, or
        the PWM's list of one-letter strings).  The batch needs no fragments.  Fills T_BIAS, bit-identical to Context.pwm_bias."""
        so = np.ascontiguousarray(seq_off, dtype=np.int64)
        sq = np.ascontiguousarray(seq, dtype=np.uint8)
        logp = _f64(pwm_log)
        if not isinstance(nucleotides, np.ndarray):
            if set(len(x) for x in nucleotides) != {1}:
                raise NotImplementedError("k-mer PWMs are not supported by natac_run_pwm_track: single-nucleotide PWMs only")
            nucleotides = np.frombuffer("".join(nucleotides).encode("ascii"), dtype=np.uint8)
        nucs = np.ascontiguousarray(nucleotides, dtype=np.uint8)
        if logp.ndim != 2 or nucs.shape != (logp.shape[0],):
            raise ValueError("pwm_log must be (nrow, K) with one letter per row")
        if so.shape != (self.packed.n_chunks + 1,) or so[-1] != sq.shape[0]:
            raise ValueError("seq_off needs n_chunks + 1 entries that end at len(seq)")
        L.check(self._lib.natac_run_pwm_track(self._h, _ptr(so), _ptr(sq), _ptr(logp), _ptr(nucs), logp.shape[0], logp.shape[1]))

    def run_candidates(self, cand_chunk, cand_pos):
        cc =np.ascontiguousarray(cand_chunk, dtype=np.int32)
        cp = np.ascontiguousarray(cand_pos, dtype=np.int32)
        if cc.shape != cp.shape:
            raise ValueError("cand_chunk / cand_pos shape mismatch")
        n = cc.shape[0]
        lr, var, z = (np.empty(n, dtype=np.float64) for _ in range(3))
        L.check(self._lib.natac_run_candidates(self._h, n, _ptr(cc), _ptr(cp), _ptr(lr), _ptr(var), _ptr(z)))
        return lr, var, z

    def run_candidates_cov(self, cand_chunk, cand_pos, mode="closed"):
        """calculateCov at many candidates in one arithmetic variant (natac_run_candidates_cov): "closed" (fp64 closed form),
        "literal" (the .pyx's O(N^2) pair sum, fp64) or "fp32" (closed form in float)"""
        cc = np.ascontiguousarray(cand_chunk, dtype=np.int32)
        cp = np.ascontiguousarray(cand_pos, dtype=np.int32)
        if cc.shape != cp.shape:
            raise ValueError("cand_chunk / cand_pos shape mismatch")
        var = np.empty(cc.shape[0], dtype=np.float64)
        L.check(self._lib.natac_run_candidates_cov(self._h, cc.shape[0], _ptr(cc), _ptr(cp),
                                                   {"closed": 0, "literal": 1, "fp32": 2}[mode], _ptr(var)))
        return var

    def run_peaks(self, min_signal=0.0, sep=25, boundary=60, order=12, download=True):
        """candidate search + LR / var / z on the device (natac_run_peaks): call_peaks(norm + smoothed, ...) of every chunk
        as NucChunk.findAllNucs does it (nucleoatac/NucleosomeCalling.py:297-301).  Returns (chunk, pos, lr, var, z), or with
        download=False only the number of candidates (the arrays stay in HBM for download_peaks)."""
        maxL = int(self.packed.chunk_len.max())
        jitter = np.ascontiguousarray(np.random.RandomState(seed=25).uniform(0, 10 ** -12, maxL))   # utils.py:94-97
        n = C.c_int64(0)
        L.check(self._lib.natac_run_peaks(self._h, float(min_signal), int(sep), int(boundary), int(order), _ptr(jitter), maxL,
                                          C.byref(n)))
        n = n.value
        if not download:
            return n
        return self.download_peaks(n)

    def download_peaks(self, n):
        """(chunk, pos, lr, var, z) of the last run_peaks"""
        cc, cp = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        lr, var, z = (np.empty(n, dtype=np.float64) for _ in range(3))
        L.check(self._lib.natac_download_peaks(self._h, n, _ptr(cc), _ptr(cp), _ptr(lr), _ptr(var), _ptr(z)))
        return cc, cp, lr, var, z

    def run_track_peaks(self, track, min_signal=0.0, sep=120, boundary=None, order=1):
        """utils.call_peaks on one per-base track of every chunk, on the device (natac_run_track_peaks).
        Returns (chunk, pos) arrays in chunk order."""
        if boundary is None:
            boundary = sep // 2
        maxL = int(self.packed.chunk_len.max())
        jitter = np.ascontiguousarray(np.random.RandomState(seed=25).uniform(0, 10 ** -12, maxL))
        n = C.c_int64(0)
        L.check(self._lib.natac_run_track_peaks(self._h, int(track), float(min_signal), int(sep), int(boundary), int(order),
                                                _ptr(jitter), maxL, C.byref(n)))
        n = n.value
        cc, cp = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        L.check(self._lib.natac_download_peaks(self._h, n, _ptr(cc), _ptr(cp), None, None, None))
        return cc, cp

    def run_occ_peaks(self, min_occ=0.1, sep=120):
        """OccChunk.callPeaks + getNucDist of every chunk on the device (natac_run_occ_peaks).  Returns
        (chunk, pos, occ, lower, upper, reads, keep) of every call_peaks peak and nuc_dist[n_chunks, upper]."""
        maxL = int(self.packed.chunk_len.max())
        jitter = np.ascontiguousarray(np.random.RandomState(seed=25).uniform(0, 10 ** -12, maxL))
        n = C.c_int64(0)
        L.check(self._lib.natac_run_occ_peaks(self._h, float(min_occ), int(sep), _ptr(jitter), maxL, C.byref(n)))
        n = n.value
        cc, cp, keep = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int32)
        occ, lo, up, rd = (np.empty(n, np.float64) for _ in range(4))
        L.check(self._lib.natac_download_occ_peaks(self._h, n, _ptr(cc), _ptr(cp), _ptr(occ), _ptr(lo), _ptr(up), _ptr(rd), _ptr(keep)))
        # the context's size range is the run's here: natac_run_occ_peaks above refuses (NATAC_E_STATE) when the occupancy geometry
        # was changed after natac_run_occ, and natac_download_nuc_dist checks the buffer's size against the run's
        upper = self.ctx.occ_upper
        nd = np.empty((self.packed.n_chunks, upper), dtype=np.float64)
        L.check(self._lib.natac_download_nuc_dist(self._h, _ptr(nd), nd.nbytes))
        return cc, cp, occ, lo, up, rd, keep, nd

    def format_track(self, t, chroms, chunk_start, write_zero=True, compress=True, keep_runs_before_nan=False, out=None, wait=True):
        """Track.write_track of per-base track `t` for every chunk ON THE DEVICE (natac_batch_format_track): returns
        (bytes as a uint8 array -- bedGraph text, or BGZF members when `compress` --, info dict).  `chroms`: one chromosome name
        per chunk; `out`: a function n_bytes -> uint8 buffer (e.g. a pinned slot) that receives the result.  `wait=False`: the copy into
        `out`'s (pinned) buffer is only STARTED (natac_batch_format_fetch_begin) so that the next track can be formatted meanwhile; the
        bytes are valid after `format_wait()`."""
        nc = self.packed.n_chunks
        if len(chroms) != nc or len(chunk_start) != nc:
            raise ValueError("one chromosome name and start per chunk")
        # the name table of a batch is formed once, not once per track: a per-chunk Python loop here (str(), a dict lookup) holds the GIL for
        # ~2 ms per 2,500 chunks -- with five tracks per sub-batch and six executor threads that serialised the whole bedGraph.gz
        # pipeline on the interpreter (round 6: kernels busy 55 % of the leg's wall time)
        key = (id(chroms), id(chunk_start))
        cached = getattr(self, "_fmt_names", None)
        if cached is None or cached[0] != key:
            uniq, inv = np.unique(np.asarray(chroms, dtype=str), return_inverse=True)      # sorted, like sorted(set(...))
            names = [str(c) for c in uniq]
            cached = (key, names, np.ascontiguousarray(inv, dtype=np.int32), np.ascontiguousarray(chunk_start, dtype=np.int64),
                      (C.c_char_p * len(names))(*[c.encode("ascii") for c in names]), chroms, chunk_start)   # (the two objects are kept alive: id() stays theirs)
            self._fmt_names = cached
        _, names, cid, cs, arr = cached[:5]
        nb, nt, nl, hard = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        L.check(self._lib.natac_batch_format_track(self._h, int(t), _ptr(cid), arr, len(names), _ptr(cs),
                                                   (1 if write_zero else 0) | (2 if keep_runs_before_nan else 0), 1 if compress else 0,
                                                   C.byref(nb), C.byref(nt), C.byref(nl), C.byref(hard)))
        buf = out(nb.value) if out is not None else np.empty(nb.value, dtype=np.uint8)
        if buf.dtype != np.uint8 or buf.size < nb.value:
            raise ValueError("out must give a uint8 buffer of at least %d bytes" % nb.value)
        if wait:
            L.check(self._lib.natac_batch_format_fetch(self._h, _ptr(buf), buf.nbytes))
        else:
            L.check(self._lib.natac_batch_format_fetch_begin(self._h, _ptr(buf), buf.nbytes))
        info = dict(bytes=nb.value, text_bytes=nt.value, lines=nl.value, hard=hard.value)
        if compress:
            # tabix records of this result (runs of lines per 16-kb leaf bin) for writer.TbiBuilder.push
            ng, nm, ntx = C.c_int64(0), C.c_int64(0), C.c_int64(0)
            L.check(self._lib.natac_batch_format_index_size(self._h, C.byref(ng), C.byref(nm), C.byref(ntx)))
            ng, nm = ng.value, nm.value
            rec = dict(names=names, n_text=ntx.value, cid=np.empty(ng, np.int32), beg=np.empty(ng, np.int64), end=np.empty(ng, np.int64),
                       count=np.empty(ng, np.int64), t0=np.empty(ng, np.uint64), t1=np.empty(ng, np.uint64),
                       member_pos=np.zeros(nm + 1, np.uint64))
            L.check(self._lib.natac_batch_format_index_fetch(self._h, _ptr(rec["cid"]), _ptr(rec["beg"]), _ptr(rec["end"]), _ptr(rec["count"]),
                                                             _ptr(rec["t0"]), _ptr(rec["t1"]), _ptr(rec["member_pos"])))
            info["index"] = rec
        return buf[:nb.value], info

    def format_wait(self):
        """wait for every result whose copy `format_track(..., wait=False)` started"""
        L.check(self._lib.natac_batch_format_fetch_wait(self._h))

    def set_track(self, t, vals):
        """overwrite float64 per-base track `t` with host values (natac_batch_set_track), e.g. to send an externally computed
        track through the device-side writer"""
        v = _f64(vals)
        L.check(self._lib.natac_batch_set_track(self._h, int(t), _ptr(v), v.shape[0]))

    def track(self, t, out=None):
        """download one per-base track (concatenated over chunks); `out`: destination array (e.g. pinned_empty)"""
        dt = np.int32 if t == L.T_INS else np.float64
        if out is None:
            out = np.empty(self.total_bp, dtype=dt)
        elif out.dtype != dt or out.size != self.total_bp or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous %s array of %d elements" % (dt.__name__, self.total_bp))
        L.check(self._lib.natac_batch_download(self._h, int(t), _ptr(out), out.nbytes))
        return out

    def grid_info(self):
        bp, grid, nf = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L.check(self._lib.natac_batch_info(self._h, C.byref(bp), C.byref(grid), C.byref(nf)))
        return bp.value, grid.value, nf.value

    def grid(self, which):
        _, total_grid, _ = self.grid_info()
        out = np.empty(total_grid, dtype=np.float64)
        L.check(self._lib.natac_batch_download_grid(self._h, int(which), _ptr(out), out.nbytes))
        return out

    def status(self):
        out = np.empty(self.packed.n_chunks, dtype=np.int32)
        L.check(self._lib.natac_batch_status(self._h, _ptr(out), out.nbytes))
        return out

    def split(self, flat):
        """split a concatenated per-base array into per-chunk views"""
        off = self.packed.out_off
        return [flat[int(off[i]):int(off[i + 1])] for i in range(self.packed.n_chunks)]
