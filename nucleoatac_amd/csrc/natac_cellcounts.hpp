// natac_cellcounts.hpp -- the kernels behind `pyatac cellcounts` (this package's own command: the reference has no such tool): the
// cell-by-region count matrix of one chromosome, CSR with one row per region (natac_region_cell_counts, include/natac.h).
//
// The candidates of a region and its number of counting records h ("hits") come from natac_sites.hpp (natac_region_ranges,
// natac_region_count_short / _long: the counting rule is region_record_hit there, asked again here).  A row's cells are then reduced by h:
//   cc_rows_wave    h <= CC_WAVE_MAX: one wave per row.  The hit cells are gathered through 64 words of LDS per wave, sorted by a
//                   bitonic network over the lanes (shuffles) and run-length encoded with one ballot.
//   cc_rows_block   h <= CC_SHORT_MAX: one workgroup per row.  The hit cells are gathered into LDS (at most 16 KiB of keys: a cell index is
//                   below 2^23), sorted there by a bitonic network and run-length encoded with a block scan of the run heads.
//   cc_long_*       longer rows, one at a time: every hit adds 1 to a dense array of n_cells 32-bit counters in global memory (integer
//                   atomicAdd: exact in any order), then the non-zero counters are compacted in cell order and the array is cleared.
// Every arm writes (cell, count) pairs, cell ascending, at the row's offset of a staging area (a row needs at most min(h, n_cells)
// pairs) and the row's number of pairs; a scan of those gives row_ptr, and cc_gather_rows / cc_gather_long move the pairs to their place.
// Nothing depends on the order of records, waves or blocks: the sort, not the gather order, fixes a row's layout.
// Behind the kernels: the entry point, which picks every row's arm on the host between two waits.
#pragma once
#include <hip/hip_runtime.h>

#include "natac_sites.hpp"

namespace natac_cellcounts {

using natac_sites::region_record_hit;

constexpr int CC_BLOCK = 256;               // 4 waves
constexpr int CC_WAVE_MAX = 64;             // NATAC_CELLCOUNT_WAVE_MAX: one key per lane
constexpr int CC_SHORT_MAX = 4096;          // NATAC_CELLCOUNT_SHORT_MAX: keys + run heads = 32 KiB of LDS per workgroup
constexpr int CC_CELLS_PER_BLOCK = 2048;    // cells per block of the long arm's compaction (8 per thread)
constexpr unsigned CC_PAD = 0xffffffffu;    // sorts behind every cell index

__device__ __forceinline__ unsigned long long cc_lanes_below(int lane) { return (1ULL << lane) - 1ULL; }

// rows of 1 .. CC_WAVE_MAX hits: one wave each
__global__ void __launch_bounds__(CC_BLOCK) cc_rows_wave(const long long *__restrict__ pos, const long long *__restrict__ tlen,
                                                         const int *__restrict__ cell, long long nr, const long long *__restrict__ start,
                                                         const long long *__restrict__ end, const long long *__restrict__ cand_lo,
                                                         const long long *__restrict__ cand_n, const unsigned long long *__restrict__ hits,
                                                         const unsigned long long *__restrict__ stage_off, int lower, int upper, int shift,
                                                         int trim, int *__restrict__ stage_col, int *__restrict__ stage_val,
                                                         unsigned long long *__restrict__ nnz) {
    __shared__ unsigned s_key[CC_BLOCK / 64][64];
    const int lane = threadIdx.x & 63;
    volatile unsigned *keys = s_key[threadIdx.x >> 6];      // this wave's own words: wave barriers order its writes and reads
    const long long nwaves = (long long)gridDim.x * (CC_BLOCK / 64);
    for (long long i = (long long)blockIdx.x * (CC_BLOCK / 64) + (threadIdx.x >> 6); i < nr; i += nwaves) {
        const unsigned long long h = hits[i];
        if (h == 0 || h > (unsigned long long)CC_WAVE_MAX) continue;       // (nnz is zero before the launch)
        const long long f0 = cand_lo[i], f1 = f0 + cand_n[i], s = start[i], e = end[i];
        unsigned base = 0;
        for (long long f = f0; f < f1; f += 64) {           // wave-uniform bounds: every lane takes part in every ballot
            const bool hit = f + lane < f1 && region_record_hit(pos[f + lane], tlen[f + lane], s, e, lower, upper, shift, trim);
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const unsigned r = base + (unsigned)__popcll(m & cc_lanes_below(lane));
                if (r < (unsigned)CC_WAVE_MAX) keys[r] = (unsigned)cell[f + lane];
            }
            base += (unsigned)__popcll(m);
        }
        __builtin_amdgcn_wave_barrier();
        unsigned key = (unsigned long long)lane < h ? keys[lane] : CC_PAD;
        __builtin_amdgcn_wave_barrier();                    // the next row writes the same words
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const unsigned o = (unsigned)__shfl_xor((int)key, j);
                const bool up = (lane & k) == 0, low = (lane & j) == 0;
                key = (low == up) ? (key < o ? key : o) : (key > o ? key : o);
            }
        const unsigned prev = (unsigned)__shfl_up((int)key, 1);
        const bool head = (unsigned long long)lane < h && (lane == 0 || key != prev);
        const unsigned long long hm = __ballot(head);
        if (head) {
            const unsigned long long rest = lane < 63 ? hm >> (lane + 1) : 0ULL;
            const int next = rest ? lane + 1 + __builtin_ctzll(rest) : (int)h;
            const unsigned long long o = stage_off[i] + (unsigned long long)__popcll(hm & cc_lanes_below(lane));
            stage_col[o] = (int)key;
            stage_val[o] = next - lane;
        }
        if (lane == 0) nnz[i] = (unsigned long long)__popcll(hm);
    }
}

// rows of CC_WAVE_MAX + 1 .. CC_SHORT_MAX hits (list[n_list], any order): one workgroup each
__global__ void __launch_bounds__(CC_BLOCK) cc_rows_block(const long long *__restrict__ pos, const long long *__restrict__ tlen,
                                                          const int *__restrict__ cell, const long long *__restrict__ list, long long n_list,
                                                          const long long *__restrict__ start, const long long *__restrict__ end,
                                                          const long long *__restrict__ cand_lo, const long long *__restrict__ cand_n,
                                                          const unsigned long long *__restrict__ hits,
                                                          const unsigned long long *__restrict__ stage_off, int lower, int upper, int shift,
                                                          int trim, int *__restrict__ stage_col, int *__restrict__ stage_val,
                                                          unsigned long long *__restrict__ nnz) {
    __shared__ unsigned s_key[CC_SHORT_MAX];
    __shared__ unsigned s_head[CC_SHORT_MAX + 1];           // s_head[q] = where run q starts in s_key; one more for the end
    __shared__ unsigned s_n, s_w[CC_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (long long k = blockIdx.x; k < n_list; k += gridDim.x) {
        const long long i = list[k];
        unsigned h = (unsigned)hits[i];
        if (h > (unsigned)CC_SHORT_MAX) h = CC_SHORT_MAX;  // (the host lists no such row)
        const long long f0 = cand_lo[i], f1 = f0 + cand_n[i], s = start[i], e = end[i];
        if (tid == 0) s_n = 0;
        __syncthreads();
        for (long long f = f0; f < f1; f += CC_BLOCK) {     // block-uniform bounds
            const bool hit = f + tid < f1 && region_record_hit(pos[f + tid], tlen[f + tid], s, e, lower, upper, shift, trim);
            const unsigned long long m = __ballot(hit);
            unsigned wb = 0;
            if (lane == 0 && m) wb = atomicAdd(&s_n, (unsigned)__popcll(m));
            wb = (unsigned)__shfl((int)wb, 0);
            if (hit) {
                const unsigned r = wb + (unsigned)__popcll(m & cc_lanes_below(lane));
                if (r < (unsigned)CC_SHORT_MAX) s_key[r] = (unsigned)cell[f + tid];
            }
        }
        unsigned P = 2 * CC_WAVE_MAX;                       // the power of two the network runs over
        while (P < h) P <<= 1;
        __syncthreads();
        for (unsigned t = h + tid; t < P; t += CC_BLOCK) s_key[t] = CC_PAD;
        __syncthreads();
        for (unsigned kk = 2; kk <= P; kk <<= 1)
            for (unsigned j = kk >> 1; j > 0; j >>= 1) {
                for (unsigned t = tid; t < P / 2; t += CC_BLOCK) {
                    const unsigned a = 2 * t - (t & (j - 1)), b = a + j;     // a has bit j clear
                    const unsigned x = s_key[a], y = s_key[b];
                    if ((x > y) == ((a & kk) == 0)) { s_key[a] = y; s_key[b] = x; }
                }
                __syncthreads();
            }
        unsigned carry = 0;                                 // runs before this pass (block-uniform)
        for (unsigned base = 0; base < h; base += CC_BLOCK) {
            const unsigned t = base + tid;
            const bool head = t < h && (t == 0 || s_key[t] != s_key[t - 1]);
            const unsigned long long m = __ballot(head);
            if (lane == 0) s_w[w] = (unsigned)__popcll(m);
            __syncthreads();
            unsigned before = carry;
            for (int q = 0; q < w; ++q) before += s_w[q];
            if (head) s_head[before + (unsigned)__popcll(m & cc_lanes_below(lane))] = t;
            carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
            __syncthreads();
        }
        if (tid == 0) s_head[carry] = h;
        __syncthreads();
        const unsigned long long o = stage_off[i];
        for (unsigned q = tid; q < carry; q += CC_BLOCK) {
            stage_col[o + q] = (int)s_key[s_head[q]];
            stage_val[o + q] = (int)(s_head[q + 1] - s_head[q]);
        }
        if (tid == 0) nnz[i] = carry;
        __syncthreads();                                    // the next row reuses the arrays
    }
}

// ---- a long row: dense[n_cells] (zero before and after) ----
__global__ void __launch_bounds__(CC_BLOCK) cc_long_count(const long long *__restrict__ pos, const long long *__restrict__ tlen,
                                                          const int *__restrict__ cell, long long row, const long long *__restrict__ start,
                                                          const long long *__restrict__ end, const long long *__restrict__ cand_lo,
                                                          const long long *__restrict__ cand_n, int lower, int upper, int shift, int trim,
                                                          unsigned *__restrict__ dense) {
    const long long f0 = cand_lo[row], f1 = f0 + cand_n[row], s = start[row], e = end[row];
    for (long long f = f0 + (long long)blockIdx.x * CC_BLOCK + threadIdx.x; f < f1; f += (long long)gridDim.x * CC_BLOCK)
        if (region_record_hit(pos[f], tlen[f], s, e, lower, upper, shift, trim)) atomicAdd(&dense[cell[f]], 1u);
}

// sums[b] = the non-zero counters among the cells of block b
__global__ void __launch_bounds__(CC_BLOCK) cc_long_block_nnz(const unsigned *__restrict__ dense, int n_cells,
                                                              unsigned long long *__restrict__ sums) {
    __shared__ unsigned red[CC_BLOCK / 64];
    const int base = blockIdx.x * CC_CELLS_PER_BLOCK + threadIdx.x * 8;
    unsigned n = 0;
    for (int j = 0; j < 8; ++j)
        if (base + j < n_cells && dense[base + j]) ++n;
    for (int off = 32; off > 0; off >>= 1) n += (unsigned)__shfl_xor((int)n, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (unsigned long long)red[0] + red[1] + red[2] + red[3];
}

// sums scanned (natac_textz::tz_scan_sums: exclusive, the total behind them): the non-zero counters go out in cell order and are cleared
__global__ void __launch_bounds__(CC_BLOCK) cc_long_compact(unsigned *__restrict__ dense, int n_cells,
                                                            const unsigned long long *__restrict__ sums, long long row,
                                                            const unsigned long long *__restrict__ stage_off, int *__restrict__ stage_col,
                                                            int *__restrict__ stage_val, unsigned long long *__restrict__ nnz) {
    __shared__ unsigned wtot[CC_BLOCK / 64];
    const int base = blockIdx.x * CC_CELLS_PER_BLOCK + threadIdx.x * 8;
    const int lane = threadIdx.x & 63;
    unsigned v[8], n = 0;
    for (int j = 0; j < 8; ++j) {
        v[j] = base + j < n_cells ? dense[base + j] : 0u;
        if (v[j]) { ++n; dense[base + j] = 0u; }
    }
    unsigned inc = n;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wtot[threadIdx.x >> 6] = inc;
    __syncthreads();
    unsigned long long o = stage_off[row] + sums[blockIdx.x] + (inc - n);
    for (int q = 0; q < (int)(threadIdx.x >> 6); ++q) o += wtot[q];
    for (int j = 0; j < 8; ++j)
        if (v[j]) {
            stage_col[o] = base + j;
            stage_val[o] = (int)v[j];
            ++o;
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) nnz[row] = sums[gridDim.x];
}

// ---- staging -> CSR ----
// one wave per row of at most CC_SHORT_MAX hits
__global__ void __launch_bounds__(CC_BLOCK) cc_gather_rows(long long nr, const unsigned long long *__restrict__ hits,
                                                           const unsigned long long *__restrict__ stage_off,
                                                           const unsigned long long *__restrict__ row_ptr, const int *__restrict__ stage_col,
                                                           const int *__restrict__ stage_val, int *__restrict__ col, int *__restrict__ val) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * (CC_BLOCK / 64);
    for (long long i = (long long)blockIdx.x * (CC_BLOCK / 64) + (threadIdx.x >> 6); i < nr; i += nwaves) {
        if (hits[i] > (unsigned long long)CC_SHORT_MAX) continue;
        const unsigned long long a = row_ptr[i], n = row_ptr[i + 1] - a, o = stage_off[i];
        for (unsigned long long q = lane; q < n; q += 64) {
            col[a + q] = stage_col[o + q];
            val[a + q] = stage_val[o + q];
        }
    }
}

// one long row over the whole grid
__global__ void __launch_bounds__(CC_BLOCK) cc_gather_long(long long row, const unsigned long long *__restrict__ stage_off,
                                                           const unsigned long long *__restrict__ row_ptr, const int *__restrict__ stage_col,
                                                           const int *__restrict__ stage_val, int *__restrict__ col, int *__restrict__ val) {
    const unsigned long long a = row_ptr[row], n = row_ptr[row + 1] - a, o = stage_off[row];
    for (unsigned long long q = (unsigned long long)blockIdx.x * CC_BLOCK + threadIdx.x; q < n; q += (unsigned long long)gridDim.x * CC_BLOCK) {
        col[a + q] = stage_col[o + q];
        val[a + q] = stage_val[o + q];
    }
}

}  // namespace natac_cellcounts

// ---- entry point -----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_region_cell_counts(natac_ctx *c, int64_t nf, const int64_t *pos, const int64_t *tlen, const int32_t *cell, int32_t n_cells,
                             int64_t nr, const int64_t *start, const int64_t *end, int lower, int upper, int atac, int64_t *row_ptr, int64_t cap,
                             int32_t *col, int32_t *val, double *kernel_ms) {
    using namespace natac_cellcounts;
    static_assert(CC_WAVE_MAX == NATAC_CELLCOUNT_WAVE_MAX && CC_SHORT_MAX == NATAC_CELLCOUNT_SHORT_MAX, "the arms' bounds are in natac.h");
    if (!c || !row_ptr) return fail(NATAC_E_ARG, "null argument");
    if (nf < 0 || nr < 0 || cap < 0) return fail(NATAC_E_ARG, "negative size");
    if ((nf > 0 && (!pos || !tlen || !cell)) || (nr > 0 && (!start || !end))) return fail(NATAC_E_ARG, "null argument");
    if (!col != !val || (!col && cap != 0)) return fail(NATAC_E_ARG, "col and val go together; a sizing call passes neither and cap 0");
    if (n_cells < 1 || n_cells > NATAC_SPLIT_MAX_BARCODES) return fail(NATAC_E_ARG, "n_cells must be in [1, %d] (got %d)", NATAC_SPLIT_MAX_BARCODES, n_cells);
    if (upper <= lower) return fail(NATAC_E_ARG, "upper (%d) <= lower (%d)", upper, lower);
    if (nf >= (1LL << 40) || nr >= (1LL << 40)) return fail(NATAC_E_ARG, "too many records or regions in one call");
    if (kernel_ms) *kernel_ms = 0;
    if (const int rc = check_intervals("region", nr, start, end, false)) return rc;
    if (const int rc = check_fragments(nf, pos, tlen, cell, n_cells)) return rc;
    for (int64_t i = 0; i <= nr; ++i) row_ptr[i] = 0;
    if (nr == 0 || nf == 0) return NATAC_OK;
    DeviceCall dc(c, "region_cell_counts");
    const long long *d_pos = dc.upload((const long long *)pos, (size_t)nf), *d_tlen = dc.upload((const long long *)tlen, (size_t)nf);
    const int *d_cell = dc.upload((const int *)cell, (size_t)nf);
    const long long *d_s = dc.upload((const long long *)start, (size_t)nr), *d_e = dc.upload((const long long *)end, (size_t)nr);
    long long *d_lo = dc.alloc<long long>((size_t)nr), *d_n = dc.alloc<long long>((size_t)nr), *d_long = dc.alloc<long long>((size_t)nr);
    unsigned long long *d_hits = dc.zeroed<unsigned long long>((size_t)nr + 1);     // hits[nr], then natac_region_ranges' long-region count
    const int shift = atac ? 4 : 0, trim = atac ? 8 : 0;
    // the events span the whole call on the stream: its kernels and the two host round trips between them
    dc.time_begin(kernel_ms);
    // (1) candidates and hits per row, as natac_region_counts
    region_hits(dc, c, d_pos, d_tlen, nf, nr, d_s, d_e, lower, upper, shift, trim, d_lo, d_n, d_long, d_hits);
    std::vector<unsigned long long> h_hits((size_t)nr);
    dc.fetch(h_hits.data(), d_hits, (size_t)nr);
    if (const int rc = dc.sync()) return rc;
    // (2) the arm of every row and its place in the staging area: a row of h hits has at most min(h, n_cells) pairs
    std::vector<unsigned long long> h_off((size_t)nr + 1);
    std::vector<long long> mid_rows, long_rows;
    unsigned long long n_stage = 0;
    for (int64_t i = 0; i < nr; ++i) {
        const unsigned long long h = h_hits[(size_t)i];
        if (h > 2147483647ULL) return fail(NATAC_E_ARG, "region %lld: %llu counting records, more than 2147483647", (long long)i, h);
        h_off[(size_t)i] = n_stage;
        n_stage += std::min<unsigned long long>(h, (unsigned long long)n_cells);
        if (h > (unsigned long long)CC_SHORT_MAX) long_rows.push_back(i);
        else if (h > (unsigned long long)CC_WAVE_MAX) mid_rows.push_back(i);
    }
    h_off[(size_t)nr] = n_stage;
    const unsigned long long *d_off = dc.upload(h_off.data(), h_off.size());
    int *d_scol = dc.alloc<int>((size_t)n_stage), *d_sval = dc.alloc<int>((size_t)n_stage);
    unsigned long long *d_nnz = dc.zeroed<unsigned long long>((size_t)nr);
    unsigned long long *d_rp = dc.alloc<unsigned long long>((size_t)nr + 1);
    if (dc.ok()) {
        const unsigned bx = (unsigned)std::min<long long>((nr + CC_BLOCK / 64 - 1) / (CC_BLOCK / 64), 16384);
        hipLaunchKernelGGL(cc_rows_wave, dim3(bx), dim3(CC_BLOCK), 0, c->stream, d_pos, d_tlen, d_cell, (long long)nr, d_s, d_e, d_lo, d_n, d_hits,
                           d_off, lower, upper, shift, trim, d_scol, d_sval, d_nnz);
        dc.launched();
    }
    if (!mid_rows.empty()) {
        const long long *d_list = dc.upload(mid_rows.data(), mid_rows.size());
        if (dc.ok()) {
            const unsigned bx = (unsigned)std::min<size_t>(mid_rows.size(), 16384);
            hipLaunchKernelGGL(cc_rows_block, dim3(bx), dim3(CC_BLOCK), 0, c->stream, d_pos, d_tlen, d_cell, d_list, (long long)mid_rows.size(), d_s,
                               d_e, d_lo, d_n, d_hits, d_off, lower, upper, shift, trim, d_scol, d_sval, d_nnz);
            dc.launched();
        }
    }
    const unsigned cell_blocks = (unsigned)(((long long)n_cells + CC_CELLS_PER_BLOCK - 1) / CC_CELLS_PER_BLOCK);
    if (!long_rows.empty()) {
        unsigned *d_dense = dc.zeroed<unsigned>((size_t)n_cells);
        unsigned long long *d_sums = dc.alloc<unsigned long long>((size_t)cell_blocks + 1);
        for (const long long row : long_rows) {             // one long row at a time: they share the counters
            if (!dc.ok()) break;
            hipLaunchKernelGGL(cc_long_count, dim3(2048), dim3(CC_BLOCK), 0, c->stream, d_pos, d_tlen, d_cell, row, d_s, d_e, d_lo, d_n, lower,
                               upper, shift, trim, d_dense);
            hipLaunchKernelGGL(cc_long_block_nnz, dim3(cell_blocks), dim3(CC_BLOCK), 0, c->stream, d_dense, (int)n_cells, d_sums);
            hipLaunchKernelGGL(natac_textz::tz_scan_sums, dim3(1), dim3(1024), 0, c->stream, d_sums, (long long)cell_blocks);
            hipLaunchKernelGGL(cc_long_compact, dim3(cell_blocks), dim3(CC_BLOCK), 0, c->stream, d_dense, (int)n_cells, d_sums, row, d_off, d_scol,
                               d_sval, d_nnz);
            dc.launched();
        }
    }
    // (3) row_ptr = the scan of the rows' pair counts
    dev_scan(c, d_nnz, (long long)nr, d_rp, dc);
    dc.fetch(row_ptr, d_rp, (size_t)nr + 1);
    if (const int rc = dc.sync()) {
        for (int64_t i = 0; i <= nr; ++i) row_ptr[i] = 0;
        return rc;
    }
    const int64_t nnz = row_ptr[nr];
    if (!col || nnz > cap) {
        dc.time_end();
        const int rc = dc.finish();
        if (rc) return rc;
        if (!col) return NATAC_OK;                          // the sizing call
        return fail(NATAC_E_ARG, "cap %lld is less than the %lld entries of the matrix", (long long)cap, (long long)nnz);
    }
    // (4) staging -> CSR
    int *d_col = dc.alloc<int>((size_t)nnz), *d_val = dc.alloc<int>((size_t)nnz);
    if (dc.ok() && nnz) {
        const unsigned bx = (unsigned)std::min<long long>((nr + CC_BLOCK / 64 - 1) / (CC_BLOCK / 64), 16384);
        hipLaunchKernelGGL(cc_gather_rows, dim3(bx), dim3(CC_BLOCK), 0, c->stream, (long long)nr, d_hits, d_off, d_rp, d_scol, d_sval, d_col, d_val);
        for (const long long row : long_rows)
            hipLaunchKernelGGL(cc_gather_long, dim3(1024), dim3(CC_BLOCK), 0, c->stream, row, d_off, d_rp, d_scol, d_sval, d_col, d_val);
        dc.launched();
    }
    dc.time_end();
    dc.fetch(col, d_col, (size_t)nnz);
    dc.fetch(val, d_val, (size_t)nnz);
    return dc.finish();
}

}  // extern "C"
