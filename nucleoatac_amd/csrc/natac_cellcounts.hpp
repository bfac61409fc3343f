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
