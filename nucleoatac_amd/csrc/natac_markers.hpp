// natac_markers.hpp -- the kernels behind `pyatac markers` (this package's own command: the reference has no such tool): for every window
// and every cell group the exact integers a Wilcoxon rank-sum test of depth-normalised accessibility needs (natac_group_rank_sums,
// include/natac.h states the rule), and the host-only launch plan (natac_group_rank_sums_plan).
//
// The counts arrive as natac_region_cell_counts leaves them: CSR with one row per window (m of them), the cells (N = n) ascending
// within a row.  Cell c has depth d[c] in [1, 2^31) and group grp[c] in [0, G).  Row p has L entries (c, a) and z0 = N - L cells at
// value 0; an entry's value is the exact rational a / d[c].  Two values are compared through the 64-bit products a_i * d_j and
// a_j * d_i (both factors below 2^31): less_i / eq_i count the row's entries below / equal to entry i (eq_i counts i itself), and
//   2 rank_i = 2 z0 + 2 less_i + eq_i + 1,      2 rank of a zero cell = z0 + 1.
// Per row and group g with n_g cells:  detected = its entries, total = the sum of their counts,
//   rank2 = (n_g - detected)(z0 + 1) + sum over its entries of 2 rank_i,     and per row  ties = (z0^3 - z0) + sum of (eq_i^2 - 1).
//
// Three kernels by row length, the rows of each listed by the entry point from the plan (mk_plan):
//   mk_short  L <= short_max (<= 64): a lane group of 16 / 32 / 64 lanes per row, one entry per lane; every lane reads the other entries
//             of its row by cross-lane reads (all pairs, no sort).
//   mk_block  L <= block_max: a workgroup per row, the row's (count, depth) pairs and groups in LDS, sorted there (bitonic, by the exact
//             comparison); an entry's less / eq are the start and the length of its run of equal values, found by two binary searches.
//   long      beyond: mk_long_sort sorts the row's chunks of `chunk` entries in LDS (bitonic, by the exact comparison) into a work
//             buffer; mk_long_rank gives every entry its less / eq by a lower- and an upper-bound search in each sorted chunk of its row,
//             a workgroup per chunk of entries: L / chunk searches of log2(chunk) steps per entry instead of L comparisons.
// The per-group sums of a row (or of a chunk of a long row) are integer counters in LDS, added with LDS atomics; the workgroups of a long
// row add theirs to the outputs with global integer atomics, onto the values mk_long_sort's first chunk left there.  Integer adds
// commute and there is no floating point on the device: the outputs are a pure function of the operands under every threshold.
// Behind the kernels: the entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "natac_runtime.hpp"

namespace natac_mk {

typedef unsigned long long u64;

constexpr int MK_SHORT_MAX = 64;            // NATAC_MARKERS_SHORT_CAP: a wave's lanes
constexpr int MK_BLOCK_MAX = 8192;          // NATAC_MARKERS_BLOCK_CAP: 9 bytes of LDS an entry, 72 KiB + the counters: two workgroups a CU
constexpr int MK_LONG_CHUNK = 4096;         // the entries mk_long_sort sorts at once: 32 KiB of LDS
constexpr int MK_MIN_CHUNK = 16;
constexpr int MK_WG_SHORT = 256, MK_WG_BLOCK = 256, MK_WG_LONG = 256;
constexpr long long MK_MAX_OUT = 1LL << 25; // NATAC_MARKERS_MAX_OUT
constexpr long long MK_MAX_N = 1LL << 20;   // NATAC_MARKERS_MAX_CELLS
constexpr int MK_MAX_G = 255;               // NATAC_MARKERS_MAX_GROUPS

// the operands every kernel reads and the outputs every kernel writes
struct MkArgs {
    const long long *row_ptr;      // [m + 1], counted from the call's first entry
    const int *col, *count;        // [nnz]
    const int *depth;              // [N]
    const unsigned char *grp;      // [N]
    const int *n_in_group;         // [G]
    int N, G;
    int *detected;                 // [m x G]
    long long *total, *rank2;      // [m x G]
    long long *ties;               // [m]
};

// the per-group counters of `slots` rows: u64 tot[slots * G], rank[slots * G], then unsigned det[slots * G]
__host__ __device__ static inline size_t mk_counter_bytes(int slots, int G) {
    return ((size_t)slots * G * 20 + 15) / 16 * 16;
}

__device__ static inline u64 mk_cube_minus(long long z) { return (u64)z * (u64)z * (u64)z - (u64)z; }

// one row's (or one slot's) counters into the outputs: threads t = first, first + step, ... of the row's owners
__device__ static inline void mk_flush_row(const MkArgs &A, int p, long long z0, const u64 *tot, const u64 *rank, const unsigned *det,
                                           int first, int step) {
    for (int g = first; g < A.G; g += step) {
        const size_t o = (size_t)p * A.G + g;
        const unsigned dt = det[g];
        A.detected[o] = (int)dt;
        A.total[o] = (long long)tot[g];
        A.rank2[o] = (long long)((u64)(A.n_in_group[g] - (long long)dt) * (u64)(z0 + 1) + rank[g]);
    }
}

// ---- short arm: a lane group per row ----
__global__ void __launch_bounds__(MK_WG_SHORT) mk_short(MkArgs A, const int *__restrict__ rows, int n_rows, int lanes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mk_lds[];
    const int slots = MK_WG_SHORT / lanes;
    u64 *s_tot = (u64 *)mk_lds, *s_rank = s_tot + (size_t)slots * A.G;
    unsigned *s_det = (unsigned *)(s_rank + (size_t)slots * A.G);
    const int tid = threadIdx.x, lane = tid & 63, slot = tid / lanes, sub = tid & (lanes - 1), first = lane & ~(lanes - 1);
    u64 *tot = s_tot + (size_t)slot * A.G, *rank = s_rank + (size_t)slot * A.G;
    unsigned *det = s_det + (size_t)slot * A.G;
    for (long long base = (long long)blockIdx.x * slots; base < n_rows; base += (long long)gridDim.x * slots) {     // workgroup-uniform
        const bool have = base + slot < n_rows;
        const int p = have ? rows[base + slot] : 0;
        const long long e0 = have ? A.row_ptr[p] : 0;
        const int L = have ? (int)(A.row_ptr[p + 1] - e0) : 0;
        const long long z0 = A.N - L;
        for (int g = sub; g < A.G; g += lanes) { tot[g] = 0; rank[g] = 0; det[g] = 0; }
        unsigned a = 0, d = 1, grp = 0;
        if (sub < L) {
            const int c = A.col[e0 + sub];
            a = (unsigned)A.count[e0 + sub];
            d = (unsigned)A.depth[c];
            grp = A.grp[c];
        }
        int l_max = L;                                      // the longest row of the wave bounds the walk
        for (int off = 32; off >= lanes; off >>= 1) l_max = max(l_max, __shfl_xor(l_max, off));
        unsigned less = 0, eq = 0;
        for (int j = 0; j < l_max; ++j) {
            const unsigned aj = __shfl(a, first + j), dj = __shfl(d, first + j);
            const u64 x = (u64)aj * d, y = (u64)a * dj;     // a_j / d_j < a / d  <=>  a_j * d < a * d_j
            const bool on = j < L;
            less += on && x < y;
            eq += on && x == y;
        }
        __syncthreads();                                    // the counters are clear
        u64 tp = 0;
        if (sub < L) {
            atomicAdd(&det[grp], 1u);
            atomicAdd(&tot[grp], (u64)a);
            atomicAdd(&rank[grp], (u64)(2 * z0 + 2 * (long long)less + eq + 1));
            tp = (u64)eq * eq - 1;
        }
        for (int off = lanes >> 1; off >= 1; off >>= 1) tp += __shfl_xor(tp, off);
        __syncthreads();                                    // the counters are complete
        if (have) {
            mk_flush_row(A, p, z0, tot, rank, det, sub, lanes);
            if (sub == 0) A.ties[p] = (long long)(mk_cube_minus(z0) + tp);
        }
        __syncthreads();                                    // read before the next rows clear them
    }
}

// ---- block arm: a workgroup per row ----
// a_x / d_x > a_y / d_y, exactly
__device__ static inline bool mk_above(uint2 x, uint2 y) { return (u64)x.x * y.y > (u64)y.x * x.y; }
// past a row's or a chunk's end: above every value (a < 2^31, d >= 1)
__device__ static inline uint2 mk_sentinel() { return make_uint2(0xFFFFFFFFu, 1u); }

// dynamic LDS: the counters of one row, u64 ties, then uint2 (count, depth)[cap] and unsigned char group[cap]; cap a power of two
__host__ __device__ static inline size_t mk_block_lds(int cap, int G) {
    return mk_counter_bytes(1, G) + 16 + ((size_t)cap * 9 + 15) / 16 * 16;
}

// The row is sorted in LDS (bitonic, by the exact comparison, the groups moving with their values); then every entry finds the run of
// values equal to its own by two binary searches: less = the run's start, eq = its length.
__global__ void __launch_bounds__(MK_WG_BLOCK) mk_block(MkArgs A, const int *__restrict__ rows, int n_rows, int cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mk_lds[];
    u64 *s_tot = (u64 *)mk_lds, *s_rank = s_tot + A.G;
    unsigned *s_det = (unsigned *)(s_rank + A.G);
    u64 *s_ties = (u64 *)(mk_lds + mk_counter_bytes(1, A.G));
    uint2 *s_v = (uint2 *)(s_ties + 2);
    unsigned char *s_g = (unsigned char *)(s_v + cap);
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {                            // workgroup-uniform
        const int p = rows[r];
        const long long e0 = A.row_ptr[p];
        const int L = min((int)(A.row_ptr[p + 1] - e0), cap);                          // the entry point lists no longer row
        const long long z0 = A.N - L;
        int n_sort = MK_MIN_CHUNK;                                                     // a power of two, at most cap
        while (n_sort < L) n_sort *= 2;
        for (int g = tid; g < A.G; g += MK_WG_BLOCK) { s_tot[g] = 0; s_rank[g] = 0; s_det[g] = 0; }
        if (tid == 0) s_ties[0] = 0;
        for (int i = tid; i < n_sort; i += MK_WG_BLOCK) {
            const int c = i < L ? A.col[e0 + i] : 0;
            s_v[i] = i < L ? make_uint2((unsigned)A.count[e0 + i], (unsigned)A.depth[c]) : mk_sentinel();
            s_g[i] = i < L ? A.grp[c] : (unsigned char)0;
        }
        __syncthreads();
        for (int k = 2; k <= n_sort; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < n_sort / 2; t += MK_WG_BLOCK) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                    const uint2 x = s_v[lo], y = s_v[hi];
                    if ((lo & k) == 0 ? mk_above(x, y) : mk_above(y, x)) {
                        const unsigned char gx = s_g[lo];
                        s_v[lo] = y; s_v[hi] = x;
                        s_g[lo] = s_g[hi]; s_g[hi] = gx;
                    }
                }
                __syncthreads();
            }
        u64 tp = 0;
        for (int i = tid; i < L; i += MK_WG_BLOCK) {
            const uint2 v = s_v[i];
            int lo = 0, hi = i;                             // the first entry not below v: at most i
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (mk_above(v, s_v[mid])) lo = mid + 1; else hi = mid;
            }
            const int less = lo;
            lo = i + 1; hi = L;                             // the first entry above v: past i
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (mk_above(s_v[mid], v)) hi = mid; else lo = mid + 1;
            }
            const unsigned eq = (unsigned)(lo - less), grp = s_g[i];
            atomicAdd(&s_det[grp], 1u);
            atomicAdd(&s_tot[grp], (u64)v.x);
            atomicAdd(&s_rank[grp], (u64)(2 * z0 + 2 * (long long)less + eq + 1));
            tp += (u64)eq * eq - 1;
        }
        for (int off = 32; off >= 1; off >>= 1) tp += __shfl_xor(tp, off);
        if ((tid & 63) == 0 && tp) atomicAdd(s_ties, tp);
        __syncthreads();                                    // the counters are complete
        mk_flush_row(A, p, z0, s_tot, s_rank, s_det, tid, MK_WG_BLOCK);
        if (tid == 0) A.ties[p] = (long long)(mk_cube_minus(z0) + s_ties[0]);
        __syncthreads();                                    // read before the next row clears them
    }
}

// ---- long arm ----
// chunks[k] = (row, index of the chunk within the row): chunk c of row p holds the row's entries [c * chunk, min((c + 1) * chunk, L))
// sorts one chunk ascending into sorted[] (at the entries' own offsets) and, as a row's chunk 0, starts the row's outputs
__global__ void __launch_bounds__(MK_WG_LONG) mk_long_sort(MkArgs A, const int2 *__restrict__ chunks, int chunk, uint2 *__restrict__ sorted) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mk_lds[];
    uint2 *s_v = (uint2 *)mk_lds;
    const int tid = threadIdx.x;
    const int p = chunks[blockIdx.x].x, c = chunks[blockIdx.x].y;
    const long long e0 = A.row_ptr[p], L = A.row_ptr[p + 1] - e0;
    const long long b0 = e0 + (long long)c * chunk;
    const int len = (int)min((long long)chunk, L - (long long)c * chunk);
    if (c == 0) {
        const long long z0 = A.N - L;
        for (int g = tid; g < A.G; g += MK_WG_LONG) {
            const size_t o = (size_t)p * A.G + g;
            A.detected[o] = 0;
            A.total[o] = 0;
            A.rank2[o] = (long long)((u64)A.n_in_group[g] * (u64)(z0 + 1));
        }
        if (tid == 0) A.ties[p] = (long long)mk_cube_minus(z0);
    }
    int n_sort = MK_MIN_CHUNK;                              // a power of two, at most `chunk`
    while (n_sort < len) n_sort *= 2;
    for (int i = tid; i < n_sort; i += MK_WG_LONG)
        s_v[i] = i < len ? make_uint2((unsigned)A.count[b0 + i], (unsigned)A.depth[A.col[b0 + i]]) : mk_sentinel();
    __syncthreads();
    for (int k = 2; k <= n_sort; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < n_sort / 2; t += MK_WG_LONG) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint2 x = s_v[lo], y = s_v[hi];
                const bool up = (lo & k) == 0;
                if (up ? mk_above(x, y) : mk_above(y, x)) { s_v[lo] = y; s_v[hi] = x; }
            }
            __syncthreads();
        }
    for (int i = tid; i < len; i += MK_WG_LONG) sorted[b0 + i] = s_v[i];
}

// every entry of one chunk against every sorted chunk of its row
__global__ void __launch_bounds__(MK_WG_LONG) mk_long_rank(MkArgs A, const int2 *__restrict__ chunks, int chunk, const uint2 *__restrict__ sorted) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mk_lds[];
    u64 *s_tot = (u64 *)mk_lds, *s_rank = s_tot + A.G;
    unsigned *s_det = (unsigned *)(s_rank + A.G);
    u64 *s_ties = (u64 *)(mk_lds + mk_counter_bytes(1, A.G));
    const int tid = threadIdx.x;
    const int p = chunks[blockIdx.x].x, c = chunks[blockIdx.x].y;
    const long long e0 = A.row_ptr[p], L = A.row_ptr[p + 1] - e0, z0 = A.N - L;
    const long long b0 = e0 + (long long)c * chunk;
    const int len = (int)min((long long)chunk, L - (long long)c * chunk);
    const int n_chunks = (int)((L + chunk - 1) / chunk);
    for (int g = tid; g < A.G; g += MK_WG_LONG) { s_tot[g] = 0; s_rank[g] = 0; s_det[g] = 0; }
    if (tid == 0) s_ties[0] = 0;
    __syncthreads();
    u64 tp = 0;
    for (int i = tid; i < len; i += MK_WG_LONG) {
        const int cell = A.col[b0 + i];
        const uint2 v = make_uint2((unsigned)A.count[b0 + i], (unsigned)A.depth[cell]);
        long long less = 0, eq = 0;
        for (int k = 0; k < n_chunks; ++k) {
            const uint2 *s = sorted + e0 + (long long)k * chunk;
            const int n = (int)min((long long)chunk, L - (long long)k * chunk);
            int lo = 0, hi = n;                             // the first element not below v
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (mk_above(v, s[mid])) lo = mid + 1; else hi = mid;
            }
            const int lb = lo;
            hi = n;                                         // the first element above v
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (mk_above(s[mid], v)) hi = mid; else lo = mid + 1;
            }
            less += lb;
            eq += lo - lb;
        }
        const unsigned grp = A.grp[cell];
        atomicAdd(&s_det[grp], 1u);
        atomicAdd(&s_tot[grp], (u64)v.x);
        atomicAdd(&s_rank[grp], (u64)(2 * z0 + 2 * less + eq + 1) - (u64)(z0 + 1));     // the cell leaves the row's zeros
        tp += (u64)eq * (u64)eq - 1;
    }
    for (int off = 32; off >= 1; off >>= 1) tp += __shfl_xor(tp, off);
    if ((tid & 63) == 0 && tp) atomicAdd(s_ties, tp);
    __syncthreads();
    for (int g = tid; g < A.G; g += MK_WG_LONG) {
        if (!s_det[g]) continue;
        const size_t o = (size_t)p * A.G + g;
        atomicAdd(&A.detected[o], (int)s_det[g]);
        atomicAdd((u64 *)&A.total[o], s_tot[g]);
        atomicAdd((u64 *)&A.rank2[o], s_rank[g]);
    }
    if (tid == 0 && s_ties[0]) atomicAdd((u64 *)&A.ties[p], s_ties[0]);
}

// how a call launches: what natac_group_rank_sums runs and natac_group_rank_sums_plan reports
struct MkPlan {
    int short_max, block_max;      // a row of L entries: short when L <= short_max, else block when L <= block_max, else long
    int lanes;                     // the lanes of a row of the short arm: 16, 32 or 64, the least that holds min(short_max, longest row)
    int chunk;                     // the long arm's chunk: the largest power of two up to block_max, in [MK_MIN_CHUNK, MK_LONG_CHUNK]
    int block_cap;                 // entries of LDS the block arm is launched with: the power of two at or above min(longest row, block_max),
                                   // 0 when no row can take it
    int wg[3];                     // threads of a workgroup: short, block, long
    long long lds[3];              // dynamic LDS of a workgroup, bytes (long: the larger of its two kernels); 0 when no row can take the arm
    int grid_short, grid_block;    // the most workgroups the two grid-stride kernels are launched with
};

static int mk_env(const char *name, long long lo, long long hi, int dflt) {
    if (const char *e = getenv(name)) {
        const long long v = atoll(e);
        if (v >= lo && v <= hi) return (int)v;
    }
    return dflt;
}

static size_t mk_long_lds(int chunk, int G) { return std::max<size_t>((size_t)chunk * sizeof(uint2), mk_counter_bytes(1, G) + 16); }

// for n_groups groups, the longest row of `longest` entries (>= 0) and n_cu compute units
static void mk_plan(long long longest, int G, int n_cu, MkPlan *p) {
    p->short_max = mk_env("NATAC_MARKERS_SHORT_MAX", 1, MK_SHORT_MAX, MK_SHORT_MAX);
    p->block_max = std::max(p->short_max, mk_env("NATAC_MARKERS_BLOCK_MAX", 1, MK_BLOCK_MAX, MK_BLOCK_MAX));
    const long long widest = std::max<long long>(1, std::min<long long>(p->short_max, longest));
    p->lanes = widest <= 16 ? 16 : widest <= 32 ? 32 : 64;
    p->chunk = MK_MIN_CHUNK;
    while (p->chunk * 2 <= std::min(p->block_max, MK_LONG_CHUNK)) p->chunk *= 2;
    p->block_cap = 0;
    if (longest > p->short_max && p->block_max > p->short_max)
        for (p->block_cap = MK_MIN_CHUNK; p->block_cap < std::min<long long>(longest, p->block_max);) p->block_cap *= 2;
    p->wg[0] = MK_WG_SHORT; p->wg[1] = MK_WG_BLOCK; p->wg[2] = MK_WG_LONG;
    p->lds[0] = (long long)mk_counter_bytes(MK_WG_SHORT / p->lanes, G);
    p->lds[1] = p->block_cap ? (long long)mk_block_lds(p->block_cap, G) : 0;
    p->lds[2] = longest > p->block_max ? (long long)mk_long_lds(p->chunk, G) : 0;
    p->grid_short = 8 * n_cu;
    p->grid_block = 8 * n_cu;
}

}  // namespace natac_mk

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_group_rank_sums(natac_ctx *c, int64_t m, int64_t n, const int64_t *row_ptr, const int32_t *col, const int32_t *count,
                          const int64_t *depth, const int32_t *group, int32_t n_groups, int32_t *detected, int64_t *total, int64_t *rank2,
                          int64_t *ties, int64_t *arm_rows, double *kernel_ms) {
    using namespace natac_mk;
    static_assert(MK_MAX_OUT == NATAC_MARKERS_MAX_OUT && MK_MAX_N == NATAC_MARKERS_MAX_CELLS && MK_MAX_G == NATAC_MARKERS_MAX_GROUPS &&
                      MK_SHORT_MAX == NATAC_MARKERS_SHORT_CAP && MK_BLOCK_MAX == NATAC_MARKERS_BLOCK_CAP,
                  "the limits are in natac.h");
    if (!c || !row_ptr || !depth || !group) return fail(NATAC_E_ARG, "null argument");
    if (n < 2 || n > MK_MAX_N) return fail(NATAC_E_ARG, "n must be in [2, %lld] (got %lld)", MK_MAX_N, (long long)n);
    if (n_groups < 1 || n_groups > MK_MAX_G) return fail(NATAC_E_ARG, "n_groups must be in [1, %d] (got %d)", MK_MAX_G, n_groups);
    if (m < 0 || m > MK_MAX_OUT || m * (int64_t)n_groups > MK_MAX_OUT)
        return fail(NATAC_E_ARG, "m must be at least 0 and m x n_groups at most %lld (got %lld x %d)", MK_MAX_OUT, (long long)m, n_groups);
    if (m > 0 && (!detected || !total || !rank2 || !ties)) return fail(NATAC_E_ARG, "null argument");
    const int G = n_groups;
    std::vector<int> h_depth((size_t)n), n_in_group((size_t)G, 0);
    std::vector<unsigned char> h_grp((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (depth[i] < 1 || depth[i] >= (1LL << 31)) return fail(NATAC_E_ARG, "depth[%lld] = %lld outside [1, 2^31)", (long long)i, (long long)depth[i]);
        if (group[i] < 0 || group[i] >= G) return fail(NATAC_E_ARG, "group[%lld] = %d outside [0, %d)", (long long)i, group[i], G);
        h_depth[(size_t)i] = (int)depth[i];
        h_grp[(size_t)i] = (unsigned char)group[i];
        n_in_group[(size_t)group[i]] += 1;
    }
    if (row_ptr[0] < 0) return fail(NATAC_E_ARG, "row_ptr[0] is negative");
    long long longest = 0;
    for (int64_t i = 0; i < m; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) return fail(NATAC_E_ARG, "row_ptr is not monotone (row %lld)", (long long)i);
        longest = std::max<long long>(longest, row_ptr[i + 1] - row_ptr[i]);
    }
    const int64_t e0 = row_ptr[0], nnz = row_ptr[m] - e0;
    if (nnz > 0 && (!col || !count)) return fail(NATAC_E_ARG, "null argument");
    for (int64_t i = 0; i < m; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) return fail(NATAC_E_ARG, "row %lld: column %d outside [0, %lld)", (long long)i, col[e], (long long)n);
            if (e > row_ptr[i] && col[e] <= col[e - 1]) return fail(NATAC_E_ARG, "row %lld: columns must be strictly ascending", (long long)i);
            if (count[e] < 1) return fail(NATAC_E_ARG, "row %lld: count %d is below 1", (long long)i, count[e]);
        }
    if (kernel_ms) *kernel_ms = 0;
    if (arm_rows) arm_rows[0] = arm_rows[1] = arm_rows[2] = 0;
    if (m == 0) return NATAC_OK;

    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);     // 256 stands if the query fails
    MkPlan plan;
    mk_plan(longest, G, n_cu, &plan);
    // the rows of every arm, and the long rows' chunks
    std::vector<int> rows[3];
    std::vector<int2> chunks;
    std::vector<long long> ptr((size_t)m + 1);
    for (int64_t i = 0; i <= m; ++i) ptr[(size_t)i] = row_ptr[i] - e0;
    for (int64_t i = 0; i < m; ++i) {
        const long long L = row_ptr[i + 1] - row_ptr[i];
        const int arm = L <= plan.short_max ? 0 : L <= plan.block_max ? 1 : 2;
        rows[arm].push_back((int)i);
        if (arm == 2) {
            const long long nc = (L + plan.chunk - 1) / plan.chunk;
            if ((long long)chunks.size() + nc > 2147483647LL) return fail(NATAC_E_ARG, "row %lld: too many chunks of %d entries for one call", (long long)i, plan.chunk);
            for (long long k = 0; k < nc; ++k) chunks.push_back(make_int2((int)i, (int)k));
        }
    }
    DeviceCall dc(c, "group_rank_sums");
    MkArgs A;
    A.row_ptr = dc.upload(ptr.data(), ptr.size());
    A.col = dc.upload(nnz ? (const int *)(col + e0) : nullptr, (size_t)nnz);
    A.count = dc.upload(nnz ? (const int *)(count + e0) : nullptr, (size_t)nnz);
    A.depth = dc.upload(h_depth.data(), h_depth.size());
    A.grp = dc.upload(h_grp.data(), h_grp.size());
    A.n_in_group = dc.upload(n_in_group.data(), n_in_group.size());
    A.N = (int)n;
    A.G = G;
    const size_t n_out = (size_t)m * G;
    A.detected = dc.alloc<int>(n_out);
    A.total = dc.alloc<long long>(n_out);
    A.rank2 = dc.alloc<long long>(n_out);
    A.ties = dc.alloc<long long>((size_t)m);
    const int *d_rows[3] = {nullptr, nullptr, nullptr};
    for (int a = 0; a < 3; ++a)
        if (!rows[a].empty()) d_rows[a] = dc.upload(rows[a].data(), rows[a].size());
    const int2 *d_chunks = chunks.empty() ? nullptr : dc.upload(chunks.data(), chunks.size());
    uint2 *d_sorted = chunks.empty() ? nullptr : dc.alloc<uint2>((size_t)nnz);
    dc.time_begin(kernel_ms);
    if (dc.ok() && !rows[0].empty()) {
        const int slots = MK_WG_SHORT / plan.lanes;
        const unsigned bx = (unsigned)std::min<long long>(((long long)rows[0].size() + slots - 1) / slots, plan.grid_short);
        if (plan.lds[0] > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)mk_short, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds[0]));
        hipLaunchKernelGGL(mk_short, dim3(bx), dim3(MK_WG_SHORT), (size_t)plan.lds[0], c->stream, A, d_rows[0], (int)rows[0].size(), plan.lanes);
        dc.launched();
    }
    if (dc.ok() && !rows[1].empty()) {
        const unsigned bx = (unsigned)std::min<long long>((long long)rows[1].size(), plan.grid_block);
        if (plan.lds[1] > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)mk_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds[1]));
        hipLaunchKernelGGL(mk_block, dim3(bx), dim3(MK_WG_BLOCK), (size_t)plan.lds[1], c->stream, A, d_rows[1], (int)rows[1].size(), plan.block_cap);
        dc.launched();
    }
    if (dc.ok() && !chunks.empty()) {
        hipLaunchKernelGGL(mk_long_sort, dim3((unsigned)chunks.size()), dim3(MK_WG_LONG), (size_t)plan.chunk * sizeof(uint2), c->stream, A, d_chunks,
                           plan.chunk, d_sorted);
        hipLaunchKernelGGL(mk_long_rank, dim3((unsigned)chunks.size()), dim3(MK_WG_LONG), mk_counter_bytes(1, G) + 16, c->stream, A, d_chunks,
                           plan.chunk, (const uint2 *)d_sorted);
        dc.launched();
    }
    dc.time_end();
    // into temporaries first: a failed call leaves the caller's arrays as they were
    std::vector<int> h_det(n_out);
    std::vector<long long> h_tot(n_out), h_rank(n_out), h_ties((size_t)m);
    dc.fetch(h_det.data(), A.detected, n_out);
    dc.fetch(h_tot.data(), A.total, n_out);
    dc.fetch(h_rank.data(), A.rank2, n_out);
    dc.fetch(h_ties.data(), A.ties, (size_t)m);
    if (const int rc = dc.finish()) return rc;
    std::copy(h_det.begin(), h_det.end(), detected);
    std::copy(h_tot.begin(), h_tot.end(), (long long *)total);
    std::copy(h_rank.begin(), h_rank.end(), (long long *)rank2);
    std::copy(h_ties.begin(), h_ties.end(), (long long *)ties);
    if (arm_rows)
        for (int a = 0; a < 3; ++a) arm_rows[a] = (int64_t)rows[a].size();
    return NATAC_OK;
}

int natac_group_rank_sums_plan(int64_t m, int64_t n, int64_t nnz, int64_t longest_row, int32_t n_groups, int32_t n_cu, int32_t *short_max,
                               int32_t *block_max, int32_t *lanes, int32_t *chunk, int32_t *wg, int64_t *lds_bytes, int32_t *grid) {
    using namespace natac_mk;
    if (!short_max || !block_max || !lanes || !chunk || !wg || !lds_bytes || !grid) return fail(NATAC_E_ARG, "null argument");
    if (m < 1 || m > MK_MAX_OUT || n < 2 || n > MK_MAX_N || nnz < 0 || longest_row < 0 || longest_row > n || longest_row > nnz || nnz > m * n ||
        n_groups < 1 || n_groups > MK_MAX_G || n_cu < 1 || m * (int64_t)n_groups > MK_MAX_OUT)
        return fail(NATAC_E_ARG, "natac_group_rank_sums_plan: m >= 1, n in [2, %lld], longest_row <= min(n, nnz) <= m x n, n_groups in [1, %d], "
                                 "m x n_groups <= %lld, n_cu >= 1", MK_MAX_N, MK_MAX_G, MK_MAX_OUT);
    MkPlan p;
    mk_plan(longest_row, n_groups, n_cu, &p);
    *short_max = p.short_max;
    *block_max = p.block_max;
    *lanes = p.lanes;
    *chunk = p.chunk;
    for (int a = 0; a < 3; ++a) { wg[a] = p.wg[a]; lds_bytes[a] = p.lds[a]; }
    grid[0] = (int32_t)std::min<long long>((m + MK_WG_SHORT / p.lanes - 1) / (MK_WG_SHORT / p.lanes), p.grid_short);
    grid[1] = (int32_t)std::min<long long>(m, p.grid_block);
    return NATAC_OK;
}

}  // extern "C"
