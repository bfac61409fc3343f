// natac_coaccess.hpp -- the kernels behind `pyatac coaccess` (this package's own command: the reference has no such tool): for every pair of
// listed windows the exact integers a Pearson correlation over the cells needs (natac_window_pair_sums, include/natac.h states the rule),
// and the host-only launch plan (natac_window_pair_sums_plan).
//
// The counts arrive as natac_region_cell_counts leaves them: CSR with one row per window (m of them), the cells (n) ascending within a
// row, every count >= 1.  order[k] lists rows in rank sequence; owner i is paired with the partners order[i + 1 .. hi[i]), and its pairs
// start at pair_ptr[i].  Per pair (p, q):  sxy = the sum over the cells both rows hold of a[p, c] * a[q, c],  both = the number of such
// cells.
//
// A workgroup of 256 threads owns one window at a time (grid stride over the owners) and keeps the owner's row in LDS; every partner row
// goes to a lane group of `lanes` threads (16 / 32 / 64, the least that holds the mean length of the listed rows), a lane takes the
// partner's entries with stride `lanes`, looks the cell up in the owner's row and accumulates count * owner_count (u32 x u32 + u64) and
// the matches; the group reduces across lanes by cross-lane reads and one lane stores the pair.  Two kernels, one per call (ca_plan):
//   ca_table   n <= table_max: the LDS holds a dense table of the owner's counts over all cells, zeroed once per workgroup; per owner the
//              row is scattered into it, the partners read one word per entry, and zeros go back at the owner's columns only.
//   ca_search  any n: the owner's (cell, count) pairs sit in LDS, at most `chunk` at a time, and every partner entry does a binary search
//              among them.  A longer owner is walked chunk by chunk: the first chunk stores the pair's outputs, the later ones add to them
//              with plain loads and stores -- the same lane of the same workgroup every time, so there is nothing to order.
// No atomics, no floating point: the outputs are a pure function of the operands under every threshold and chunk.
// Behind the kernels: the entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "natac_runtime.hpp"

namespace natac_ca {

typedef unsigned long long u64;

constexpr int CA_TABLE_MAX = 16384;         // NATAC_COACCESS_TABLE_CAP: 64 KiB of int32
constexpr int CA_CHUNK = 8192;              // NATAC_COACCESS_CHUNK_CAP: 64 KiB at 8 bytes an entry
constexpr int CA_MIN_CHUNK = 16;
constexpr int CA_WG = 256;
constexpr long long CA_MAX_PAIRS = 1LL << 25;   // NATAC_COACCESS_MAX_PAIRS
constexpr long long CA_MAX_N = 1LL << 20;       // NATAC_COACCESS_MAX_CELLS

struct CaArgs {
    const long long *row_ptr;      // [m + 1], counted from the call's first entry
    const int *col, *count;        // [nnz]
    const int *order;              // [k]
    const long long *hi, *pair_ptr;    // [k], [k + 1]
    long long k;
    long long *sxy;                // [pairs]
    int *both;                     // [pairs]
};

// the sum of a lane group's values, in every lane of it
__device__ static inline void ca_reduce(u64 &s, unsigned &b, int lanes) {
    for (int off = lanes >> 1; off >= 1; off >>= 1) {
        s += __shfl_xor(s, off);
        b += __shfl_xor(b, off);
    }
}

// ---- table arm ----
__global__ void __launch_bounds__(CA_WG) ca_table(CaArgs A, int lanes, int n_words) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ca_lds[];
    unsigned *s_tab = (unsigned *)ca_lds;               // [n_words >= n]: the owner's count of every cell, 0 where it has none
    const int tid = threadIdx.x, groups = CA_WG / lanes, grp = tid / lanes, sub = tid & (lanes - 1);
    for (int i = tid; i < n_words; i += CA_WG) s_tab[i] = 0;
    __syncthreads();
    for (long long i = blockIdx.x; i < A.k; i += gridDim.x) {                          // workgroup-uniform
        const long long partners = A.hi[i] - i - 1;
        if (partners <= 0) continue;
        const long long e0 = A.row_ptr[A.order[i]], out0 = A.pair_ptr[i];
        const int L = (int)(A.row_ptr[A.order[i] + 1] - e0);
        for (int e = tid; e < L; e += CA_WG) s_tab[A.col[e0 + e]] = (unsigned)A.count[e0 + e];
        __syncthreads();
        for (long long j0 = 0; j0 < partners; j0 += groups) {                          // workgroup-uniform: every lane reaches the reduction
            const long long j = j0 + grp;
            const bool have = j < partners;
            const int q = have ? A.order[i + 1 + j] : 0;
            const long long f0 = have ? A.row_ptr[q] : 0;
            const int Lq = have ? (int)(A.row_ptr[q + 1] - f0) : 0;
            u64 s = 0;
            unsigned b = 0;
            for (int e = sub; e < Lq; e += lanes) {
                const unsigned v = s_tab[A.col[f0 + e]];
                s += (u64)(unsigned)A.count[f0 + e] * v;
                b += v != 0;
            }
            ca_reduce(s, b, lanes);
            if (have && sub == 0) {
                A.sxy[out0 + j] = (long long)s;
                A.both[out0 + j] = (int)b;
            }
        }
        __syncthreads();                                    // read before the owner's columns are cleared
        for (int e = tid; e < L; e += CA_WG) s_tab[A.col[e0 + e]] = 0;
        __syncthreads();                                    // clear before the next owner scatters
    }
}

// ---- search arm ----
__global__ void __launch_bounds__(CA_WG) ca_search(CaArgs A, int lanes, int chunk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ca_lds[];
    uint2 *s_own = (uint2 *)ca_lds;                     // [chunk]: (cell, count) of the owner's entries, the cells ascending
    const int tid = threadIdx.x, groups = CA_WG / lanes, grp = tid / lanes, sub = tid & (lanes - 1);
    for (long long i = blockIdx.x; i < A.k; i += gridDim.x) {                          // workgroup-uniform
        const long long partners = A.hi[i] - i - 1;
        if (partners <= 0) continue;
        const long long e0 = A.row_ptr[A.order[i]], out0 = A.pair_ptr[i];
        const long long L = A.row_ptr[A.order[i] + 1] - e0;
        long long c0 = 0;
        do {                                                // an empty owner still stores its zeros
            const int len = (int)min((long long)chunk, L - c0);
            for (int e = tid; e < len; e += CA_WG) s_own[e] = make_uint2((unsigned)A.col[e0 + c0 + e], (unsigned)A.count[e0 + c0 + e]);
            __syncthreads();
            for (long long j0 = 0; j0 < partners; j0 += groups) {                      // workgroup-uniform
                const long long j = j0 + grp;
                const bool have = j < partners;
                const int q = have ? A.order[i + 1 + j] : 0;
                const long long f0 = have ? A.row_ptr[q] : 0;
                const int Lq = have ? (int)(A.row_ptr[q + 1] - f0) : 0;
                u64 s = 0;
                unsigned b = 0;
                for (int e = sub; e < Lq; e += lanes) {
                    const unsigned c = (unsigned)A.col[f0 + e];
                    int lo = 0, up = len;                   // the first of the chunk's cells not below c
                    while (lo < up) {
                        const int mid = (lo + up) >> 1;
                        if (s_own[mid].x < c) lo = mid + 1; else up = mid;
                    }
                    const uint2 hit = s_own[min(lo, max(len - 1, 0))];
                    const bool found = lo < len && hit.x == c;
                    s += found ? (u64)(unsigned)A.count[f0 + e] * hit.y : 0;
                    b += found;
                }
                ca_reduce(s, b, lanes);
                if (have && sub == 0) {
                    if (c0 == 0) {
                        A.sxy[out0 + j] = (long long)s;
                        A.both[out0 + j] = (int)b;
                    } else if (b) {                         // this lane stored them under the first chunk
                        A.sxy[out0 + j] += (long long)s;
                        A.both[out0 + j] += (int)b;
                    }
                }
            }
            __syncthreads();                                // read before the next chunk or owner overwrites it
            c0 += chunk;
        } while (c0 < L);
    }
}

// how a call launches: what natac_window_pair_sums runs and natac_window_pair_sums_plan reports
struct CaPlan {
    int table_max, arm;            // arm 0 = table (n <= table_max), 1 = search
    int lanes;                     // of a partner row: 16, 32 or 64, the least that holds ceil(listed entries / k)
    int chunk;                     // the owner's entries the search arm holds at once: a power of two
    int wg;                        // threads of a workgroup
    long long lds;                 // dynamic LDS of a workgroup, bytes: 4 n rounded up to 16 (table), 8 chunk (search)
    int grid;                      // the most workgroups the kernel is launched with
};

static int ca_env(const char *name, long long lo, long long hi, int dflt) {
    if (const char *e = getenv(name)) {
        const long long v = atoll(e);
        if (v >= lo && v <= hi) return (int)v;
    }
    return dflt;
}

// for n cells, k listed windows with listed_entries entries between them (counted with multiplicity) and n_cu compute units
static void ca_plan(long long n, long long k, long long listed_entries, int n_cu, CaPlan *p) {
    p->table_max = ca_env("NATAC_COACCESS_TABLE_MAX", 1, CA_TABLE_MAX, CA_TABLE_MAX);
    p->chunk = ca_env("NATAC_COACCESS_CHUNK", CA_MIN_CHUNK, CA_CHUNK, CA_CHUNK);
    if (p->chunk & (p->chunk - 1)) p->chunk = CA_CHUNK;     // not a power of two: not taken
    p->arm = n <= p->table_max ? 0 : 1;
    const long long mean = k > 0 ? (listed_entries + k - 1) / k : 0;
    p->lanes = mean <= 16 ? 16 : mean <= 32 ? 32 : 64;
    p->wg = CA_WG;
    p->lds = p->arm == 0 ? (n * 4 + 15) / 16 * 16 : (long long)p->chunk * (long long)sizeof(uint2);
    p->grid = 8 * n_cu;
}

}  // namespace natac_ca

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_window_pair_sums(natac_ctx *c, int64_t m, int64_t n, const int64_t *row_ptr, const int32_t *col, const int32_t *count, int64_t k,
                           const int32_t *order, const int64_t *hi, const int64_t *pair_ptr, int64_t *sxy, int32_t *both, int64_t *arm_owners,
                           double *kernel_ms) {
    using namespace natac_ca;
    static_assert(CA_MAX_PAIRS == NATAC_COACCESS_MAX_PAIRS && CA_MAX_N == NATAC_COACCESS_MAX_CELLS && CA_TABLE_MAX == NATAC_COACCESS_TABLE_CAP &&
                      CA_CHUNK == NATAC_COACCESS_CHUNK_CAP,
                  "the limits are in natac.h");
    if (!c || !row_ptr || !pair_ptr) return fail(NATAC_E_ARG, "null argument");
    if (n < 1 || n > CA_MAX_N) return fail(NATAC_E_ARG, "n must be in [1, %lld] (got %lld)", CA_MAX_N, (long long)n);
    if (m < 0 || m > 2147483647LL) return fail(NATAC_E_ARG, "m must be in [0, 2^31) (got %lld)", (long long)m);
    if (k < 0 || k > 2147483647LL) return fail(NATAC_E_ARG, "k must be in [0, 2^31) (got %lld)", (long long)k);
    if (k > 0 && (!order || !hi)) return fail(NATAC_E_ARG, "null argument");
    if (row_ptr[0] < 0) return fail(NATAC_E_ARG, "row_ptr[0] is negative");
    for (int64_t i = 0; i < m; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return fail(NATAC_E_ARG, "row_ptr is not monotone (row %lld)", (long long)i);
    const int64_t e0 = row_ptr[0], nnz = row_ptr[m] - e0;
    if (nnz > 0 && (!col || !count)) return fail(NATAC_E_ARG, "null argument");
    long long a_max = 0;
    for (int64_t i = 0; i < m; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) return fail(NATAC_E_ARG, "row %lld: column %d outside [0, %lld)", (long long)i, col[e], (long long)n);
            if (e > row_ptr[i] && col[e] <= col[e - 1]) return fail(NATAC_E_ARG, "row %lld: columns must be strictly ascending", (long long)i);
            if (count[e] < 1) return fail(NATAC_E_ARG, "row %lld: count %d is below 1", (long long)i, count[e]);
            a_max = std::max<long long>(a_max, count[e]);
        }
    long long l_max = 0, listed = 0, with_partner = 0;
    if (pair_ptr[0] != 0) return fail(NATAC_E_ARG, "pair_ptr[0] must be 0 (got %lld)", (long long)pair_ptr[0]);
    for (int64_t i = 0; i < k; ++i) {
        if (order[i] < 0 || order[i] >= m) return fail(NATAC_E_ARG, "order[%lld] = %d outside [0, %lld)", (long long)i, order[i], (long long)m);
        if (hi[i] <= i || hi[i] > k) return fail(NATAC_E_ARG, "hi[%lld] = %lld outside (%lld, %lld]", (long long)i, (long long)hi[i], (long long)i, (long long)k);
        if (pair_ptr[i + 1] - pair_ptr[i] != hi[i] - i - 1)
            return fail(NATAC_E_ARG, "pair_ptr[%lld] - pair_ptr[%lld] = %lld, but owner %lld has %lld partners", (long long)i + 1, (long long)i,
                        (long long)(pair_ptr[i + 1] - pair_ptr[i]), (long long)i, (long long)(hi[i] - i - 1));
        if (pair_ptr[i + 1] > CA_MAX_PAIRS) return fail(NATAC_E_ARG, "more than %lld pairs (owner %lld)", CA_MAX_PAIRS, (long long)i);
        const long long L = row_ptr[order[i] + 1] - row_ptr[order[i]];
        l_max = std::max(l_max, L);
        listed += L;
        with_partner += hi[i] > i + 1;
    }
    if ((unsigned __int128)n * (unsigned __int128)a_max * (unsigned __int128)a_max * (unsigned __int128)l_max >= ((unsigned __int128)1 << 62))
        return fail(NATAC_E_ARG, "N * a_max^2 * L_max must be below 2^62: N = %lld cells, a_max = %lld the largest count, L_max = %lld the longest listed row",
                    (long long)n, a_max, l_max);
    const long long pairs = k > 0 ? pair_ptr[k] : 0;
    if (kernel_ms) *kernel_ms = 0;
    if (arm_owners) arm_owners[0] = arm_owners[1] = 0;
    if (pairs == 0) return NATAC_OK;
    if (!sxy || !both) return fail(NATAC_E_ARG, "null argument");

    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);     // 256 stands if the query fails
    CaPlan plan;
    ca_plan(n, k, listed, n_cu, &plan);
    std::vector<long long> ptr((size_t)m + 1);
    for (int64_t i = 0; i <= m; ++i) ptr[(size_t)i] = row_ptr[i] - e0;
    DeviceCall dc(c, "window_pair_sums");
    CaArgs A;
    A.row_ptr = dc.upload(ptr.data(), ptr.size());
    A.col = dc.upload(nnz ? (const int *)(col + e0) : nullptr, (size_t)nnz);
    A.count = dc.upload(nnz ? (const int *)(count + e0) : nullptr, (size_t)nnz);
    A.order = dc.upload((const int *)order, (size_t)k);
    A.hi = dc.upload((const long long *)hi, (size_t)k);
    A.pair_ptr = dc.upload((const long long *)pair_ptr, (size_t)k + 1);
    A.k = k;
    A.sxy = dc.alloc<long long>((size_t)pairs);
    A.both = dc.alloc<int>((size_t)pairs);
    dc.time_begin(kernel_ms);
    if (dc.ok()) {
        const unsigned bx = (unsigned)std::min<long long>(k, plan.grid);
        if (plan.arm == 0) {
            if (plan.lds >= 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)ca_table, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
            hipLaunchKernelGGL(ca_table, dim3(bx), dim3(CA_WG), (size_t)plan.lds, c->stream, A, plan.lanes, (int)(plan.lds / 4));
        } else {
            if (plan.lds >= 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)ca_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
            hipLaunchKernelGGL(ca_search, dim3(bx), dim3(CA_WG), (size_t)plan.lds, c->stream, A, plan.lanes, plan.chunk);
        }
        dc.launched();
    }
    dc.time_end();
    // into temporaries first: a failed call leaves the caller's arrays as they were
    std::vector<long long> h_sxy((size_t)pairs);
    std::vector<int> h_both((size_t)pairs);
    dc.fetch(h_sxy.data(), A.sxy, (size_t)pairs);
    dc.fetch(h_both.data(), A.both, (size_t)pairs);
    if (const int rc = dc.finish()) return rc;
    std::copy(h_sxy.begin(), h_sxy.end(), (long long *)sxy);
    std::copy(h_both.begin(), h_both.end(), both);
    if (arm_owners) arm_owners[plan.arm] = with_partner;
    return NATAC_OK;
}

int natac_window_pair_sums_plan(int64_t m, int64_t n, int64_t nnz, int64_t k, int64_t listed_entries, int32_t n_cu, int32_t *arm,
                                int32_t *table_max, int32_t *lanes, int32_t *chunk, int32_t *wg, int64_t *lds_bytes, int32_t *grid) {
    using namespace natac_ca;
    if (!arm || !table_max || !lanes || !chunk || !wg || !lds_bytes || !grid) return fail(NATAC_E_ARG, "null argument");
    if (m < 1 || m > 2147483647LL || n < 1 || n > CA_MAX_N || nnz < 0 || nnz > m * n || k < 1 || k > 2147483647LL || listed_entries < 0 ||
        listed_entries > k * n || n_cu < 1)
        return fail(NATAC_E_ARG, "natac_window_pair_sums_plan: m and k in [1, 2^31), n in [1, %lld], nnz <= m x n, listed_entries <= k x n, n_cu >= 1",
                    CA_MAX_N);
    CaPlan p;
    ca_plan(n, k, listed_entries, n_cu, &p);
    *arm = p.arm;
    *table_max = p.table_max;
    *lanes = p.lanes;
    *chunk = p.chunk;
    *wg = p.wg;
    *lds_bytes = p.lds;
    *grid = (int32_t)std::min<long long>(k, p.grid);
    return NATAC_OK;
}

}  // extern "C"
