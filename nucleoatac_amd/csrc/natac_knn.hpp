// natac_knn.hpp -- exact k-nearest-neighbour search in at most 64 dimensions (natac_knn, include/natac.h states the rule), the device
// part of `pyatac doublets`, and the host-only launch plan (natac_knn_plan).
//
// d2(i, j) is the plain sum over the columns of (q[i, c] - x[j, c])^2, every operation rounded once and added in column order, and row i
// of the result holds the k smallest references by (d2, j).  Both are exact rules, so every order of evaluation below must give the same
// bytes: the kernel keeps, per query, the k best seen so far and a threshold tau = the k-th best, and nothing else decides.
//
// One kernel, kn_search<QW, WAVE>.  A workgroup of 4 waves owns a tile of 4 QW queries, QW per wave, and walks the references in tiles of
// ref_tile rows with a grid stride over the query tiles.  A reference tile is read from global memory as one contiguous block (coalesced)
// and stored transposed in LDS, s_x[c][ref_tile + 1]: a wave reading one reference per lane at a fixed column reads consecutive doubles,
// and the odd row length spreads the transposing stores over the banks.  A wave's query coordinates lie in LDS as s_q[c][QW] and are read
// by all lanes at one address (a broadcast).  Per 64 references a lane holds one reference and QW accumulators: one LDS read of x feeds
// 3 QW fp64 operations.
// Selection is per query and stays inside the query's wave: the lanes whose (d2, j) lies below tau are found by one ballot and appended
// to the query's buffer in LDS at their prefix count.  When the next 64 candidates might not fit, the buffer and the list are reduced to
// the k best and tau drops.  The key (bits of d2 as uint64, j) orders like (d2, j) since d2 >= +0.
//   WAVE arm (k <= wave_k_max, at most 64): the list is one entry per lane in registers, kept ascending.  The buffer holds 64 entries;
//            a reduction sorts it over the lanes (bitonic, shuffles), takes the lane-wise minimum with the reversed list and merges.
//   LDS arm  (larger k): list and buffer are one array of C = the power of two >= max(k + 64, 128) entries per query, the list in [0, k), the
//            buffer behind it; a reduction pads to the next power of two and sorts that many entries in LDS (bitonic, one wave).
// No scratch, no atomics of any kind: the same bytes from two calls and under every arm, query tile and reference tile.
// Behind the kernel: the plan and the entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace natac_knn_ns {

typedef unsigned long long u64;

constexpr int KN_WG = 256, KN_WAVES = 4;
constexpr int KN_MAX_QW = 8;                // queries per wave: 1, 2, 4 or 8
constexpr int KN_MIN_RT = 64, KN_MAX_RT = 256;
constexpr long long KN_LDS_CAP = NATAC_KNN_LDS_CAP;
constexpr long long KN_LDS_SHARE = 80 * 1024;       // what a workgroup takes by default: two a CU
constexpr u64 KN_PAD_D = ~0ULL;             // above the bits of every finite d2
constexpr int KN_PAD_J = 0x7fffffff;

struct KnArgs {
    const double *q, *x;           // [nq, dim], [nr, dim]
    long long nq, nr, self_offset;
    int dim, k;
    int rt;                        // reference tile
    int cap;                       // entries of a query's LDS array: 64 (WAVE) or C
    int *idx;                      // [nq, k]
    double *dist2;                 // [nq, k]
};

__device__ __forceinline__ bool kn_less(u64 d, int j, u64 e, int i) { return d < e || (d == e && j < i); }

// compare-exchange with the lane `mask` away: keep the smaller pair (keep_min) or the larger
__device__ __forceinline__ void kn_cx(u64 &d, int &j, int mask, bool keep_min) {
    const u64 od = __shfl_xor(d, mask);
    const int oj = __shfl_xor(j, mask);
    const bool take = keep_min ? kn_less(od, oj, d, j) : kn_less(d, j, od, oj);
    d = take ? od : d;
    j = take ? oj : j;
}

// ascending bitonic sort of one pair per lane
__device__ __forceinline__ void kn_sort64(u64 &d, int &j, int lane) {
    for (int size = 2; size <= 64; size <<= 1)
        for (int s = size >> 1; s > 0; s >>= 1) kn_cx(d, j, s, ((lane & size) == 0) == ((lane & s) == 0));
}

// (ld, lj) ascending over the lanes, (bd, bj) any order: (ld, lj) becomes the 64 smallest of both, ascending
__device__ __forceinline__ void kn_merge64(u64 &ld, int &lj, u64 bd, int bj, int lane) {
    kn_sort64(bd, bj, lane);
    const u64 rd = __shfl(bd, 63 - lane);
    const int rj = __shfl(bj, 63 - lane);
    if (kn_less(rd, rj, ld, lj)) { ld = rd; lj = rj; }
    for (int s = 32; s > 0; s >>= 1) kn_cx(ld, lj, s, (lane & s) == 0);
}

// ascending bitonic sort of the first n entries (a power of two, at least 2) of a query's LDS array by one wave
__device__ __forceinline__ void kn_sort_lds(volatile u64 *ed, volatile int *ej, int n, int lane) {
    for (int size = 2; size <= n; size <<= 1)
        for (int s = size >> 1; s > 0; s >>= 1) {
            for (int t = lane; t < (n >> 1); t += 64) {
                const int i = ((t & ~(s - 1)) << 1) | (t & (s - 1)), p = i + s;
                const u64 da = ed[i], db = ed[p];
                const int ja = ej[i], jb = ej[p];
                const bool up = (i & size) == 0;
                if (up ? kn_less(db, jb, da, ja) : kn_less(da, ja, db, jb)) {
                    ed[i] = db; ej[i] = jb;
                    ed[p] = da; ej[p] = ja;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
}

template <int QW, bool WAVE>
__global__ void __launch_bounds__(KN_WG) kn_search(KnArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kn_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int dim = A.dim, k = A.k, rt = A.rt, rtp = A.rt + 1, cap = A.cap;
    // the carve-up kn_lds_bytes counts
    double *s_x = (double *)kn_lds;                                         // [dim][rtp]
    double *s_q = s_x + (size_t)dim * rtp + (size_t)wv * dim * QW;          // this wave's [dim][QW]
    u64 *u_base = (u64 *)(s_x + (size_t)dim * rtp + (size_t)KN_WAVES * dim * QW);
    volatile u64 *s_tau_d = u_base + wv * QW;                               // [QW]
    volatile u64 *s_ent_d = u_base + KN_WAVES * QW + (size_t)wv * QW * cap;  // [QW][cap]
    int *i_base = (int *)(u_base + KN_WAVES * QW + (size_t)KN_WAVES * QW * cap);
    volatile int *s_ent_j = i_base + (size_t)wv * QW * cap;                 // [QW][cap]
    volatile int *s_tau_j = i_base + (size_t)KN_WAVES * QW * cap + wv * QW;  // [QW]

    const u64 below = (1ULL << lane) - 1ULL;
    const int buf0 = WAVE ? 0 : k;             // where a query's buffer starts in its array
    const int step_row = KN_WG / dim, step_c = KN_WG % dim;

    const long long n_qtiles = (A.nq + KN_WAVES * QW - 1) / (KN_WAVES * QW);
    for (long long qt = blockIdx.x; qt < n_qtiles; qt += gridDim.x) {          // workgroup-uniform
        const long long q0 = qt * (KN_WAVES * QW) + (long long)wv * QW;        // this wave's first query
        // the wave's queries: QW contiguous rows
        for (int e = lane; e < QW * dim; e += 64) {
            const int qi = e / dim, c = e - qi * dim;
            s_q[c * QW + qi] = q0 + qi < A.nq ? A.q[q0 * dim + e] : 0.0;
        }
        u64 ld[QW];
        int lj[QW], cnt[QW];
#pragma unroll
        for (int qi = 0; qi < QW; ++qi) {
            ld[qi] = KN_PAD_D;
            lj[qi] = KN_PAD_J;
            cnt[qi] = 0;
            if (!WAVE)
                for (int i = lane; i < k; i += 64) {
                    s_ent_d[qi * cap + i] = KN_PAD_D;
                    s_ent_j[qi * cap + i] = KN_PAD_J;
                }
            if (lane == 0) {
                s_tau_d[qi] = KN_PAD_D;
                s_tau_j[qi] = KN_PAD_J;
            }
        }
        __builtin_amdgcn_wave_barrier();

        // list and buffer of query qi -> the k best, tau = the k-th
        auto reduce = [&](int qi) {
            volatile u64 *ed = s_ent_d + qi * cap;
            volatile int *ej = s_ent_j + qi * cap;
            __builtin_amdgcn_wave_barrier();
            u64 td;
            int tj;
            if (WAVE) {
                const u64 bd = lane < cnt[qi] ? ed[lane] : KN_PAD_D;
                const int bj = lane < cnt[qi] ? ej[lane] : KN_PAD_J;
                __builtin_amdgcn_wave_barrier();
                kn_merge64(ld[qi], lj[qi], bd, bj, lane);
                td = __shfl(ld[qi], k - 1);
                tj = __shfl(lj[qi], k - 1);
            } else {
                const int n = k + cnt[qi];
                int p = 2;
                while (p < n) p <<= 1;                  // p <= cap: n <= cap and cap is a power of two
                for (int i = n + lane; i < p; i += 64) {
                    ed[i] = KN_PAD_D;
                    ej[i] = KN_PAD_J;
                }
                __builtin_amdgcn_wave_barrier();
                kn_sort_lds(ed, ej, p, lane);
                td = ed[k - 1];
                tj = ej[k - 1];
            }
            if (lane == 0) {
                s_tau_d[qi] = td;
                s_tau_j[qi] = tj;
            }
            cnt[qi] = 0;
            __builtin_amdgcn_wave_barrier();
        };

        for (long long r0 = 0; r0 < A.nr; r0 += rt) {
            __syncthreads();                        // the tile before is used up
            {
                const long long n_el = (A.nr - r0 < rt ? A.nr - r0 : (long long)rt) * dim;
                const double *src = A.x + r0 * dim;
                int row = tid / dim, c = tid - row * dim;
                for (int e = tid; e < rt * dim; e += KN_WG) {          // rows past the end are zeros: finite sums, never candidates
                    s_x[c * rtp + row] = e < n_el ? src[e] : 0.0;
                    row += step_row;
                    c += step_c;
                    if (c >= dim) { c -= dim; ++row; }
                }
            }
            __syncthreads();
            for (int sub = 0; sub < rt && r0 + sub < A.nr; sub += 64) {
                double acc[QW];
#pragma unroll
                for (int qi = 0; qi < QW; ++qi) acc[qi] = 0.0;
                const double *xp = s_x + sub + lane;
                for (int c = 0; c < dim; ++c) {
                    const double xv = xp[c * rtp];
#pragma unroll
                    for (int qi = 0; qi < QW; ++qi) {
                        const double t = s_q[c * QW + qi] - xv;
                        acc[qi] = acc[qi] + t * t;
                    }
                }
                const long long j = r0 + sub + lane;
#pragma unroll
                for (int qi = 0; qi < QW; ++qi) {
                    const long long qg = q0 + qi;
                    if (qg >= A.nq) continue;       // wave-uniform
                    const u64 d = (u64)__double_as_longlong(acc[qi]);
                    const bool mine = j < A.nr && !(A.self_offset >= 0 && j == qg + A.self_offset);
                    bool cand = mine && kn_less(d, (int)j, s_tau_d[qi], s_tau_j[qi]);
                    u64 m = __ballot(cand);
                    if (m == 0) continue;
                    if (buf0 + cnt[qi] + __popcll(m) > cap) {
                        reduce(qi);
                        cand = cand && kn_less(d, (int)j, s_tau_d[qi], s_tau_j[qi]);
                        m = __ballot(cand);
                    }
                    if (cand) {
                        const int pos = qi * cap + buf0 + cnt[qi] + __popcll(m & below);
                        s_ent_d[pos] = d;
                        s_ent_j[pos] = (int)j;
                    }
                    cnt[qi] += __popcll(m);
                }
            }
        }
        // what is left in the buffers, and the rows of the result
#pragma unroll
        for (int qi = 0; qi < QW; ++qi) {
            const long long qg = q0 + qi;
            if (qg >= A.nq) continue;
            if (cnt[qi] > 0) reduce(qi);
            if (WAVE) {
                if (lane < k) {
                    const bool pad = ld[qi] == KN_PAD_D;
                    A.idx[qg * k + lane] = pad ? -1 : lj[qi];
                    A.dist2[qg * k + lane] = pad ? __longlong_as_double(0x7ff0000000000000LL) : __longlong_as_double((long long)ld[qi]);
                }
            } else {
                for (int i = lane; i < k; i += 64) {
                    const u64 d = s_ent_d[qi * cap + i];
                    const bool pad = d == KN_PAD_D;
                    A.idx[qg * k + i] = pad ? -1 : s_ent_j[qi * cap + i];
                    A.dist2[qg * k + i] = pad ? __longlong_as_double(0x7ff0000000000000LL) : __longlong_as_double((long long)d);
                }
            }
        }
        __builtin_amdgcn_wave_barrier();        // the next tile's queries overwrite s_q and the arrays
    }
}

// how a call launches: what natac_knn runs and natac_knn_plan reports
struct KnPlan {
    int arm;                       // 0 wave, 1 lds
    int wave_k_max;
    int query_tile;                // queries of a workgroup: 4, 8, 16 or 32
    int ref_tile;                  // references staged at a time: 64, 128 or 256
    int capacity;                  // candidates a query's buffer holds: 64 (wave) or C - k (lds)
    int entries;                   // entries of a query's LDS array: 64 (wave) or C
    int wg;
    long long lds;                 // dynamic LDS of a workgroup, bytes
    int grid;
};

static long long kn_env(const char *name) {
    const char *e = getenv(name);
    return e ? atoll(e) : 0;
}

static bool kn_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

// bytes of kn_search's carve-up for qw queries a wave
static long long kn_lds_bytes(int dim, int rt, int qw, int entries) {
    return 8LL * dim * (rt + 1) + 8LL * KN_WAVES * dim * qw + 12LL * KN_WAVES * qw * (1 + entries);
}

// Unless forced: the reference tile is the largest of 256, 128, 64 whose transposed copy stays within 24 KiB; a wave takes 8 queries,
// halved while the query tiles are fewer than 4 n_cu (wave arm) or 8 n_cu (lds arm, a full grid: measured, EXPERIMENTS R17) or the
// workgroup takes more than 80 KiB of LDS.
static void kn_plan(long long nq, int dim, int k, int n_cu, KnPlan *p) {
    const long long wk = kn_env("NATAC_KNN_WAVE_K_MAX");
    p->wave_k_max = wk >= 1 && wk <= 64 ? (int)wk : 64;
    p->arm = k <= p->wave_k_max ? 0 : 1;
    int c = 128;
    while (c < k + 64) c <<= 1;
    p->entries = p->arm == 0 ? 64 : c;
    p->capacity = p->arm == 0 ? 64 : c - k;
    int rt = KN_MAX_RT;
    while (rt > KN_MIN_RT && 8LL * dim * (rt + 1) > 24 * 1024) rt >>= 1;
    const long long frt = kn_env("NATAC_KNN_REF_TILE");
    if (kn_pow2(frt) && frt >= KN_MIN_RT && frt <= KN_MAX_RT && kn_lds_bytes(dim, (int)frt, 1, p->entries) <= KN_LDS_CAP) rt = (int)frt;
    p->ref_tile = rt;
    int qw = KN_MAX_QW;
    while (qw > 1 && ((nq + KN_WAVES * qw - 1) / (KN_WAVES * qw) < (p->arm == 0 ? 4LL : 8LL) * n_cu || kn_lds_bytes(dim, rt, qw, p->entries) > KN_LDS_SHARE)) qw >>= 1;
    const long long fqt = kn_env("NATAC_KNN_QUERY_TILE");
    if (kn_pow2(fqt) && fqt >= KN_WAVES && fqt <= KN_WAVES * KN_MAX_QW && kn_lds_bytes(dim, rt, (int)fqt / KN_WAVES, p->entries) <= KN_LDS_CAP)
        qw = (int)fqt / KN_WAVES;
    p->query_tile = KN_WAVES * qw;
    p->wg = KN_WG;
    p->lds = kn_lds_bytes(dim, rt, qw, p->entries);
    p->grid = (int)std::max<long long>(1, std::min<long long>((nq + p->query_tile - 1) / p->query_tile, 8LL * n_cu));
}

static int kn_check_sizes(int64_t nq, int64_t nr, int32_t dim, int32_t k) {
    if (dim < 1 || dim > NATAC_KNN_MAX_DIM) return fail(NATAC_E_ARG, "dim must be in [1, %d] (got %d)", NATAC_KNN_MAX_DIM, dim);
    if (k < 1 || k > NATAC_KNN_MAX_K) return fail(NATAC_E_ARG, "k must be in [1, %d] (got %d)", NATAC_KNN_MAX_K, k);
    if (nr < 1 || nr > NATAC_KNN_MAX_REFS) return fail(NATAC_E_ARG, "nr must be in [1, %d] (got %lld)", NATAC_KNN_MAX_REFS, (long long)nr);
    if (nq < 0) return fail(NATAC_E_ARG, "nq must be at least 0 (got %lld)", (long long)nq);
    if ((unsigned __int128)nq * (unsigned)k > (unsigned __int128)NATAC_KNN_MAX_OUT)
        return fail(NATAC_E_ARG, "nq * k must be at most %d (got %lld * %d): cut the queries into blocks", NATAC_KNN_MAX_OUT, (long long)nq, k);
    return NATAC_OK;
}

static int kn_check_values(const char *name, const double *v, long long n) {
    for (long long i = 0; i < n; ++i)
        if (!(std::fabs(v[i]) <= 0x1p500))
            return fail(NATAC_E_ARG, "%s[%lld] = %g: every value must be finite and at most 2^500 in magnitude", name, i, v[i]);
    return NATAC_OK;
}

template <bool WAVE>
static void kn_launch(int qw, unsigned grid, size_t lds, hipStream_t stream, const KnArgs &A) {
    switch (qw) {
    case 1: hipLaunchKernelGGL((kn_search<1, WAVE>), dim3(grid), dim3(KN_WG), lds, stream, A); break;
    case 2: hipLaunchKernelGGL((kn_search<2, WAVE>), dim3(grid), dim3(KN_WG), lds, stream, A); break;
    case 4: hipLaunchKernelGGL((kn_search<4, WAVE>), dim3(grid), dim3(KN_WG), lds, stream, A); break;
    default: hipLaunchKernelGGL((kn_search<8, WAVE>), dim3(grid), dim3(KN_WG), lds, stream, A); break;
    }
}

template <bool WAVE>
static hipError_t kn_allow_lds(int qw, int lds) {
    switch (qw) {
    case 1: return hipFuncSetAttribute((const void *)kn_search<1, WAVE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    case 2: return hipFuncSetAttribute((const void *)kn_search<2, WAVE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    case 4: return hipFuncSetAttribute((const void *)kn_search<4, WAVE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    default: return hipFuncSetAttribute((const void *)kn_search<8, WAVE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    }
}

}  // namespace natac_knn_ns

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_knn(natac_ctx *c, int64_t nq, int64_t nr, int32_t dim, const double *q, const double *x, int64_t self_offset, int32_t k,
              int32_t *idx, double *dist2, int64_t *arm_queries, double *kernel_ms) {
    using namespace natac_knn_ns;
    if (!c || !x || (nq > 0 && (!q || !idx || !dist2))) return fail(NATAC_E_ARG, "null argument");
    if (const int rc = kn_check_sizes(nq, nr, dim, k)) return rc;
    if (self_offset != -1 && (self_offset < 0 || self_offset > nr - nq))
        return fail(NATAC_E_ARG, "self_offset must be -1 or in [0, nr - nq] (got %lld with nr %lld, nq %lld)", (long long)self_offset, (long long)nr,
                    (long long)nq);
    if (const int rc = kn_check_values("x", x, (long long)nr * dim)) return rc;
    const bool same = q == x && nq <= nr;       // the queries are the first nq references
    if (!same)
        if (const int rc = kn_check_values("q", q, (long long)nq * dim)) return rc;
    if (kernel_ms) *kernel_ms = 0;
    if (arm_queries) arm_queries[0] = arm_queries[1] = 0;
    if (nq == 0) return NATAC_OK;
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);     // 256 stands if the query fails
    KnPlan plan;
    kn_plan(nq, dim, k, n_cu, &plan);
    if (plan.lds > KN_LDS_CAP) return fail(NATAC_E_ARG, "knn: the plan takes %lld bytes of LDS", plan.lds);

    DeviceCall dc(c, "knn");
    KnArgs A;
    A.x = dc.upload(x, (size_t)nr * dim);
    A.q = same ? A.x : dc.upload(q, (size_t)nq * dim);
    A.nq = nq;
    A.nr = nr;
    A.self_offset = self_offset;
    A.dim = dim;
    A.k = k;
    A.rt = plan.ref_tile;
    A.cap = plan.entries;
    A.idx = dc.alloc<int>((size_t)nq * k);
    A.dist2 = dc.alloc<double>((size_t)nq * k);
    const int qw = plan.query_tile / KN_WAVES;
    if (plan.lds >= 64 * 1024) HIPCHK(plan.arm == 0 ? kn_allow_lds<true>(qw, (int)plan.lds) : kn_allow_lds<false>(qw, (int)plan.lds));
    dc.time_begin(kernel_ms);
    if (dc.ok()) {
        if (plan.arm == 0) kn_launch<true>(qw, (unsigned)plan.grid, (size_t)plan.lds, c->stream, A);
        else kn_launch<false>(qw, (unsigned)plan.grid, (size_t)plan.lds, c->stream, A);
        dc.launched();
    }
    dc.time_end();
    dc.fetch(idx, A.idx, (size_t)nq * k);
    dc.fetch(dist2, A.dist2, (size_t)nq * k);
    const int rc = dc.finish();
    if (rc == NATAC_OK && arm_queries) arm_queries[plan.arm] = nq;
    return rc;
}

int natac_knn_plan(int64_t nq, int64_t nr, int32_t dim, int32_t k, int32_t n_cu, int32_t *arm, int32_t *wave_k_max, int32_t *query_tile,
                   int32_t *ref_tile, int32_t *capacity, int32_t *wg, int64_t *lds_bytes, int32_t *grid) {
    using namespace natac_knn_ns;
    if (!arm || !wave_k_max || !query_tile || !ref_tile || !capacity || !wg || !lds_bytes || !grid) return fail(NATAC_E_ARG, "null argument");
    if (const int rc = kn_check_sizes(nq, nr, dim, k)) return rc;
    if (n_cu < 1) return fail(NATAC_E_ARG, "n_cu must be at least 1 (got %d)", n_cu);
    KnPlan p;
    kn_plan(nq, dim, k, n_cu, &p);
    *arm = p.arm;
    *wave_k_max = p.wave_k_max;
    *query_tile = p.query_tile;
    *ref_tile = p.ref_tile;
    *capacity = p.capacity;
    *wg = p.wg;
    *lds_bytes = p.lds;
    *grid = p.grid;
    return NATAC_OK;
}

}  // extern "C"
