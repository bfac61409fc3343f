// natac_deviations.hpp -- the kernels behind `pyatac deviations` (this package's own command: the reference has no such tool): per-cell
// motif accessibility deviations against sampled background window sets (natac_motif_deviations, include/natac.h states the rule), and
// the per-range base counts its GC content comes from (natac_window_base_counts).
//
// The counts arrive as natac_region_cell_counts leaves them: CSR with one row per window (P of them), the cells (N) ascending within a
// row.  A motif is a set of windows; bg[b - 1][p] is the window that stands in for window p in background set b = 1 .. B, set 0 is the
// windows themselves.  For every set b, motif m and cell c
//   O_b[m, c] = sum over the motif's windows p of X[bg_b(p), c]        E_b[m] = sum over the motif's windows p of rs[bg_b(p)]
// are exact integers, and in fp64, one rounded operation at a time,
//   x = double(E_b) * double(d[c]) / double(T),   Y_b = (double(O_b) - x) / x,
//   raw = Y_0,   and over b = 1 .. B in order:   delta = Y_b - mean,  mean += delta / b,  M2 += delta * (Y_b - mean).
//
// Kernel dev_motif_tiles: a workgroup owns one motif and one tile of `tile` consecutive cells and loops over b itself.  Per b its waves
// walk the motif's windows 64 at a time.  First every lane looks up a window of its own: p, bg_b(p) and the piece of that row of X that
// lies in the tile -- the entry point splits every row by tile once per call (split[p][t] = the first entry of row p with a cell of tile
// t or later; the entries stay where they are) -- and adds rs[bg_b(p)] into an int64 of its own.  Then the wave adds up the 64 pieces,
// `lanes` lanes to a piece (the bounds come from the owning lane by a shuffle), into per-cell integer counters in LDS with LDS atomics,
// the first entries of DEV_FLIGHT pieces loaded before any is added.  The lanes' rs sums are reduced by shuffles within the wave and
// across the waves through LDS.  Behind a barrier every thread turns its cells' counters into Y_b, advances mean and M2 (fp64 in LDS,
// carried over b) and clears the counters.
// The counters are 32-bit when the largest sum a counter can reach (the largest motif times the largest count) is below 2^32 and 64-bit
// otherwise, so every sum is exact; integer adds commute, the order over b is sequential per element and there are no floating-point
// atomics: the result is a pure function of the operands and does not depend on the tile or on the lane group.
// Behind the kernels: the entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "natac_pwmfit.hpp"
#include "natac_runtime.hpp"

namespace natac_dev {

constexpr int DEV_BLOCK = 1024;             // 16 waves: two workgroups fill a CU's 32 wave slots
constexpr int DEV_WAVES = DEV_BLOCK / 64;
constexpr int DEV_FLIGHT = 4;               // pieces whose first entries a lane has in flight at once
constexpr int DEV_TILE = 4096;              // NATAC_DEVIATIONS_TILE: 4 + 16 bytes of LDS per cell, 80 KiB, two workgroups per CU
constexpr int DEV_MIN_TILE = 256;           // the smallest tile the entry shrinks to on its own
constexpr int DEV_MAX_B = 1024;             // NATAC_DEVIATIONS_MAX_B
constexpr long long DEV_MAX_DEBUG = 1LL << 24;   // NATAC_DEVIATIONS_MAX_DEBUG: the most O_b values the testing output holds
constexpr int WBC_BLOCK = 256;

// counts[i][0 .. 4) = the A / C / G / T bases of seq[start[i] .. end[i]): one wave per range, lane t reads bases t, t + 64, ...
__global__ void __launch_bounds__(WBC_BLOCK) dev_window_base_count(const unsigned char *__restrict__ seq, long long nr,
                                                                   const long long *__restrict__ start, const long long *__restrict__ end,
                                                                   long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * (WBC_BLOCK / 64);
    for (long long i = (long long)blockIdx.x * (WBC_BLOCK / 64) + (threadIdx.x >> 6); i < nr; i += nwaves) {   // wave-uniform
        const long long s = start[i], e = end[i];
        unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (long long v = s + lane; v < e; v += 64) {
            const unsigned b = natac_pwmfit::base_row(seq[v]);
            a0 += b == 0u; a1 += b == 1u; a2 += b == 2u; a3 += b == 3u;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); a3 += __shfl_xor(a3, off);
        }
        if (lane == 0) {
            counts[i * 4 + 0] = (long long)a0; counts[i * 4 + 1] = (long long)a1;
            counts[i * 4 + 2] = (long long)a2; counts[i * 4 + 3] = (long long)a3;
        }
    }
}

// the layout of a workgroup's dynamic LDS for a tile of `tile` cells and counters of type CT:
//   double mean[tile], m2[tile]; long long wave_sum[DEV_WAVES]; CT cnt[tile]
template <class CT>
static size_t dev_lds_bytes(int tile) {
    return (size_t)tile * (2 * sizeof(double) + sizeof(CT)) + DEV_WAVES * sizeof(long long);
}

// blockIdx.x = motif * n_tiles + tile.  lanes: a power of two in [1, 64], the lanes that share a piece of a row.
template <class CT>
__global__ void __launch_bounds__(DEV_BLOCK) dev_motif_tiles(int P, int N, int M, int n_tiles, int tile, int lanes, int B,
                                                             const int *__restrict__ split, const int *__restrict__ col,
                                                             const int *__restrict__ count, const int *__restrict__ rs,
                                                             const int *__restrict__ d, double T, const long long *__restrict__ mot_ptr,
                                                             const int *__restrict__ mot_win, const int *__restrict__ bg,
                                                             double *__restrict__ raw, double *__restrict__ bg_mean,
                                                             double *__restrict__ bg_m2, long long *__restrict__ obs,
                                                             long long *__restrict__ expect) {
    extern __shared__ double s_dyn[];
    double *s_mean = s_dyn, *s_m2 = s_dyn + tile;
    long long *s_wave = (long long *)(s_dyn + 2 * (size_t)tile);
    CT *s_cnt = (CT *)(s_wave + DEV_WAVES);
    const int m = blockIdx.x / n_tiles, t = blockIdx.x - m * n_tiles;
    const int c0 = t * tile, nc = min(tile, N - c0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & (lanes - 1), piece = lane / lanes, per = 64 / lanes;        // `per` pieces per step of a wave
    const long long w0 = mot_ptr[m], w1 = mot_ptr[m + 1];
    const size_t stride = (size_t)n_tiles + 1;
    for (int i = tid; i < nc; i += DEV_BLOCK) {
        s_mean[i] = 0.0;
        s_m2[i] = 0.0;
        s_cnt[i] = 0;
    }
    __syncthreads();
    for (int b = 0; b <= B; ++b) {
        const int *bgb = b ? bg + (size_t)(b - 1) * P : nullptr;
        long long e_part = 0;
        for (long long base = w0 + wave * 64; base < w1; base += DEV_BLOCK) {         // wave-uniform: every lane shuffles
            // every lane looks up a window of its own: 64 chains of dependent loads in flight per wave
            int k0 = 0, k1 = 0;
            if (base + lane < w1) {
                const int p = mot_win[base + lane];
                const int q = bgb ? bgb[p] : p;
                const int *sp = split + (size_t)q * stride + t;
                k0 = sp[0];
                k1 = sp[1];
                e_part += rs[q];
            }
            // then the wave adds up its 64 pieces, `lanes` lanes to a piece, the first entries of DEV_FLIGHT pieces loaded before any is added
            const int n_win = (int)min((long long)64, w1 - base);
            for (int j = 0; j < n_win; j += per * DEV_FLIGHT) {
                int a[DEV_FLIGHT], z[DEV_FLIGHT], cc[DEV_FLIGHT], vv[DEV_FLIGHT];
#pragma unroll
                for (int u = 0; u < DEV_FLIGHT; ++u) {
                    const int src = j + u * per + piece;
                    a[u] = __shfl(k0, src & 63) + sub;
                    z[u] = src < 64 ? __shfl(k1, src & 63) : 0;
                }
#pragma unroll
                for (int u = 0; u < DEV_FLIGHT; ++u) {
                    const bool on = a[u] < z[u];
                    cc[u] = on ? col[a[u]] : 0;
                    vv[u] = on ? count[a[u]] : 0;
                }
#pragma unroll
                for (int u = 0; u < DEV_FLIGHT; ++u)
                    if (a[u] < z[u]) atomicAdd(&s_cnt[cc[u] - c0], (CT)vv[u]);
#pragma unroll
                for (int u = 0; u < DEV_FLIGHT; ++u)
                    for (int k = a[u] + lanes; k < z[u]; k += lanes) atomicAdd(&s_cnt[col[k] - c0], (CT)count[k]);      // pieces longer than `lanes`
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) e_part += __shfl_xor(e_part, off);
        if (lane == 0) s_wave[wave] = e_part;
        __syncthreads();                                    // the counters and the waves' sums are complete
        long long E = 0;
#pragma unroll
        for (int i = 0; i < DEV_WAVES; ++i) E += s_wave[i];
        if (expect && t == 0 && tid == 0) expect[(size_t)b * M + m] = E;
        const double Ed = (double)E;
        for (int i = tid; i < nc; i += DEV_BLOCK) {
            const long long O = (long long)s_cnt[i];
            s_cnt[i] = 0;
            const double x = Ed * (double)d[c0 + i] / T;
            const double Y = ((double)O - x) / x;
            const size_t o = (size_t)m * N + c0 + i;
            if (b == 0) {
                raw[o] = Y;
            } else {
                const double delta = Y - s_mean[i];
                const double mean = s_mean[i] + delta / (double)b;
                s_mean[i] = mean;
                s_m2[i] += delta * (Y - mean);
            }
            if (obs) obs[((size_t)b * M + m) * N + c0 + i] = O;
        }
        __syncthreads();                                    // the counters are clear and s_wave is read before the next set writes them
    }
    for (int i = tid; i < nc; i += DEV_BLOCK) {
        const size_t o = (size_t)m * N + c0 + i;
        bg_mean[o] = s_mean[i];
        bg_m2[o] = s_m2[i];
    }
}

// the cell tile of a call: NATAC_DEVIATIONS_CELL_TILE when set (the tests), else DEV_TILE, halved while motifs x tiles leaves CUs idle,
// then evened out over that number of tiles (a multiple of 64)
static int dev_tile_size(long long n, long long M, int n_cu) {
    if (const char *e = getenv("NATAC_DEVIATIONS_CELL_TILE")) {
        const long long v = atoll(e);
        if (v >= 1 && v <= DEV_TILE) return (int)v;
    }
    int tile = DEV_TILE;
    while (tile > DEV_MIN_TILE && M * ((n + tile - 1) / tile) < 2LL * n_cu) tile /= 2;
    const long long n_tiles = (n + tile - 1) / tile;       // the same number of tiles, of even size
    return (int)std::min<long long>(tile, ((n + n_tiles - 1) / n_tiles + 63) / 64 * 64);
}

// how a call launches: what natac_motif_deviations runs and natac_motif_deviations_plan reports
struct DevPlan {
    int tile;              // cells per workgroup
    long long n_tiles;     // the grid is n_motifs * n_tiles workgroups
    int lanes;             // the lanes that share a piece of a row: the power of two at or above the mean piece of a row inside a tile
    bool wide;             // 64-bit counters: the largest motif times the largest count reaches 2^32
    size_t lds;            // dynamic LDS of a workgroup, bytes
};

// the plan for m windows, n cells, nnz entries and M motifs, the largest of max_set windows, the largest count max_count, on n_cu compute
// units (all positive); false when motifs x tiles or windows x tiles are too many for one call (tile and n_tiles are set all the same)
static bool dev_plan(long long m, long long n, long long nnz, long long M, long long max_set, long long max_count, int n_cu, DevPlan *p) {
    p->tile = dev_tile_size(n, M, n_cu);
    p->n_tiles = (n + p->tile - 1) / p->tile;
    p->lanes = 0;
    p->wide = false;
    p->lds = 0;
    if (M * p->n_tiles > 2147483647LL || m * (p->n_tiles + 1) > (1LL << 33)) return false;
    p->lanes = 1;
    while (p->lanes < 64 && (long long)p->lanes * m * p->n_tiles < nnz) p->lanes *= 2;
    p->wide = max_set * max_count >= (1LL << 32);
    p->lds = p->wide ? dev_lds_bytes<unsigned long long>(p->tile) : dev_lds_bytes<unsigned>(p->tile);
    return true;
}

}  // namespace natac_dev

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_window_base_counts(natac_ctx *c, const uint8_t *seq, int64_t n, int64_t nr, const int64_t *start, const int64_t *end,
                             int64_t *counts) {
    using namespace natac_dev;
    if (!c || n < 0 || nr < 0) return fail(NATAC_E_ARG, "null argument or negative size");
    if (nr > 0 && (!start || !end || !counts)) return fail(NATAC_E_ARG, "null argument");
    long long total = 0;
    for (int64_t i = 0; i < nr; ++i) {
        if (start[i] < 0 || end[i] < start[i] || end[i] > n)
            return fail(NATAC_E_ARG, "range %lld [%lld, %lld) outside [0, %lld)", (long long)i, (long long)start[i], (long long)end[i], (long long)n);
        total += end[i] - start[i];
    }
    if (total > 0 && !seq) return fail(NATAC_E_ARG, "null argument");
    for (int64_t i = 0; i < 4 * nr; ++i) counts[i] = 0;
    if (total == 0) return NATAC_OK;
    DeviceCall dc(c, "window_base_counts");
    const unsigned char *d_s = dc.upload((const unsigned char *)seq, (size_t)n);
    const long long *d_st = dc.upload((const long long *)start, (size_t)nr), *d_en = dc.upload((const long long *)end, (size_t)nr);
    long long *d_out = dc.alloc<long long>((size_t)nr * 4);
    if (dc.ok()) {
        const unsigned bx = (unsigned)std::min<long long>((nr + WBC_BLOCK / 64 - 1) / (WBC_BLOCK / 64), 16384);
        hipLaunchKernelGGL(dev_window_base_count, dim3(bx), dim3(WBC_BLOCK), 0, c->stream, d_s, (long long)nr, d_st, d_en, d_out);
        dc.launched();
    }
    dc.fetch(counts, d_out, (size_t)nr * 4);
    return dc.finish();
}

int natac_motif_deviations(natac_ctx *c, int64_t m, int64_t n, const int64_t *row_ptr, const int32_t *col, const int32_t *count,
                           int32_t n_motifs, const int64_t *mot_ptr, const int32_t *mot_win, int32_t n_bg, const int32_t *bg, double *raw,
                           double *bg_mean, double *bg_m2, int64_t *obs, int64_t *expect, double *kernel_ms) {
    using namespace natac_dev;
    static_assert(DEV_TILE == NATAC_DEVIATIONS_TILE && DEV_MAX_B == NATAC_DEVIATIONS_MAX_B && DEV_MAX_DEBUG == NATAC_DEVIATIONS_MAX_DEBUG,
                  "the limits are in natac.h");
    if (!c || !row_ptr) return fail(NATAC_E_ARG, "null argument");
    if (m < 0 || n < 0 || m > 2147483647LL || n > 2147483647LL) return fail(NATAC_E_ARG, "m and n must be in [0, 2^31)");
    if (n_motifs < 0) return fail(NATAC_E_ARG, "negative motif count");
    if (n_bg < 2 || n_bg > DEV_MAX_B) return fail(NATAC_E_ARG, "the number of background sets must be in [2, %d] (got %d)", DEV_MAX_B, n_bg);
    if ((obs == nullptr) != (expect == nullptr)) return fail(NATAC_E_ARG, "obs and expect go together");
    const int64_t M = n_motifs;
    if (obs && ((long long)n_bg + 1) * M * n > DEV_MAX_DEBUG)
        return fail(NATAC_E_ARG, "the testing output holds at most %lld values (asked for %lld)", DEV_MAX_DEBUG, ((long long)n_bg + 1) * M * n);
    if (row_ptr[0] < 0) return fail(NATAC_E_ARG, "row_ptr[0] is negative");
    for (int64_t i = 0; i < m; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) return fail(NATAC_E_ARG, "row_ptr is not monotone (row %lld)", (long long)i);
        if (row_ptr[i + 1] == row_ptr[i]) return fail(NATAC_E_ARG, "window %lld has no entry", (long long)i);
    }
    const int64_t e0 = row_ptr[0], nnz = row_ptr[m] - e0;
    if (nnz > 0 && (!col || !count)) return fail(NATAC_E_ARG, "null argument");
    std::vector<int> rs((size_t)m), d((size_t)n, 0);
    long long T = 0, max_count = 0;
    for (int64_t i = 0; i < m; ++i) {
        long long row = 0;
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) return fail(NATAC_E_ARG, "row %lld: column %d outside [0, %lld)", (long long)i, col[e], (long long)n);
            if (e > row_ptr[i] && col[e] <= col[e - 1]) return fail(NATAC_E_ARG, "row %lld: columns must be strictly ascending", (long long)i);
            if (count[e] < 1) return fail(NATAC_E_ARG, "row %lld: count %d is below 1", (long long)i, count[e]);
            row += count[e];
            T += count[e];
            if (T >= (1LL << 31)) return fail(NATAC_E_ARG, "row %lld: the total count reaches 2^31", (long long)i);
            max_count = std::max<long long>(max_count, count[e]);
        }
        rs[(size_t)i] = (int)row;
    }
    for (int64_t e = e0; e < e0 + nnz; ++e) d[(size_t)col[e]] += count[e];
    for (int64_t i = 0; i < n; ++i)
        if (d[(size_t)i] == 0) return fail(NATAC_E_ARG, "cell %lld has no entry", (long long)i);
    if (M > 0 && !mot_ptr) return fail(NATAC_E_ARG, "null argument");
    long long max_set = 0;
    if (M > 0) {
        if (mot_ptr[0] != 0) return fail(NATAC_E_ARG, "mot_ptr[0] must be 0");
        for (int64_t k = 0; k < M; ++k) {
            if (mot_ptr[k + 1] <= mot_ptr[k]) return fail(NATAC_E_ARG, "motif %lld has no window", (long long)k);
            if (!mot_win) return fail(NATAC_E_ARG, "null argument");
            for (int64_t w = mot_ptr[k]; w < mot_ptr[k + 1]; ++w) {
                if (mot_win[w] < 0 || mot_win[w] >= m) return fail(NATAC_E_ARG, "motif %lld: window %d outside [0, %lld)", (long long)k, mot_win[w], (long long)m);
                if (w > mot_ptr[k] && mot_win[w] <= mot_win[w - 1]) return fail(NATAC_E_ARG, "motif %lld: windows must be strictly ascending", (long long)k);
            }
            max_set = std::max<long long>(max_set, mot_ptr[k + 1] - mot_ptr[k]);
        }
    }
    if (m > 0 && !bg) return fail(NATAC_E_ARG, "null argument");
    for (int64_t i = 0; i < (int64_t)n_bg * m; ++i)
        if (bg[i] < 0 || bg[i] >= m) return fail(NATAC_E_ARG, "bg[%lld] = %d outside [0, %lld)", (long long)i, bg[i], (long long)m);
    if (M > 0 && n > 0 && (!raw || !bg_mean || !bg_m2)) return fail(NATAC_E_ARG, "null argument");
    if (kernel_ms) *kernel_ms = 0;
    if (M == 0 || n == 0 || m == 0) return NATAC_OK;

    int n_cu = 256;
    hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
    DevPlan plan;
    if (!dev_plan(m, n, nnz, M, max_set, max_count, n_cu, &plan))
        return fail(NATAC_E_ARG, "%lld motifs x %lld cell tiles of %d x %lld windows are too many for one call", (long long)M, plan.n_tiles, plan.tile, (long long)m);
    const int tile = plan.tile, lanes = plan.lanes;
    const long long n_tiles = plan.n_tiles;
    const bool wide = plan.wide;
    const size_t lds = plan.lds;
    // every row split by tile: split[p][t] = the first entry of row p (counted from e0) whose cell is in tile t or later
    std::vector<int> split((size_t)m * (size_t)(n_tiles + 1));
    for (int64_t i = 0; i < m; ++i) {
        int64_t e = row_ptr[i];
        int *sp = &split[(size_t)i * (size_t)(n_tiles + 1)];
        for (long long t = 0; t <= n_tiles; ++t) {
            while (e < row_ptr[i + 1] && col[e] < t * tile) ++e;
            sp[t] = (int)(e - e0);
        }
    }
    DeviceCall dc(c, "motif_deviations");
    const int *d_split = dc.upload(split.data(), split.size());
    const int *d_col = dc.upload((const int *)(col + e0), (size_t)nnz), *d_cnt = dc.upload((const int *)(count + e0), (size_t)nnz);
    const int *d_rs = dc.upload(rs.data(), rs.size()), *d_d = dc.upload(d.data(), d.size());
    const long long *d_mp = dc.upload((const long long *)mot_ptr, (size_t)M + 1);
    const int *d_mw = dc.upload((const int *)mot_win, (size_t)mot_ptr[M]);
    const int *d_bg = dc.upload((const int *)bg, (size_t)n_bg * (size_t)m);
    double *d_raw = dc.alloc<double>((size_t)M * n), *d_mean = dc.alloc<double>((size_t)M * n), *d_m2 = dc.alloc<double>((size_t)M * n);
    long long *d_obs = obs ? dc.alloc<long long>((size_t)(n_bg + 1) * M * n) : nullptr;
    long long *d_exp = obs ? dc.alloc<long long>((size_t)(n_bg + 1) * M) : nullptr;
    dc.time_begin(kernel_ms);
    if (dc.ok()) {
        auto kfn = wide ? dev_motif_tiles<unsigned long long> : dev_motif_tiles<unsigned>;
        if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kfn, dim3((unsigned)(M * n_tiles)), dim3(DEV_BLOCK), lds, c->stream, (int)m, (int)n, (int)M, (int)n_tiles, tile, lanes,
                           (int)n_bg, d_split, d_col, d_cnt, d_rs, d_d, (double)T, d_mp, d_mw, d_bg, d_raw, d_mean, d_m2, d_obs, d_exp);
        dc.launched();
    }
    dc.time_end();
    // into temporaries first: a failed call leaves the caller's arrays as they were
    std::vector<double> h_raw((size_t)M * n), h_mean((size_t)M * n), h_m2((size_t)M * n);
    std::vector<long long> h_obs(obs ? (size_t)(n_bg + 1) * M * n : 0), h_exp(obs ? (size_t)(n_bg + 1) * M : 0);
    dc.fetch(h_raw.data(), d_raw, h_raw.size());
    dc.fetch(h_mean.data(), d_mean, h_mean.size());
    dc.fetch(h_m2.data(), d_m2, h_m2.size());
    if (obs) {
        dc.fetch(h_obs.data(), d_obs, h_obs.size());
        dc.fetch(h_exp.data(), d_exp, h_exp.size());
    }
    if (const int rc = dc.finish()) return rc;
    std::copy(h_raw.begin(), h_raw.end(), raw);
    std::copy(h_mean.begin(), h_mean.end(), bg_mean);
    std::copy(h_m2.begin(), h_m2.end(), bg_m2);
    if (obs) {
        std::copy(h_obs.begin(), h_obs.end(), (long long *)obs);
        std::copy(h_exp.begin(), h_exp.end(), (long long *)expect);
    }
    return NATAC_OK;
}

int natac_motif_deviations_plan(int64_t m, int64_t n, int64_t nnz, int32_t n_motifs, int64_t max_set, int64_t max_count, int32_t n_cu,
                                int32_t *tile, int64_t *n_tiles, int32_t *lanes, int32_t *wide, int64_t *lds_bytes) {
    using namespace natac_dev;
    if (!tile || !n_tiles || !lanes || !wide || !lds_bytes) return fail(NATAC_E_ARG, "null argument");
    if (m < 1 || n < 1 || nnz < 1 || n_motifs < 1 || max_set < 1 || max_count < 1 || n_cu < 1 || m > 2147483647LL || n > 2147483647LL ||
        max_set > 2147483647LL || max_count > 2147483647LL)
        return fail(NATAC_E_ARG, "natac_motif_deviations_plan: positive sizes; m, n, max_set and max_count below 2^31");
    DevPlan p;
    if (!dev_plan(m, n, nnz, n_motifs, max_set, max_count, n_cu, &p))
        return fail(NATAC_E_ARG, "%lld motifs x %lld cell tiles of %d x %lld windows are too many for one call", (long long)n_motifs, p.n_tiles, p.tile, (long long)m);
    *tile = p.tile;
    *n_tiles = p.n_tiles;
    *lanes = p.lanes;
    *wide = p.wide ? 1 : 0;
    *lds_bytes = (int64_t)p.lds;
    return NATAC_OK;
}

}  // extern "C"
