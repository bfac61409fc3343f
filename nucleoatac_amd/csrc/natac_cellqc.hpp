// natac_cellqc.hpp -- the kernel behind `pyatac cellqc` (this package's own command: the reference has no such tool): per-cell TSS counts,
// the aggregate TSS profile and per-cell fragments in peaks of one chromosome (natac_cell_site_qc, include/natac.h states the rule).
//
// cq_count is fragment-parallel: one thread per record of the position-sorted store, against two small sorted tables (the site centres
// and the disjoint peak intervals) that stay in L2.  Per record:
//   per-cell counts   the three classes are symmetric in d, so none needs the pairs: with lo / hi the bounds of the centres in
//                     [x - flank, x + flank], the centre class is the number of centres in [x - center, x + center] and the flank class is
//                     hi - lo minus the centres in [x - (flank - edge), x + (flank - edge)], both searched inside [lo, hi).  An insertion
//                     without a site in reach costs two searches; a record adds to tss_center / tss_flank / in_peaks of its cell with one
//                     64-bit atomic each, and only where the count is not zero.
//   in peaks          the last interval that starts at or before l (or r) is the only one that can hold it: the intervals are disjoint.
//   profile           needs the pairs.  It is privatised per workgroup in LDS as 2 * flank + 1 32-bit counters.  An insertion with at most
//                     CQ_LANE_MAX sites in reach is walked by its own lane; one with more is walked by the whole wave, 64 sites a step, and
//                     there neighbouring lanes that hit one column (repeated centres, as the transcripts of one gene give them) are
//                     run-length encoded with a ballot so that one lane adds the run's length.
// Flushing: a workgroup adds at most 2 * CQ_BLOCK * n_sites pairs per tile of CQ_BLOCK records, so after `flush_tiles` tiles with
// flush_tiles * 2 * CQ_BLOCK * n_sites < 2^32 no 32-bit counter has wrapped; the host computes flush_tiles from the n_sites of the launch and
// launches over at most CQ_SITE_CHUNK sites at a time (the sum over any split of the sites is the single call).  A flush adds the non-zero
// counters to the int64 profile with 64-bit global atomics and clears them.  Only integer atomics: the result is a pure function of the inputs.
// Behind the kernel: the entry point with the operand checks and the launches over the site chunks.
#pragma once
#include <hip/hip_runtime.h>

#include "natac_sites.hpp"

namespace natac_cellqc {

constexpr int CQ_BLOCK = 256;                   // NATAC_CELLQC_BLOCK: records per tile, one per thread (4 waves)
constexpr int CQ_MAX_FLANK = 2500;              // NATAC_CELLQC_MAX_FLANK: 5,001 counters = 20,004 B of LDS, 8 workgroups (32 waves) per CU
constexpr int CQ_LANE_MAX = 8;                  // NATAC_CELLQC_LANE_MAX: sites in reach a lane walks alone
constexpr int CQ_MAX_BLOCKS = 2048;             // NATAC_CELLQC_MAX_BLOCKS: 8 workgroups on each of 256 CUs; more tiles are walked grid-stride
constexpr long long CQ_SITE_CHUNK = 1LL << 22;  // NATAC_CELLQC_SITE_CHUNK: sites per launch, 2 * CQ_BLOCK * CQ_SITE_CHUNK = 2^31 pairs per tile at the most

// first index in [lo, hi) with a[i] >= v (hi if none)
__device__ __forceinline__ long long cq_lower(const long long *__restrict__ a, long long lo, long long hi, long long v) {
    while (lo < hi) {
        const long long m = lo + ((hi - lo) >> 1);
        if (a[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}
// first index in [lo, hi) with a[i] > v (hi if none)
__device__ __forceinline__ long long cq_upper(const long long *__restrict__ a, long long lo, long long hi, long long v) {
    while (lo < hi) {
        const long long m = lo + ((hi - lo) >> 1);
        if (a[m] <= v) lo = m + 1; else hi = m;
    }
    return lo;
}

__device__ __forceinline__ bool cq_in_peaks(const long long *__restrict__ ps, const long long *__restrict__ pe, long long np, long long x) {
    const long long j = cq_upper(ps, 0, np, x);
    return j > 0 && x < pe[j - 1];
}

// the pairs of one insertion per lane (x against sites [lo, lo + n), n == 0: none) into the workgroup's profile
__device__ __forceinline__ void cq_profile_pairs(unsigned *s_prof, const long long *__restrict__ sc, const unsigned char *__restrict__ sm,
                                                 int flank, long long x, long long lo, long long n, int lane) {
    if (n > 0 && n <= CQ_LANE_MAX)
        for (long long j = lo; j < lo + n; ++j) {
            const long long c = sc[j];
            const long long d = (sm && sm[j]) ? c - x : x - c;
            atomicAdd(&s_prof[(int)d + flank], 1u);
        }
    unsigned long long big = __ballot(n > CQ_LANE_MAX);            // wave-uniform from here: every lane takes every step
    while (big) {
        const int src = __builtin_ctzll(big);
        big &= big - 1;
        const long long bx = __shfl(x, src), blo = __shfl(lo, src), bhi = blo + __shfl(n, src);
        for (long long j0 = blo; j0 < bhi; j0 += 64) {
            const long long j = j0 + lane;
            const bool on = j < bhi;
            int bin = -1;                                           // (no column: a lane past the end heads no run and ends one)
            if (on) {
                const long long c = sc[j];
                bin = (int)((sm && sm[j]) ? c - bx : bx - c) + flank;
            }
            const int prev = __shfl_up(bin, 1);
            const bool head = on && (lane == 0 || bin != prev);
            const unsigned long long hm = __ballot(head), om = __ballot(on);
            if (head) {
                const unsigned long long rest = lane < 63 ? hm >> (lane + 1) : 0ULL;
                const int next = rest ? lane + 1 + __builtin_ctzll(rest) : __popcll(om);    // the active lanes are 0 .. popc - 1
                atomicAdd(&s_prof[bin], (unsigned)(next - lane));
            }
        }
    }
}

__device__ __forceinline__ void cq_flush(unsigned *s_prof, int K, unsigned long long *__restrict__ profile) {
    __syncthreads();
    for (int b = threadIdx.x; b < K; b += CQ_BLOCK) {
        const unsigned v = s_prof[b];
        if (v) {
            atomicAdd(&profile[b], (unsigned long long)v);
            s_prof[b] = 0u;
        }
    }
    __syncthreads();
}

// out = tss_center[n_cells], tss_flank[n_cells], in_peaks[n_cells], profile[2 * flank + 1], zero before the first launch of a call.
// ns == 0 skips the site part, np == 0 the peak part (the launches after the first of a call pass np == 0).  Dynamic LDS: 2 * flank + 1 words.
__global__ void __launch_bounds__(CQ_BLOCK) cq_count(const long long *__restrict__ pos, const long long *__restrict__ tlen,
                                                     const int *__restrict__ cell, long long nf, int n_cells,
                                                     const long long *__restrict__ sc, const unsigned char *__restrict__ sm, long long ns,
                                                     int flank, int center, int edge, const long long *__restrict__ ps,
                                                     const long long *__restrict__ pe, long long np, long long flush_tiles,
                                                     unsigned long long *__restrict__ out) {
    extern __shared__ unsigned s_prof[];
    const int K = 2 * flank + 1, lane = threadIdx.x & 63, inner = flank - edge;
    unsigned long long *tss_center = out, *tss_flank = out + n_cells, *in_peaks = out + 2 * (size_t)n_cells,
                       *profile = out + 3 * (size_t)n_cells;
    if (ns > 0) {
        for (int b = threadIdx.x; b < K; b += CQ_BLOCK) s_prof[b] = 0u;
        __syncthreads();
    }
    const long long n_tiles = (nf + CQ_BLOCK - 1) / CQ_BLOCK;
    long long since = 0;                                            // tiles since the last flush (block-uniform)
    for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {   // block-uniform bounds: every wave takes every ballot and barrier
        const long long i = t * CQ_BLOCK + threadIdx.x;
        const bool live = i < nf;
        long long x[2] = {0, 0};
        int ce = 0;
        if (live) {
            x[0] = pos[i] + 4;
            x[1] = x[0] + (tlen[i] - 8) - 1;
            ce = cell[i];
        }
        if (ns > 0) {
            unsigned long long n_center = 0, n_flank = 0;
            for (int k = 0; k < 2; ++k) {
                long long lo = 0, n = 0;
                if (live) {
                    lo = cq_lower(sc, 0, ns, x[k] - flank);
                    const long long hi = cq_upper(sc, lo, ns, x[k] + flank);
                    n = hi - lo;
                    if (n > 0) {
                        n_center += (unsigned long long)(cq_upper(sc, lo, hi, x[k] + center) - cq_lower(sc, lo, hi, x[k] - center));
                        n_flank += (unsigned long long)(n - (cq_upper(sc, lo, hi, x[k] + inner) - cq_lower(sc, lo, hi, x[k] - inner)));
                    }
                }
                cq_profile_pairs(s_prof, sc, sm, flank, x[k], lo, n, lane);
            }
            if (n_center) atomicAdd(&tss_center[ce], n_center);
            if (n_flank) atomicAdd(&tss_flank[ce], n_flank);
            if (++since == flush_tiles) {
                cq_flush(s_prof, K, profile);
                since = 0;
            }
        }
        if (np > 0 && live && (cq_in_peaks(ps, pe, np, x[0]) || cq_in_peaks(ps, pe, np, x[1]))) atomicAdd(&in_peaks[ce], 1ULL);
    }
    if (ns > 0 && since) cq_flush(s_prof, K, profile);
}

}  // namespace natac_cellqc

// ---- entry point -----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_cell_site_qc(natac_ctx *c, int64_t nf, const int64_t *pos, const int64_t *tlen, const int32_t *cell, int32_t n_cells, int64_t ns,
                       const int64_t *site_center, const uint8_t *site_minus, int flank, int center, int edge, int64_t np,
                       const int64_t *peak_start, const int64_t *peak_end, int64_t *tss_center, int64_t *tss_flank, int64_t *in_peaks,
                       int64_t *profile, double *kernel_ms) {
    using namespace natac_cellqc;
    static_assert(CQ_MAX_FLANK == NATAC_CELLQC_MAX_FLANK && CQ_BLOCK == NATAC_CELLQC_BLOCK && CQ_LANE_MAX == NATAC_CELLQC_LANE_MAX &&
                      CQ_MAX_BLOCKS == NATAC_CELLQC_MAX_BLOCKS && CQ_SITE_CHUNK == NATAC_CELLQC_SITE_CHUNK,
                  "the kernel's sizes are in natac.h");
    static_assert(2ULL * CQ_BLOCK * CQ_SITE_CHUNK <= 0xffffffffULL, "a tile's pairs fit a 32-bit counter");
    static_assert((2 * CQ_MAX_FLANK + 1) * sizeof(unsigned) * 8 <= 160 * 1024, "eight workgroups' profiles fit the LDS of a CU");
    if (!c || !tss_center || !tss_flank || !in_peaks || !profile) return fail(NATAC_E_ARG, "null argument");
    if (nf < 0 || ns < 0 || np < 0) return fail(NATAC_E_ARG, "negative size");
    if ((nf > 0 && (!pos || !tlen || !cell)) || (ns > 0 && !site_center) || (np > 0 && (!peak_start || !peak_end)))
        return fail(NATAC_E_ARG, "null argument");
    if (flank < 1 || flank > NATAC_CELLQC_MAX_FLANK) return fail(NATAC_E_ARG, "flank must be in [1, %d] (got %d)", NATAC_CELLQC_MAX_FLANK, flank);
    if (center < 0 || edge < 1 || (long long)center + edge > flank)
        return fail(NATAC_E_ARG, "0 <= center, 1 <= edge and center + edge <= flank must hold (got center %d, edge %d, flank %d)", center, edge,
                    flank);
    if (n_cells < 1 || n_cells > NATAC_SPLIT_MAX_BARCODES) return fail(NATAC_E_ARG, "n_cells must be in [1, %d] (got %d)", NATAC_SPLIT_MAX_BARCODES, n_cells);
    if (nf >= (1LL << 40) || ns >= (1LL << 40) || np >= (1LL << 40)) return fail(NATAC_E_ARG, "too many records, sites or peaks in one call");
    // the kernel searches the two tables and indexes counters by cell and by d + flank: all of that is checked here
    if (const int rc = check_fragments(nf, pos, tlen, cell, n_cells)) return rc;
    if (const int rc = check_site_centres(ns, site_center)) return rc;
    if (const int rc = check_intervals("peak", np, peak_start, peak_end, true)) return rc;
    const int K = 2 * flank + 1;
    if (kernel_ms) *kernel_ms = 0;       // behind the checks: a refused call leaves every output as it was
    for (int32_t i = 0; i < n_cells; ++i) tss_center[i] = tss_flank[i] = in_peaks[i] = 0;
    for (int i = 0; i < K; ++i) profile[i] = 0;
    if (nf == 0 || (ns == 0 && np == 0)) return NATAC_OK;
    DeviceCall dc(c, "cell_site_qc");
    const long long *d_pos = dc.upload((const long long *)pos, (size_t)nf), *d_tlen = dc.upload((const long long *)tlen, (size_t)nf);
    const int *d_cell = dc.upload((const int *)cell, (size_t)nf);
    const long long *d_sc = ns ? dc.upload((const long long *)site_center, (size_t)ns) : nullptr;
    const unsigned char *d_sm = ns && site_minus ? dc.upload((const unsigned char *)site_minus, (size_t)ns) : nullptr;
    const long long *d_ps = np ? dc.upload((const long long *)peak_start, (size_t)np) : nullptr;
    const long long *d_pe = np ? dc.upload((const long long *)peak_end, (size_t)np) : nullptr;
    const size_t n_out = 3 * (size_t)n_cells + (size_t)K;          // tss_center, tss_flank, in_peaks, profile
    unsigned long long *d_out = dc.zeroed<unsigned long long>(n_out);
    const long long n_tiles = (nf + CQ_BLOCK - 1) / CQ_BLOCK;
    const unsigned bx = (unsigned)std::min<long long>(n_tiles, CQ_MAX_BLOCKS);
    dc.time_begin(kernel_ms);
    for (long long s0 = 0; s0 == 0 || s0 < ns; s0 += CQ_SITE_CHUNK) {      // the peaks go with the first launch
        if (!dc.ok()) break;
        const long long n = std::min<long long>(ns - s0, CQ_SITE_CHUNK);
        const long long flush_tiles = n ? std::max<long long>(1, (long long)(0xffffffffULL / (2ULL * CQ_BLOCK * (unsigned long long)n))) : 1;
        hipLaunchKernelGGL(cq_count, dim3(bx), dim3(CQ_BLOCK), (size_t)K * sizeof(unsigned), c->stream, d_pos, d_tlen, d_cell, (long long)nf,
                           (int)n_cells, d_sc ? d_sc + s0 : nullptr, d_sm ? d_sm + s0 : nullptr, n, flank, center, edge, d_ps, d_pe,
                           s0 == 0 ? (long long)np : 0LL, flush_tiles, d_out);
        dc.launched();
    }
    dc.time_end();
    dc.fetch(tss_center, d_out, (size_t)n_cells);
    dc.fetch(tss_flank, d_out + n_cells, (size_t)n_cells);
    dc.fetch(in_peaks, d_out + 2 * (size_t)n_cells, (size_t)n_cells);
    dc.fetch(profile, d_out + 3 * (size_t)n_cells, (size_t)K);
    return dc.finish();
}

}  // extern "C"
