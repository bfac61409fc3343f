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
#pragma once
#include <hip/hip_runtime.h>

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
