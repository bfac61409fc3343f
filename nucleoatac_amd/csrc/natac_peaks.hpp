// natac_peaks.hpp -- the device peak search (utils.call_peaks per chunk) as one unit: the launch plan that the host dispatcher, the
// kernels and natac_peaks_plan all read, the kernels, the occupancy peak tail (K9), and peaks_enqueue, which launches a planned search.
// What belongs to the batch (jitter, slot and candidate buffers, statistics, state flags) stays in natac_api.hip, run_peaks_impl.
#pragma once
#include "natac_kernels.hpp"
#include "natac_runtime.hpp"

#include <utility>

namespace natac {

// ------------------------------------------------------------------------------------------------
// K8  candidate search on the device: utils.call_peaks (pyatac/utils.py:82-102) applied to norm + smoothed signal as in
// NucChunk.findAllNucs (nucleoatac/NucleosomeCalling.py:297-301).
//   1. NaNs of the combined signal are replaced by the chunk's minimum finite value (all-NaN chunk: no candidates);
//   2. local maxima: y[g] > y[clip(g +- s)] for s = 1..order on the jittered signal y = x * (1 + u[g]); u is the host
//      generated RandomState(25).uniform(0, 1e-12) stream of the reference (same tie-break, bit for bit);
//   3. x[g] >= min_signal, boundary <= g < L - boundary;
//   4. reduce_peaks: visit peaks by decreasing x, keep a peak and drop every peak closer than `sep` (utils.py:56-78).
// ------------------------------------------------------------------------------------------------
constexpr int PEAK_MAX = 2048;   // local maxima per chunk held in LDS.  natac_peaks_chunk (chunks longer than 16,384 bases) keeps the lists of a
                                 // chunk with more in global scratch; the register variants set status bit 1 (host fallback)
constexpr int PK_SM_H = 30;      // half window of the smoothing a register variant can fuse (the cli's smooth_sd = 10)

// ---- the launch plan: which kernel a batch takes, from its longest chunk (maxL) and `order`.  One statement of every edge; the host
// reads peaks_plan(), the register kernel calls the same functions with its NJ and NW.
constexpr int PK_REG_MAX_NJ = 16;                    // bases per thread of a register variant: NJ 1..16 at 256 threads (up to 4,096 bases) ...
constexpr int PK_REG1K_MIN_NJ = 256 * PK_REG_MAX_NJ / 1024 + 1;   // ... and 5..16 at 1,024 threads (up to 16,384)
constexpr int PK_REG_MAX_LDS = 150 * 1024;           // dynamic LDS a 1,024-thread variant may ask for (gfx950: 160 KB per workgroup)
constexpr int PK_SEG = 4096;                         // bases per segment of natac_peaks_chunk (16 rows of 256)
constexpr int PK_LIST_MIN = 2 * 128;                 // bytes of survivor list below which two phases do not pay

// slots of a chunk's LDS lists (sig, pos, state)
__host__ __device__ constexpr int peaks_list_cap(int maxL, int order) {
    const int m = maxL / (order + 1) + 2;            // a chunk of L bases holds at most L / (order + 1) + 1 maxima
    return ((m < PEAK_MAX ? m : PEAK_MAX) + 7) & ~7;
}
// ... their bytes: 13 per slot.  Before the lists are in use the register kernel cuts the region into one share per wave (8-byte aligned)
__host__ __device__ constexpr int peaks_list_region(int pk_cap) { return pk_cap * (int)(sizeof(double) + sizeof(int) + 1); }
__host__ __device__ constexpr int peaks_wave_stride(int region, int nw) { return (region / nw) & ~7; }
// ... which holds the wave's NJ row masks, or not (a large `order` shrinks the lists: maxL 4,096, order 150: 104 bytes for 128) ...
__host__ __device__ constexpr bool peaks_masks_in_registers(int stride, int nj) { return stride < nj * 8; }
// ... and behind them a survivor list, if there is room for a useful one
__host__ __device__ constexpr bool peaks_two_phase(int stride, int nj, int order) { return order > 2 && stride >= nj * 8 + PK_LIST_MIN; }
enum PeakKernel : int { PK_KERNEL_REG = 0, PK_KERNEL_SEG = 1 };
enum PeakMask : int { PK_MASK_NONE = -1, PK_MASK_REGISTERS = 0, PK_MASK_TWO_PHASE = 1, PK_MASK_DIRECT = 2 };
__host__ __device__ constexpr PeakMask peaks_mask_mode(int stride, int nj, int order) {
    return peaks_masks_in_registers(stride, nj) ? PK_MASK_REGISTERS : peaks_two_phase(stride, nj, order) ? PK_MASK_TWO_PHASE : PK_MASK_DIRECT;
}
// doubles of a register variant's LDS before the lists: BT NJ + max(2 order + 1, 2 H with the fused smoothing), even
__host__ __device__ constexpr int peaks_reg_ysn(int bt_nj, int order, bool smooth) {
    return (bt_nj + ((smooth && 2 * PK_SM_H > 2 * order + 1) ? 2 * PK_SM_H : 2 * order + 1)) & ~1;
}

struct PeakPlan {
    PeakKernel kernel;       // natac_peaks_chunk_reg<nj, bt> or the segmented natac_peaks_chunk (bt 256, nj 0, no mask mode)
    int bt, nj, pk_cap;
    PeakMask mask;
    bool global_lists;       // SEG: some chunk can hold more maxima than the LDS lists
    bool forms_smooth;       // the kernel can form a pending SMOOTH itself: <nj, 256, true>, which needs its masks in LDS
    size_t lds, lds_smooth;  // dynamic LDS bytes without and with the fused smoothing (equal where it cannot fuse)
};

// maxL >= 1, 1 <= order <= 255
__host__ __device__ constexpr PeakPlan peaks_plan(int maxL, int order) {
    PeakPlan p{};
    p.pk_cap = peaks_list_cap(maxL, order);
    const int region = peaks_list_region(p.pk_cap);
    p.bt = maxL <= 256 * PK_REG_MAX_NJ ? 256 : 1024;
    p.nj = (maxL - 1) / p.bt + 1;
    if (p.nj <= PK_REG_MAX_NJ) p.lds = (size_t)peaks_reg_ysn(p.bt * p.nj, order, false) * sizeof(double) + region;
    if (p.nj <= PK_REG_MAX_NJ && (p.bt == 256 || p.lds <= (size_t)PK_REG_MAX_LDS)) {
        p.kernel = PK_KERNEL_REG;
        p.mask = peaks_mask_mode(peaks_wave_stride(region, p.bt / 64), p.nj, order);
        p.forms_smooth = p.bt == 256 && p.mask != PK_MASK_REGISTERS;
        p.lds_smooth = p.forms_smooth ? (size_t)peaks_reg_ysn(p.bt * p.nj, order, true) * sizeof(double) + region : p.lds;
    } else {   // longer still: segments, signal read per segment
        p.kernel = PK_KERNEL_SEG;
        p.bt = 256;
        p.nj = 0;
        p.mask = PK_MASK_NONE;
        p.global_lists = maxL / (order + 1) + 2 > p.pk_cap;
        p.lds = p.lds_smooth = (size_t)((PK_SEG + 2 * order + 1) & ~1) * sizeof(double) + region;
    }
    return p;
}
// one look at each edge at compile time: the last 256-thread chunk, the first and last 1,024-thread chunks, masks that do not fit
static_assert(peaks_plan(4096, 12).bt == 256 && peaks_plan(4096, 12).nj == PK_REG_MAX_NJ && peaks_plan(4096, 12).forms_smooth &&
              peaks_plan(4097, 12).bt == 1024 && peaks_plan(4097, 12).nj == PK_REG1K_MIN_NJ && !peaks_plan(4097, 12).forms_smooth &&
              peaks_plan(16384, 12).kernel == PK_KERNEL_REG && peaks_plan(16385, 12).kernel == PK_KERNEL_SEG &&
              peaks_plan(4096, 150).mask == PK_MASK_REGISTERS && !peaks_plan(4096, 150).forms_smooth, "peak search plan");

// steps 4 + output of the peak search for one chunk (see natac_peaks_chunk): n maxima in (pos, sig, state = 0), ascending
__device__ __forceinline__ void peaks_thin_and_write(int n, int pk_cap, int sep, const double *sig, const int *pos, unsigned char *state,
                                                      int *wave_cnt, int *__restrict__ dst, int *__restrict__ count_out,
                                                      int *__restrict__ status_out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, bt = blockDim.x, nw = bt >> 6;   // wave_cnt holds nw <= 16 counts
    const bool overflow = n > pk_cap;
    if (overflow) n = pk_cap;
    // ---- 4. reduce_peaks as parallel rounds.  A kept peak (state 1) has no free peak closer than sep once its round is
    // over, so in later rounds the tests below never meet one: "free or kept" in the first pass only covers peaks that another
    // thread keeps during the same pass
    for (;;) {
        int nfree = 0;
        for (int i = threadIdx.x; i < n; i += bt) {
            if (state[i] != 0) continue;
            const double si = sig[i];
            const int pi = pos[i];
            bool top = true;
            for (int k = i - 1; top && k >= 0 && pi - pos[k] < sep; --k) top = !(state[k] <= 1 && sig[k] > si);
            for (int k = i + 1; top && k < n && pos[k] - pi < sep; ++k) top = !(state[k] <= 1 && sig[k] >= si);
            if (top) state[i] = 1; else ++nfree;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += bt) {
            if (state[i] != 0) continue;
            const int pi = pos[i];
            bool ex = false;
            for (int k = i - 1; !ex && k >= 0 && pi - pos[k] < sep; --k) ex = state[k] == 1;
            for (int k = i + 1; !ex && k < n && pos[k] - pi < sep; ++k) ex = state[k] == 1;
            if (ex) { state[i] = 2; --nfree; }
        }
        if (__syncthreads_or(nfree > 0) == 0) break;
    }
    // ---- kept positions, ascending
    int m_out = 0;
    for (int base = 0; base < n; base += bt) {
        const int i = base + threadIdx.x;
        const bool kp = i < n && state[i] == 1;
        const unsigned long long m = __ballot(kp);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = m_out;
        int tot = 0;
        for (int w = 0; w < nw; ++w) { const int cw = wave_cnt[w]; off += (w < wave) ? cw : 0; tot += cw; }
        if (kp) dst[off + __popcll(m & ((1ull << lane) - 1ull))] = pos[i];
        m_out += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *count_out = m_out;
        if (overflow) atomicOr(status_out, 2);
    }
}

// One workgroup per chunk does the whole search: minimum of the finite values, the jittered local-maximum test on
// segments of `seg` bases staged in LDS, ordered compaction of the maxima, greedy thinning, and writes the kept positions
// (ascending) into the chunk's slot region cand_slot[cap_off[chunk] ...] and their number into count[chunk].
// The thinning runs as parallel rounds: a free peak that out-ranks every free peak closer than `sep` is kept and excludes
// those neighbours -- the same set the reference's sequential visit by decreasing signal produces (a peak is only ever
// excluded by a kept peak of higher rank, and a kept peak is the highest-ranked free one of its neighbourhood at the time it
// is visited).  Rank: larger signal first, ties: the later position first (a stable ascending sort read backwards).
// Dynamic LDS: ys[seg + 2 order (even)] | sig[pk_cap] | pos[pk_cap] (int) | state[pk_cap] (bytes); seg a multiple of 256.
__global__ void __launch_bounds__(256) natac_peaks_chunk(ChunkTable ct, const double *__restrict__ norm,
                                                           const double *__restrict__ smooth, const double *__restrict__ jitter,
                                                           double min_signal, int boundary, int order, int sep, int seg, int pk_cap,
                                                           const long long *__restrict__ cap_off, int *__restrict__ cand_slot,
                                                           int *__restrict__ count, int *__restrict__ status,
                                                           double *__restrict__ big_sig, int *__restrict__ big_pos,
                                                           unsigned char *__restrict__ big_state) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double red[4];
    __shared__ int wave_cnt[16];
    __shared__ int row_cnt[4 * 16];
    const int ysn = (seg + 2 * order + 1) & ~1;
    double *ys = smem;                              // jittered signal, index u <-> base clip(x0 - order + u)
    double *sig = ys + ysn;
    int *pos = (int *)(sig + pk_cap);
    unsigned char *state = (unsigned char *)(pos + pk_cap);   // 0 free, 1 kept, 2 excluded
    const int chunk = blockIdx.x;
    {   // a chunk that can hold more maxima than the LDS lists (L / (order + 1) + 2 > pk_cap: tens of kb and more, what ChunkList.merge
        // makes of adjacent windows) keeps its lists in the global scratch, region cap_off[chunk] ...: no overflow, no host fallback
        const long long c0 = cap_off[chunk];
        const int cap_c = (int)(cap_off[chunk + 1] - c0);
        if (big_sig && cap_c > pk_cap) { sig = big_sig + c0; pos = big_pos + c0; state = big_state + c0; pk_cap = cap_c; }
    }
    const int L = ct.chunk_len[chunk];
    const long long ob = ct.out_off[chunk];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // ---- 1. minimum finite value of the combined signal
    double mn = __builtin_inf();
    for (int g0 = threadIdx.x; g0 < L; g0 += 8 * 256) {      // eight independent loads per thread in flight
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int g = g0 + 256 * q;
            v[q] = __builtin_nan("");
            if (g < L) v[q] = smooth ? norm[ob + g] + smooth[ob + g] : norm[ob + g];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (v[q] == v[q]) mn = fmin(mn, v[q]);
    }
    mn = wave_min(mn);
    if (lane == 0) red[wave] = mn;
    __syncthreads();
    const double fillv = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    if (fillv == __builtin_inf()) {                 // all-NaN chunk: nothing
        if (threadIdx.x == 0) count[chunk] = 0;
        return;
    }
    // ---- 2. + 3. local maxima of the jittered signal, thresholds, ordered compaction
    int n = 0;
    for (int x0 = 0; x0 < L; x0 += seg) {
        const int len = min(seg, L - x0);
        __syncthreads();
        for (int u0 = threadIdx.x; u0 < len + 2 * order; u0 += 8 * 256) {
            double v[8], jt[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int u = u0 + 256 * q;
                int g = x0 - order + u;
                g = g < 0 ? 0 : (g > L - 1 ? L - 1 : g);                 // numpy take(..., mode='clip')
                v[q] = smooth ? norm[ob + g] + smooth[ob + g] : norm[ob + g];
                jt[q] = jitter[g];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int u = u0 + 256 * q;
                if (u < len + 2 * order) ys[u] = ((v[q] != v[q]) ? fillv : v[q]) * (1 + jt[q]);
            }
        }
        __syncthreads();
        // the segment's <= 16 rows of 256 bases: local-maximum tests first, then the un-jittered values of the maxima (all
        // loads of a thread in flight), thresholds, and one ordered compaction for all rows
        unsigned pkf = 0;
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int t = 256 * it + threadIdx.x;
            bool pk = t < len;
            if (pk) {
                const double y = ys[t + order];
                for (int sft = 1; sft <= order && pk; ++sft) pk = (y > ys[t + order + sft]) && (y > ys[t + order - sft]);
            }
            pkf |= pk ? (1u << it) : 0u;
        }
        double v[16];
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int g = x0 + 256 * it + threadIdx.x;
            v[it] = 0.0;
            if (pkf & (1u << it)) v[it] = smooth ? norm[ob + g] + smooth[ob + g] : norm[ob + g];
        }
        unsigned long long bal[16];
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int g = x0 + 256 * it + threadIdx.x;
            if (v[it] != v[it]) v[it] = fillv;
            const bool pk = (pkf & (1u << it)) && (v[it] >= min_signal) && (g >= boundary) && (g < L - boundary);
            bal[it] = __ballot(pk);
            if (lane == 0) row_cnt[it * 4 + wave] = __popcll(bal[it]);
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            int off = n;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int cw = row_cnt[it * 4 + w];
                off += (w < wave) ? cw : 0;
                n += cw;
            }
            if ((bal[it] >> lane) & 1ull) {
                const int i = off + __popcll(bal[it] & ((1ull << lane) - 1ull));
                if (i < pk_cap) { pos[i] = x0 + 256 * it + threadIdx.x; sig[i] = v[it]; state[i] = 0; }
            }
        }
    }
    __syncthreads();
    peaks_thin_and_write(n, pk_cap, sep, sig, pos, state, wave_cnt, cand_slot + cap_off[chunk], count + chunk, status + chunk);
}

// The same search for batches whose chunks all fit one segment (L <= BT NJ; BT = 256 threads, or 1,024 for chunks up to 16,384
// bases: gfx950 gives a workgroup up to 160 KB of LDS): every thread keeps its NJ bases in registers,
// so the signal is read from memory once, with all loads of a thread in flight together (the general kernel above walks
// the chunk three times with one dependent load per iteration).  LDS as above with seg = 256 NJ.
//
// SMOOTH: the second signal does not exist yet -- it is natac_smooth_same<true> of `norm` for the window M = 2 PK_SM_H + 1, and this
// workgroup forms it (it holds the whole chunk anyway), writes it to smooth_out and searches norm + that: one read of norm and one write
// of the smoothed track instead of a smoothing kernel's read + write and two more reads here.  Same bits as natac_smooth_same:
//   numerators   a thread takes NJ consecutive bases and slides over their NJ + 2 H inputs (clamped, NaN and beyond-the-chunk -> 0, staged
//                where the jittered signal goes later), descending, so every output adds its taps in ascending n;
//   denominators per base, after the numerators went through LDS back to the search's layout (lane = base: coalesced stores): which of
//                a base's 2 H + 1 inputs hold a number is a bit field cut from the chunk's validity mask (ballots of the staging loop).
//                All of them (a wave sees that for its 64 bases of a row in three words of the mask): the host-formed win_sum.  Only a
//                chunk end missing: the host-formed sum of the taps that are left, win[M ..] / win[2 M ..] (ensure_window), one load.
//                Else (a NaN under the window) the fma sum over the set bits.  The first cut ran that 61-trip loop for the 60 bases
//                at a chunk's ends too, with a vector load per trip inside a divergent branch: 1.1 ms per step, the whole gain.
// LDS: BT NJ + max(2 order + 1, 2 H) doubles (even) before the lists.
template <int NJ, int BT, bool SMOOTH = false>
__global__ void __launch_bounds__(BT) natac_peaks_chunk_reg(ChunkTable ct, const double *__restrict__ norm,
                                                               const double *__restrict__ smooth, const double *__restrict__ jitter,
                                                               double min_signal, int boundary, int order, int sep, int pk_cap,
                                                               const long long *__restrict__ cap_off, int *__restrict__ cand_slot,
                                                               int *__restrict__ count, int *__restrict__ status,
                                                               const double *__restrict__ win, double win_sum,
                                                               double *__restrict__ smooth_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    constexpr int NW = BT / 64;
    __shared__ double red[NW];
    __shared__ int wave_cnt[16];
    __shared__ int row_cnt[NW * NJ];
    const int ysn = peaks_reg_ysn(BT * NJ, order, SMOOTH);
    double *ys = smem;                              // jittered signal, index u <-> base clip(u - order)
    double *sig = ys + ysn;
    int *pos = (int *)(sig + pk_cap);
    unsigned char *state = (unsigned char *)(pos + pk_cap);
    const int chunk = blockIdx.x;
    const int L = ct.chunk_len[chunk];
    const long long ob = ct.out_off[chunk];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double v[NJ], jt[NJ];
    if constexpr (SMOOTH) {
        constexpr int H = PK_SM_H, M = 2 * H + 1;
        static_assert(BT >= 2 * H && M < 64, "the halo is zeroed by one pass of the workgroup; a window's validity bits fit one word");
        __shared__ unsigned long long okb[NW * NJ + 2];   // bit b & 63 of word 1 + (b >> 6): base b holds a number; first and last word: none do
        double *xs = smem;                          // index u <-> base u - H; after the numerators are formed: their exchange, index = base
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int g = threadIdx.x + BT * j;
            double x = __builtin_nan("");
            if (g < L) x = norm[ob + g];
            v[j] = x;
            const bool okv = x == x;
            xs[H + g] = okv ? (x < 0 ? 0.0 : x) : 0.0;
            const unsigned long long m = __ballot(okv);
            if (lane == 0) okb[1 + NW * j + wave] = m;
        }
        if (threadIdx.x < 2 * H) xs[threadIdx.x < H ? threadIdx.x : BT * NJ + threadIdx.x] = 0.0;
        if (threadIdx.x == 0) { okb[0] = 0ull; okb[NW * NJ + 1] = 0ull; }
        __syncthreads();
        const int g0 = threadIdx.x * NJ;
        double num[NJ];
#pragma unroll
        for (int o = 0; o < NJ; ++o) num[o] = 0.0;
        if (g0 < L) {
            // the window values are wave-uniform: scalar loads, SGPR operands of the FMAs
#pragma unroll
            for (int kk = 0; kk < 2 * H + NJ; ++kk) {
                const int k = 2 * H + NJ - 1 - kk;          // inputs in descending order = taps n ascending for every output
                const double r = xs[g0 + k];
#pragma unroll
                for (int o = 0; o < NJ; ++o) {
                    const int n = o + 2 * H - k;
                    if (n >= 0 && n < M) num[o] = fma(win[n], r, num[o]);
                }
            }
        }
        __syncthreads();
        if (g0 < L) {
#pragma unroll
            for (int o = 0; o < NJ; ++o) xs[g0 + o] = num[o];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int g = threadIdx.x + BT * j;
            const bool in = g < L;
            jt[j] = 0.0;
            if (in) jt[j] = jitter[g];
            double den = win_sum;
            // the windows of this wave's 64 bases of the row lie in three words of the mask: all set (most rows of most chunks),
            // every denominator is win_sum
            const int iw = NW * j + wave;
            constexpr unsigned long long HM = (1ull << H) - 1ull;
            const bool clean = (okb[iw] >> (64 - H)) == HM && okb[iw + 1] == ~0ull && (okb[iw + 2] & HM) == HM;
            if (__ballot(!clean) != 0ull) {
                constexpr unsigned long long FULL = (1ull << M) - 1ull;
                const int p = g - H + 64, i = p >> 6, sh = p & 63;
                unsigned long long f = okb[i] >> sh;
                if (sh) f |= okb[i + 1] << (64 - sh);
                f &= FULL;                              // bit q <-> base g - H + q <-> tap n = 2 H - q
                bool generic = false;
                if (in && f != FULL) {
                    // a chunk end under the window and nothing else: the taps are n = 0 .. 2 H - k (the k bases before the chunk are
                    // missing) or n = k .. 2 H (the k after it): the host-formed sums of exactly those, win[M + .] and win[2 M + .]
                    const int lo = __builtin_ctzll(f | (1ull << M)), hi = __builtin_clzll(f | 1ull) - (64 - M);
                    if (f == 0ull) den = 0.0;
                    else if (f == ((FULL >> lo) << lo)) den = win[M + 2 * H - lo];
                    else if (f == (FULL >> hi)) den = win[2 * M + hi];
                    else generic = true;
                }
                if (__ballot(generic) != 0ull) {        // a NaN under a window.  Wave-uniform branch: the window values stay scalar loads
                    double d = 0.0;
#pragma unroll 8
                    for (int n = 0; n < M; ++n) {
                        const double wv = win[n];
                        if ((f >> (2 * H - n)) & 1ull) d = fma(wv, 1.0, d);
                    }
                    if (generic) den = d;
                }
            }
            if (in) {
                const double s = (den == 0.0) ? __builtin_nan("") : xs[g] / den;
                smooth_out[ob + g] = s;
                v[j] += s;
            }
        }
    } else {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int g = threadIdx.x + BT * j;
        v[j] = __builtin_nan("");
        jt[j] = 0.0;
        if (g < L) {
            v[j] = smooth ? norm[ob + g] + smooth[ob + g] : norm[ob + g];
            jt[j] = jitter[g];
        }
    }
    }
    double mn = __builtin_inf();
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        if (v[j] == v[j]) mn = fmin(mn, v[j]);
    mn = wave_min(mn);
    if (lane == 0) red[wave] = mn;
    __syncthreads();
    double fillv = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) fillv = fmin(fillv, red[w]);
    if (fillv == __builtin_inf()) {                 // all-NaN chunk: nothing
        if (threadIdx.x == 0) count[chunk] = 0;
        return;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int g = threadIdx.x + BT * j;
        if (v[j] != v[j]) v[j] = fillv;
        if (g < L) {
            const double y = v[j] * (1 + jt[j]);
            ys[order + g] = y;
            if (g == 0)
                for (int u = 0; u < order; ++u) ys[u] = y;                 // numpy take(..., mode='clip')
            if (g == L - 1)
                for (int u = 0; u < order; ++u) ys[order + L + u] = y;
        }
    }
    __syncthreads();
    // maxima of the thread's bases, then one ordered compaction for all NJ rows (base order = row-major over (j, thread)).
    // The test "larger than both neighbours at every distance up to `order`" leaves a lane after 1.5 comparisons on average, but a wave
    // only when its last lane leaves -- and among 64 consecutive bases one nearly always stays to the end, so every row cost `order`
    // trips.  Two phases (round 5): distances 1 and 2 for every base (thresholds first), the survivors -- about a fifth -- go into a
    // per-wave list, and the remaining distances run over that dense list, 64 candidates at a time; the rows' masks are put back
    // together in LDS.  The list lives where the chunk's peak lists go afterwards (not in use yet).
    unsigned long long bal[NJ];
    {
        const int stride = peaks_wave_stride(peaks_list_region(pk_cap), NW);
        unsigned long long *wmask = (unsigned long long *)((unsigned char *)sig + wave * stride);     // [NJ] survivors of row j
        unsigned short *wlist = (unsigned short *)(wmask + NJ);
        const int cap = (stride - NJ * 8) / 2;
        const bool two_phase = peaks_two_phase(stride, NJ, order);          // room for a useful list (else: the direct test below)
        if (peaks_masks_in_registers(stride, NJ)) {
            // a large `order` shrinks the peak lists (pk_cap = maxL / (order + 1)) below even the NJ masks of a wave: the masks then
            // stay in registers, every row takes the direct test
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int g = threadIdx.x + BT * j;
                bool pk = g < L && (v[j] >= min_signal) && (g >= boundary) && (g < L - boundary);
                if (pk) {
                    const double y = ys[g + order];
                    for (int sft = 1; sft <= order && pk; ++sft) pk = (y > ys[g + order + sft]) && (y > ys[g + order - sft]);
                }
                bal[j] = __ballot(pk);
                if (lane == 0) row_cnt[j * NW + wave] = __popcll(bal[j]);
            }
        } else {
        if (lane < NJ) wmask[lane] = 0ull;
        __builtin_amdgcn_wave_barrier();
        int cnt = 0;
        const int o1 = order < 2 ? order : 2;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int g = threadIdx.x + BT * j;
            bool pk = g < L && (v[j] >= min_signal) && (g >= boundary) && (g < L - boundary);
            double y = 0.0;
            if (pk) {
                y = ys[g + order];
                for (int sft = 1; sft <= o1 && pk; ++sft) pk = (y > ys[g + order + sft]) && (y > ys[g + order - sft]);
            }
            const unsigned long long m = __ballot(pk);
            const int alive = __popcll(m);
            if (two_phase && cnt + alive <= cap) {                      // wave-uniform
                if (pk) wlist[cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                            (unsigned short)(j * 64 + lane);
                cnt += alive;
            } else {                                                    // no list (or full): finish the row here
                if (pk)
                    for (int sft = o1 + 1; sft <= order && pk; ++sft) pk = (y > ys[g + order + sft]) && (y > ys[g + order - sft]);
                const unsigned long long mf = __ballot(pk);
                if (lane == 0) wmask[j] = mf;
            }
        }
        __builtin_amdgcn_wave_barrier();
        unsigned int *wm32 = (unsigned int *)wmask;
        for (int idx = lane; idx - lane < cnt; idx += 64) {             // wave-uniform trip count
            if (idx < cnt) {
                const int e = wlist[idx], jj = e >> 6, ll = e & 63;
                const int g = (wave << 6) + ll + BT * jj;
                const double y = ys[g + order];
                bool pk = true;
                for (int sft = 3; sft <= order && pk; ++sft) pk = (y > ys[g + order + sft]) && (y > ys[g + order - sft]);
                if (pk) atomicOr(&wm32[2 * jj + (ll >> 5)], 1u << (ll & 31));
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            bal[j] = wmask[j];
            if (lane == 0) row_cnt[j * NW + wave] = __popcll(bal[j]);
        }
        }
    }
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        int off = n;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int cw = row_cnt[j * NW + w];
            off += (w < wave) ? cw : 0;
            n += cw;
        }
        if ((bal[j] >> lane) & 1ull) {
            const int i = off + __popcll(bal[j] & ((1ull << lane) - 1ull));
            if (i < pk_cap) { pos[i] = threadIdx.x + BT * j; sig[i] = v[j]; state[i] = 0; }
        }
    }
    __syncthreads();
    peaks_thin_and_write(n, pk_cap, sep, sig, pos, state, wave_cnt, cand_slot + cap_off[chunk], count + chunk, status + chunk);
}

// exclusive prefix sum of per-chunk counts (single workgroup) + total: tiles of 4,096 counts, four consecutive ones per thread
// (coalesced), wave scans by shuffles, the 16 wave totals through LDS, a running carry between tiles
__global__ void __launch_bounds__(1024) natac_scan_counts(const int *__restrict__ count, int nc, long long *__restrict__ offs) {
    __shared__ long long wtot[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long carry = 0;
    for (int base = 0; base < nc; base += 4096) {
        const int i0 = base + 4 * t;
        int c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = (i0 + q < nc) ? count[i0 + q] : 0;
        const long long mine = (long long)c[0] + c[1] + c[2] + c[3];
        long long incl = mine;                               // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        long long before = carry, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const long long v = wtot[w];
            before += (w < wave) ? v : 0;
            total += v;
        }
        long long run = before + incl - mine;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (i0 + q < nc) offs[i0 + q] = run;
            run += c[q];
        }
        carry += total;
        __syncthreads();
    }
    if (t == 0) offs[nc] = carry;
}

__global__ void __launch_bounds__(256) natac_compact_candidates(int nc, const int *__restrict__ count,
                                                                  const long long *__restrict__ offs,
                                                                  const long long *__restrict__ cap_off,
                                                                  const int *__restrict__ cand_slot, int *__restrict__ cand_chunk,
                                                                  int *__restrict__ cand_pos) {
    const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nc) return;
    const int lane = threadIdx.x & 63;
    const int n = count[chunk];
    const long long o = offs[chunk];
    const int *src = cand_slot + cap_off[chunk];
    for (int i = lane; i < n; i += 64) { cand_chunk[o + i] = chunk; cand_pos[o + i] = src[i]; }
}

// ------------------------------------------------------------------------------------------------
// K9  OccChunk.callPeaks filter + OccChunk.getNucDist on the device (nucleoatac/Occupancy.py:225-240).
// One workgroup per chunk walks the chunk's occupancy peaks (ascending, as call_peaks returns them): a peak is kept if
// smoothed_lower[pos] > min_occ and cov[pos] > 0 (:229-230); every kept peak adds its window's insert-size histogram
// (fragments centred within +-flank, sizes [0, upper)) divided by its total to the chunk's nuc_dist, in peak order like
// the reference's `nuc_dist += sub_sum` (:236-239).  out_vals[4][n] = occ, lower, upper, reads of every peak (OccPeak).
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) natac_occ_peak_dist(ChunkTable ct, const long long *__restrict__ pk_offs,
                                                             const int *__restrict__ pk_pos, const double *__restrict__ occ,
                                                             const double *__restrict__ lower, const double *__restrict__ upper_t,
                                                             const double *__restrict__ cov, double min_occ, int flank, int U,
                                                             long long cap, double *__restrict__ out_vals,
                                                             int *__restrict__ keep, double *__restrict__ nuc_dist) {
    extern __shared__ int hist_s[];                 // [U]
    __shared__ int total_s;
    const int chunk = blockIdx.x;
    const long long ob = ct.out_off[chunk];
    const int nfr = (int)(ct.frag_off[chunk + 1] - ct.frag_off[chunk]);
    const int *cen = ct.centre + ct.frag_off[chunk];
    const int *iln = ct.ilen + ct.frag_off[chunk];
    const int nj = (U + 255) / 256;                 // insert sizes per thread (1 for upper <= 256)
    double nd[4] = {0.0, 0.0, 0.0, 0.0};            // thread t owns sizes t, t + 256, ... (U <= 1024)
    for (long long k = pk_offs[chunk]; k < pk_offs[chunk + 1]; ++k) {
        const int p = pk_pos[k];
        const double lo = lower[ob + p], rd = cov[ob + p];
        const bool kp = lo > min_occ && rd > 0;      // block-uniform
        if (threadIdx.x == 0) {
            out_vals[k] = occ[ob + p];
            out_vals[cap + k] = lo;
            out_vals[2 * cap + k] = upper_t[ob + p];
            out_vals[3 * cap + k] = rd;
            keep[k] = kp ? 1 : 0;
        }
        if (!kp) continue;
        for (int j = threadIdx.x; j < U; j += 256) hist_s[j] = 0;
        if (threadIdx.x == 0) total_s = 0;
        __syncthreads();
        const int f0 = lower_bound_i32(cen, 0, nfr, p - flank);
        const int f1 = lower_bound_i32(cen, f0, nfr, p + flank + 1);
        int mine = 0;
        for (int f = f0 + threadIdx.x; f < f1; f += 256) {
            const int n = iln[f];
            if (n >= 0 && n < U) { atomicAdd(&hist_s[n], 1); ++mine; }
        }
        if (mine) atomicAdd(&total_s, mine);
        __syncthreads();
        const double tot = (double)total_s;
        for (int q = 0; q < nj && q < 4; ++q) {
            const int j = threadIdx.x + 256 * q;
            if (j < U) nd[q] = nd[q] + (double)hist_s[j] / tot;
        }
        __syncthreads();
    }
    for (int q = 0; q < nj && q < 4; ++q) {
        const int j = threadIdx.x + 256 * q;
        if (j < U) nuc_dist[(long long)chunk * U + j] = nd[q];
    }
}

// ---- host: launching a planned search
using PeaksRegFn = decltype(&natac_peaks_chunk_reg<1, 256, false>);
template <int BT, bool SMOOTH, int NJ0, int... I>
static PeaksRegFn peaks_reg_instance(int nj, std::integer_sequence<int, I...>) {
    static const PeaksRegFn table[] = {natac_peaks_chunk_reg<NJ0 + I, BT, SMOOTH>...};
    return table[nj - NJ0];
}
// the instances there are: NJ 1..16 at 256 threads, with and without the fused smoothing, and 5..16 at 1,024 without
static PeaksRegFn peaks_reg_kernel(int bt, int nj, bool smooth) {
    using At256 = std::make_integer_sequence<int, PK_REG_MAX_NJ>;
    using At1024 = std::make_integer_sequence<int, PK_REG_MAX_NJ - PK_REG1K_MIN_NJ + 1>;
    if (bt == 256) return smooth ? peaks_reg_instance<256, true, 1>(nj, At256{}) : peaks_reg_instance<256, false, 1>(nj, At256{});
    return peaks_reg_instance<1024, false, PK_REG1K_MIN_NJ>(nj, At1024{});
}

struct PeakSearch {          // the device operands of one search over the nc chunks of ct
    const double *norm, *smooth;      // the signal is norm (+ smooth if not null)
    const double *jitter;
    double min_signal;
    int boundary, order, sep;
    const long long *cap_off;         // [nc + 1] slot regions
    int *slot, *count, *status;
    long long *offs;                  // [nc + 1] exclusive scan of count + total
    const double *win;                // the smoothing window and where the formed track goes: only with smooth_out
    double win_sum;
    double *smooth_out;               // not null: form SMOOTH from norm (p.forms_smooth must hold) and search norm + that
    double *big_sig;                  // global lists (p.global_lists), else null
    int *big_pos;
    unsigned char *big_state;
};

// Enqueues on st: the status clear (bit 1 of the status words belongs to the peak search: it describes this one), the kernel of plan p
// -- one workgroup per chunk: LDS = the jittered signal (or a segment of it) + the chunk's list of maxima -- and the scan of the counts.
static int peaks_enqueue(const PeakPlan &p, const ChunkTable &ct, int nc, const PeakSearch &s, hipStream_t st) {
    hipLaunchKernelGGL(natac_status_clear, dim3((nc + 255) / 256), dim3(256), 0, st, s.status, nc, 2);
    if (p.kernel == PK_KERNEL_REG) {
        const bool form_smooth = s.smooth_out != nullptr;
        if (form_smooth && !p.forms_smooth) return fail(NATAC_E_STATE, "peak search: this arm cannot form the smoothed track");
        const size_t lds = form_smooth ? p.lds_smooth : p.lds;
        const PeaksRegFn kfn = peaks_reg_kernel(p.bt, p.nj, form_smooth);
        if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kfn, dim3(nc), dim3(p.bt), lds, st, ct, s.norm, form_smooth ? nullptr : s.smooth, s.jitter, s.min_signal,
                           s.boundary, s.order, s.sep, p.pk_cap, s.cap_off, s.slot, s.count, s.status, s.win, s.win_sum, s.smooth_out);
    } else {
        hipLaunchKernelGGL(natac_peaks_chunk, dim3(nc), dim3(p.bt), p.lds, st, ct, s.norm, s.smooth, s.jitter, s.min_signal, s.boundary,
                           s.order, s.sep, PK_SEG, p.pk_cap, s.cap_off, s.slot, s.count, s.status, s.big_sig, s.big_pos, s.big_state);
    }
    hipLaunchKernelGGL(natac_scan_counts, dim3(1), dim3(1024), 0, st, s.count, nc, s.offs);
    return NATAC_OK;
}

}  // namespace natac
