// natac_pwmfit.hpp -- the two counting kernels behind `pyatac pwm` (pyatac/get_pwm.py of the reference):
//   natac_ins_seq_counts  the base content of the (2*flank + 1)-base window around every Tn5 insertion of a chunk list
//                         (InsertionTrack.getInsertionSequences / getStrandedInsertionSequences, pyatac/tracks.py:179-201, summed over
//                         the chunks by _pwmHelper, get_pwm.py:21-40)
//   natac_base_count      A / C / G / T counts over byte ranges (the numerators of seq.getNucFreqs / getNucFreqsFromChunkList,
//                         pyatac/seq.py:47-72)
// Every count is an integer: the kernels add in registers and LDS as 32-bit, and every block adds its totals to the int64 result with
// one atomic per counter, so the result is exact and does not depend on the order of the fragments, the blocks or the waves.
// Behind the kernels: their entry points (natac_insertion_seq_counts, natac_base_counts).
#pragma once
#include <hip/hip_runtime.h>

#include "natac_runtime.hpp"

namespace natac_pwmfit {

constexpr int PF_MAX_FLANK = 1000;      // K = 2 * flank + 1 <= 2001 columns
constexpr int PF_BLOCK = 256;           // 4 waves
constexpr int PF_SEG = 1024;            // fragments per wave segment (one chunk lookup per lane and segment)
constexpr int PF_SPAN = PF_BLOCK * 16;  // bases per block step of natac_base_count

// row of a base in the A C G T matrix; 4 = counts in no row (N and anything else).  Lower case counts like upper case (the reference
// upper-cases every sequence it reads, pyatac/seq.py:21, 55, 67).
__device__ __forceinline__ unsigned base_row(unsigned ch) {
    ch &= 0xDFu;
    return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
}

// Window counts M[4][K] and the insertion count n of a packed chunk list (csr layout of natac_pack_chunks: lpos relative to the chunk
// start with the ATAC shift applied, ilen the insert size).  seq[seq_off[k] ..) holds the bases of [start_k - flank, end_k + flank).
// A fragment is kept if lower <= ilen < upper; its left end l and its right end r = l + ilen - 1 each count if they lie in [0, L_k).
//   sym:   an end at p adds row(seq[p + j]) to column j (both ends)
//   !sym:  left ends as above; a right end at p adds the complement of seq[p + 2*flank - j] to column j
// Lane layout: a wave is NG groups of CW lanes (CW = min(K, 64), NG = 64 / CW); the group takes one fragment at a time and lane c of it
// owns column tile * CW + c, so the K bases of a window are read by consecutive lanes from consecutive addresses and every lane counts
// into its own four registers -- no lane ever adds to a counter another lane of the wave adds to.  blockIdx.y = the column tile.
__global__ void __launch_bounds__(PF_BLOCK) natac_ins_seq_counts(const long long *__restrict__ frag_off, const int *__restrict__ lpos,
                                                                 const int *__restrict__ ilen, long long nf, int nc,
                                                                 const int *__restrict__ chunk_len, const long long *__restrict__ seq_off,
                                                                 const unsigned char *__restrict__ seq, int flank, int lower, int upper,
                                                                 int sym, unsigned long long *__restrict__ counts,
                                                                 unsigned long long *__restrict__ n_ins) {
    __shared__ unsigned s_cnt[4 * 64];
    __shared__ unsigned s_n;
    const int K = 2 * flank + 1;
    const int CW = K < 64 ? K : 64;
    const int NG = 64 / CW;
    const int lane = threadIdx.x & 63;
    const int g = lane / CW, c = lane - g * CW;
    const int tile = blockIdx.y;
    const int j = tile * CW + c;                 // this lane's column
    const bool col_ok = g < NG && j < K;
    const bool counts_n = g < NG && tile == 0 && c == 0;   // one lane per group counts insertions
    for (int i = threadIdx.x; i < 4 * 64; i += PF_BLOCK) s_cnt[i] = 0;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();

    unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0, an = 0;
    const long long nseg = (nf + PF_SEG - 1) / PF_SEG;
    const long long nwaves = (long long)gridDim.x * (PF_BLOCK / 64);
    const long long wave = (long long)blockIdx.x * (PF_BLOCK / 64) + (threadIdx.x >> 6);
    if (g < NG) {
        for (long long s = wave; s < nseg; s += nwaves) {
            const long long f0 = s * PF_SEG;
            const long long f1 = f0 + PF_SEG < nf ? f0 + PF_SEG : nf;
            long long f = f0 + g;
            if (f >= f1) continue;
            // chunk of fragment f: the last k with frag_off[k] <= f (empty chunks are skipped by taking the last)
            int lo = 0, hi = nc - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (frag_off[mid] <= f) lo = mid; else hi = mid - 1;
            }
            int k = lo;
            long long kend = frag_off[k + 1];
            for (; f < f1; f += NG) {
                while (kend <= f) kend = frag_off[++k + 1];
                const int n = ilen[f];
                if (n < lower || n >= upper) continue;
                const long long L = chunk_len[k];
                const unsigned char *w = seq + seq_off[k];
                const long long l = lpos[f];
                const long long r = l + n - 1;
                if (l >= 0 && l < L) {
                    an += 1u;
                    if (col_ok) {
                        const unsigned b = base_row(w[l + j]);
                        a0 += b == 0u; a1 += b == 1u; a2 += b == 2u; a3 += b == 3u;
                    }
                }
                if (r >= 0 && r < L) {
                    an += 1u;
                    if (col_ok) {
                        unsigned b;
                        if (sym) {
                            b = base_row(w[r + j]);
                        } else {
                            b = base_row(w[r + 2 * flank - j]);
                            b = b < 4u ? 3u - b : 4u;          // complement: A <-> T, C <-> G
                        }
                        a0 += b == 0u; a1 += b == 1u; a2 += b == 2u; a3 += b == 3u;
                    }
                }
            }
        }
    }
    if (col_ok) {
        if (a0) atomicAdd(&s_cnt[0 * 64 + c], a0);
        if (a1) atomicAdd(&s_cnt[1 * 64 + c], a1);
        if (a2) atomicAdd(&s_cnt[2 * 64 + c], a2);
        if (a3) atomicAdd(&s_cnt[3 * 64 + c], a3);
    }
    if (counts_n && an) atomicAdd(&s_n, an);
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * CW; i += PF_BLOCK) {
        const int row = i / CW, cc = i - row * CW, col = tile * CW + cc;
        const unsigned v = s_cnt[row * 64 + cc];
        if (col < K && v) atomicAdd(&counts[(long long)row * K + col], (unsigned long long)v);
    }
    if (threadIdx.x == 0 && tile == 0 && s_n) atomicAdd(n_ins, (unsigned long long)s_n);
}

// counts[4] += the A / C / G / T bases of seq[start[i] .. end[i]) over all ranges; cum[i] = sum of the lengths of ranges < i
// (cum[n_ranges] = total).  Overlapping ranges count their bases once per range.  Block steps of PF_SPAN bases of the concatenated
// ranges; lane t reads bases t, t + 256, ... of a step, so a wave reads 64 consecutive bytes per load.
__global__ void __launch_bounds__(PF_BLOCK) natac_base_count(const unsigned char *__restrict__ seq, int nr,
                                                             const long long *__restrict__ start, const long long *__restrict__ cum,
                                                             unsigned long long *__restrict__ counts) {
    __shared__ unsigned s_cnt[4];
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long total = cum[nr];
    unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (long long s0 = (long long)blockIdx.x * PF_SPAN; s0 < total; s0 += (long long)gridDim.x * PF_SPAN) {
        long long v = s0 + threadIdx.x;
        if (v >= total) continue;
        int lo = 0, hi = nr - 1;                 // range of v: the last i with cum[i] <= v
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (cum[mid] <= v) lo = mid; else hi = mid - 1;
        }
        int r = lo;
        long long rend = cum[r + 1];
        const long long s1 = s0 + PF_SPAN < total ? s0 + PF_SPAN : total;
        for (; v < s1; v += PF_BLOCK) {
            while (rend <= v) rend = cum[++r + 1];
            const unsigned b = base_row(seq[start[r] + (v - cum[r])]);
            a0 += b == 0u; a1 += b == 1u; a2 += b == 2u; a3 += b == 3u;
        }
    }
    if (a0) atomicAdd(&s_cnt[0], a0);
    if (a1) atomicAdd(&s_cnt[1], a1);
    if (a2) atomicAdd(&s_cnt[2], a2);
    if (a3) atomicAdd(&s_cnt[3], a3);
    __syncthreads();
    if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

}  // namespace natac_pwmfit

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_insertion_seq_counts(natac_ctx *c, int32_t nc, const int32_t *chunk_len, const int64_t *frag_off, const int32_t *frag_lpos,
                               const int32_t *frag_ilen, const int64_t *seq_off, const uint8_t *seq, int flank, int lower, int upper, int sym,
                               int64_t *counts, int64_t *n_ins, double *kernel_ms) {
    using namespace natac_pwmfit;
    if (!c || !counts || !n_ins) return fail(NATAC_E_ARG, "null argument");
    if (flank < 0 || flank > PF_MAX_FLANK) return fail(NATAC_E_ARG, "flank must be in [0, %d] (got %d)", PF_MAX_FLANK, flank);
    if (upper <= lower) return fail(NATAC_E_ARG, "upper (%d) <= lower (%d)", upper, lower);
    if (nc < 0) return fail(NATAC_E_ARG, "negative chunk count");
    if (nc > 0 && (!chunk_len || !frag_off || !seq_off)) return fail(NATAC_E_ARG, "null argument");
    const int K = 2 * flank + 1;
    if (kernel_ms) *kernel_ms = 0;
    for (int i = 0; i < 4 * K; ++i) counts[i] = 0;
    *n_ins = 0;
    if (nc == 0) return NATAC_OK;
    // the kernel trusts both offset arrays: every window access lies in [seq_off[k], seq_off[k+1]), every fragment in one chunk
    if (frag_off[0] != 0 || seq_off[0] != 0) return fail(NATAC_E_ARG, "frag_off[0] and seq_off[0] must be 0");
    for (int k = 0; k < nc; ++k) {
        if (chunk_len[k] < 0) return fail(NATAC_E_ARG, "chunk %d: negative length", k);
        if (frag_off[k + 1] < frag_off[k]) return fail(NATAC_E_ARG, "frag_off must be non-decreasing (chunk %d)", k);
        if (seq_off[k + 1] - seq_off[k] != (int64_t)chunk_len[k] + K - 1)
            return fail(NATAC_E_ARG, "seq_off: chunk %d has %lld bases, its window [start - %d, end + %d) needs %lld", k,
                        (long long)(seq_off[k + 1] - seq_off[k]), flank, flank, (long long)chunk_len[k] + K - 1);
    }
    const long long nf = frag_off[nc], ns = seq_off[nc];
    if (nf > 0 && (!frag_lpos || !frag_ilen)) return fail(NATAC_E_ARG, "null argument");
    if (ns > 0 && !seq) return fail(NATAC_E_ARG, "null argument");
    if (nf >= (1LL << 40)) return fail(NATAC_E_ARG, "too many fragments in one call");
    if (nf == 0) return NATAC_OK;
    DeviceCall dc(c, "insertion_seq_counts");
    const int *d_len = dc.upload(chunk_len, (size_t)nc);
    const long long *d_fo = dc.upload((const long long *)frag_off, (size_t)nc + 1), *d_so = dc.upload((const long long *)seq_off, (size_t)nc + 1);
    const int *d_l = dc.upload(frag_lpos, (size_t)nf), *d_n = dc.upload(frag_ilen, (size_t)nf);
    const unsigned char *d_s = dc.upload((const unsigned char *)seq, (size_t)ns);
    std::vector<unsigned long long> h((size_t)4 * K + 1);
    unsigned long long *d_out = dc.zeroed<unsigned long long>(h.size());
    dc.time_begin(kernel_ms);
    if (dc.ok()) {
        const int CW = K < 64 ? K : 64;
        const long long nseg = (nf + PF_SEG - 1) / PF_SEG;
        const int bx = (int)std::min<long long>((nseg + PF_BLOCK / 64 - 1) / (PF_BLOCK / 64), 2048);
        hipLaunchKernelGGL(natac_ins_seq_counts, dim3(bx, (K + CW - 1) / CW), dim3(PF_BLOCK), 0, c->stream, d_fo, d_l, d_n, nf, (int)nc,
                           d_len, d_so, d_s, flank, lower, upper, sym ? 1 : 0, d_out, d_out + 4 * K);
        dc.launched();
    }
    dc.time_end();
    dc.fetch(h.data(), d_out, h.size());
    const int rc = dc.finish();
    if (rc) return rc;
    for (int i = 0; i < 4 * K; ++i) counts[i] = (int64_t)h[i];
    *n_ins = (int64_t)h[4 * K];
    return NATAC_OK;
}

int natac_base_counts(natac_ctx *c, const uint8_t *seq, int64_t n, int32_t nr, const int64_t *start, const int64_t *end, int64_t *counts) {
    using namespace natac_pwmfit;
    if (!c || !counts || n < 0 || nr < 0) return fail(NATAC_E_ARG, "null argument or negative size");
    if (nr > 0 && (!start || !end)) return fail(NATAC_E_ARG, "null argument");
    for (int i = 0; i < 4; ++i) counts[i] = 0;
    std::vector<long long> cum((size_t)nr + 1, 0);
    for (int i = 0; i < nr; ++i) {
        if (start[i] < 0 || end[i] < start[i] || end[i] > n)
            return fail(NATAC_E_ARG, "range %d [%lld, %lld) outside [0, %lld)", i, (long long)start[i], (long long)end[i], (long long)n);
        cum[i + 1] = cum[i] + (end[i] - start[i]);
    }
    const long long total = cum[nr];
    if (total == 0) return NATAC_OK;
    if (!seq) return fail(NATAC_E_ARG, "null argument");
    // lane counters are 32-bit: a block adds at most ceil(total / blocks) bases
    const long long bx = std::min<long long>((total + PF_SPAN - 1) / PF_SPAN, 8192);
    if ((total + bx - 1) / bx >= (1LL << 31)) return fail(NATAC_E_ARG, "ranges too long for one call");
    DeviceCall dc(c, "base_counts");
    const unsigned char *d_s = dc.upload((const unsigned char *)seq, (size_t)n);
    const long long *d_st = dc.upload((const long long *)start, (size_t)nr), *d_cum = dc.upload(cum.data(), cum.size());
    unsigned long long h[4] = {0, 0, 0, 0};
    unsigned long long *d_out = dc.zeroed<unsigned long long>(4);
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_base_count, dim3((unsigned)bx), dim3(PF_BLOCK), 0, c->stream, d_s, (int)nr, d_st, d_cum, d_out);
        dc.launched();
    }
    dc.fetch(h, d_out, 4);
    const int rc = dc.finish();
    if (rc) return rc;
    for (int i = 0; i < 4; ++i) counts[i] = (int64_t)h[i];
    return NATAC_OK;
}

}  // extern "C"
