// natac_pwmfit.hpp -- the two counting kernels behind `pyatac pwm` (pyatac/get_pwm.py of the reference):
//   natac_ins_seq_counts  the base content of the (2*flank + 1)-base window around every Tn5 insertion of a chunk list
//                         (InsertionTrack.getInsertionSequences / getStrandedInsertionSequences, pyatac/tracks.py:179-201, summed over
//                         the chunks by _pwmHelper, get_pwm.py:21-40)
//   natac_base_count      A / C / G / T counts over byte ranges (the numerators of seq.getNucFreqs / getNucFreqsFromChunkList,
//                         pyatac/seq.py:47-72)
// Every count is an integer: the kernels add in registers and LDS as 32-bit, and every block adds its totals to the int64 result with
// one atomic per counter, so the result is exact and does not depend on the order of the fragments, the blocks or the waves.
#pragma once
#include <hip/hip_runtime.h>

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
