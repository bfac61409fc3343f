// natac_tracks.hpp -- the per-base tracks of `pyatac ins --smooth`, `pyatac cov` and `pyatac bias` (pyatac/get_ins.py, get_cov.py,
// make_bias_track.py of the reference):
//   natac_ins_smooth   utils.smooth(insertions of [start - h, end + h), M, window="gaussian", mode="valid", norm=True)
//                      (get_ins.py:20-32, utils.py:23-52, fragments.pyx:43-67), h = M // 2
//   natac_center_cov   the flat-window count of fragment centres within h of every base times scale / W
//                      (get_cov.py:21-37, tracks.py:209-222, fragments.pyx:17-40), h = W // 2
//   natac_pwm_track    InsertionBiasTrack.computeBias (bias.py:85-92, seq.py:37-45): the log PWM score of every K-base window of the
//                      sequence under the chunk; it reads no fragments (see the kernel)
// One workgroup per (chunk, tile of TR_TILE bases), the int2 tile table of the other tiled kernels.  The workgroup finds the fragments
// that can reach its tile plus halo by a wave-wide search of the chunk's centre-sorted fragments, counts them into an int32 LDS
// histogram of the tile and its halo (LDS integer atomics: exact, independent of fragment order), and every lane then forms its outputs
// from the histogram.  No result depends on the order of the fragments, the tiling or how the chunks are batched.
#pragma once
#include <hip/hip_runtime.h>

namespace natac_tracks {

constexpr int TR_TILE = 1024;           // output bases per workgroup
constexpr int TR_BLOCK = 256;           // 4 waves; lane t owns outputs t, t + 256, t + 512, t + 768 of the tile
constexpr int TR_PER = TR_TILE / TR_BLOCK;
constexpr int TR_MAX_M = 4001;          // longest gaussian window (taps); the LDS holds it and the tile + 2 * (M / 2) counts
constexpr int TR_MAX_W = 4001;          // widest flat window (W + 1 taps when W is even)

constexpr int PT_MAX_CELLS = 4096;      // nrow * K cells of the log PWM held in LDS (32 KiB of doubles); so K <= 4096
constexpr int PT_MAX_ROWS = 255;        // a base's row index is one byte, and the value nrow means "no row"

// LDS bytes of natac_ins_smooth for an M-tap window (the window's doubles first, 8-byte aligned)
inline size_t ins_smooth_lds(int M) { return (size_t)M * sizeof(double) + (size_t)(TR_TILE + 2 * (M / 2)) * sizeof(int); }
// LDS bytes of natac_center_cov for half-width h: the exclusive prefix of the tile + halo counts (one more slot) + 4 wave totals
inline size_t center_cov_lds(int h) { return (size_t)(TR_TILE + 2 * h + 1 + 4) * sizeof(int); }

// LDS bytes of natac_pwm_track: the nrow x K table (doubles first) + one row index per base of the tile and its K - 1 bases of overhang
inline size_t pwm_track_lds(int nrow, int K) { return (size_t)nrow * K * sizeof(double) + (size_t)(TR_TILE + K - 1); }

// first index i in [lo, hi) with a[i] >= key (a non-decreasing there), hi if none.  Every lane of the wave calls it with the same
// arguments and gets the same answer: each round the 64 lanes probe 64 evenly spaced points, so a range of n shrinks to n / 65 + 1.
__device__ __forceinline__ long long wave_lower_bound(const int *__restrict__ a, long long lo, long long hi, long long key) {
    const int lane = threadIdx.x & 63;
    while (hi > lo) {
        const long long n = hi - lo;
        if (n <= 64) {
            const bool lt = lane < n && (long long)a[lo + lane] < key;
            return lo + __popcll(__ballot(lt));
        }
        const long long p = lo + n * (lane + 1) / 65;          // strictly increasing in the lane, inside [lo, hi)
        const int c = __popcll(__ballot((long long)a[p] < key));   // probes 0 .. c-1 lie below the key
        const long long nlo = c ? lo + n * c / 65 + 1 : lo;
        const long long nhi = c < 64 ? lo + n * (c + 1) / 65 : hi;
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

// the tile's fragment range [s_rng[0], s_rng[1]): fragments of `chunk` whose centre lies in [klo, khi).  Waves 0 and 1 search one end each.
__device__ __forceinline__ void tile_fragments(const long long *__restrict__ frag_off, const int *__restrict__ centre, int chunk, long long klo,
                                               long long khi, long long *s_rng) {
    const int wave = threadIdx.x >> 6;
    if (wave < 2) {
        const long long fa = frag_off[chunk], fb = frag_off[chunk + 1];
        const long long r = wave_lower_bound(centre, fa, fb, wave == 0 ? klo : khi);
        if ((threadIdx.x & 63) == 0) s_rng[wave] = r;
    }
}

// Gaussian-smoothed insertions.  Tile (chunk, x0) writes out[x0 .. x0 + n) of its chunk, n = min(TR_TILE, L - x0).  Local histogram
// index i is chunk position x0 - h + i, i in [0, n + 2h); an end e of a fragment with lower <= ilen < upper counts if it lies there
// (ends past either end of the chromosome included: the reference counts every end its window covers).  Output x sums w[j] * count of
// position x - h + j over j in [0, M), sequentially in fp64, and is divided by wsum (the window's own 'valid' sum).
__global__ void __launch_bounds__(TR_BLOCK) natac_ins_smooth(const int2 *__restrict__ tiles, const int *__restrict__ chunk_len,
                                                             const long long *__restrict__ frag_off, const int *__restrict__ lpos,
                                                             const int *__restrict__ ilen, const int *__restrict__ centre,
                                                             const long long *__restrict__ out_off, int lower, int upper,
                                                             const double *__restrict__ w, int M, double wsum, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_smem[];
    __shared__ long long s_rng[2];
    double *s_w = (double *)tr_smem;
    int *s_cnt = (int *)(tr_smem + (size_t)M * sizeof(double));
    const int2 t = tiles[blockIdx.x];
    const int chunk = t.x, x0 = t.y;
    const int L = chunk_len[chunk];
    const int n = min(TR_TILE, L - x0);
    const int h = M >> 1;
    const int span = n + 2 * h;
    const long long a = (long long)x0 - h, b = (long long)x0 + n + h;   // histogram covers chunk positions [a, b)
    // an end lies within (ilen - 1) / 2 + 1 of the centre for ilen >= 1, and at centre + 1 for ilen 0; negative sizes pass the filter
    // only with a negative lower bound
    const long long d = (long long)max(upper, 1) + (lower < 0 ? -(long long)lower : 0) + 2;
    tile_fragments(frag_off, centre, chunk, a - d, b + d, s_rng);
    for (int j = threadIdx.x; j < M; j += TR_BLOCK) s_w[j] = w[j];
    for (int i = threadIdx.x; i < span; i += TR_BLOCK) s_cnt[i] = 0;
    __syncthreads();
    const long long fa = s_rng[0], fb = s_rng[1];
    for (long long f = fa + threadIdx.x; f < fb; f += TR_BLOCK) {
        const int len = ilen[f];
        if (len < lower || len >= upper) continue;
        const long long l = lpos[f], r = l + len - 1;
        if (l >= a && l < b) atomicAdd(&s_cnt[l - a], 1);
        if (r >= a && r < b) atomicAdd(&s_cnt[r - a], 1);
    }
    __syncthreads();
    double acc[TR_PER];
#pragma unroll
    for (int k = 0; k < TR_PER; ++k) acc[k] = 0.0;
    // output x = threadIdx.x + 256 k reads counts x .. x + M - 1 (histogram index = output index + j)
    for (int j = 0; j < M; ++j) {
        const double wj = s_w[j];
#pragma unroll
        for (int k = 0; k < TR_PER; ++k) {
            const int x = threadIdx.x + k * TR_BLOCK;
            if (x < n) acc[k] = fma(wj, (double)s_cnt[x + j], acc[k]);
        }
    }
    double *o = out + out_off[chunk] + x0;
#pragma unroll
    for (int k = 0; k < TR_PER; ++k) {
        const int x = threadIdx.x + k * TR_BLOCK;
        if (x < n) o[x] = acc[k] / wsum;
    }
}

// exclusive prefix sum of s[0 .. N) in place, s[N] = the total (N + 1 slots; s_tot: 4 ints)
__device__ __forceinline__ void block_exclusive_scan(int *s, int N, int *s_tot) {
    const int per = (N + TR_BLOCK - 1) / TR_BLOCK;
    const int a = min((int)threadIdx.x * per, N), e = min(a + per, N);
    int sum = 0;
    for (int i = a; i < e; ++i) sum += s[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = sum;                                   // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
    }
    if (lane == 63) s_tot[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wave; ++k) base += s_tot[k];
    int run = base + inc - sum;                      // exclusive prefix of this lane's segment
    for (int i = a; i < e; ++i) {
        const int v = s[i];
        s[i] = run;
        run += v;
    }
    if (threadIdx.x == TR_BLOCK - 1) s[N] = run;     // the last lane's run ends at the total
    __syncthreads();
}

// Coverage of fragment centres.  Histogram index i = chunk position x0 - h + i, i in [0, n + 2h); a fragment with lower <= ilen < upper
// counts at its centre (the packed centre, lpos + (ilen - 1) // 2).  After the exclusive prefix P, output x = (P[x + 2h + 1] - P[x]) *
// mult: the centres within h of x, an exact integer, times scale / W in one fp64 multiply -- the reference's value bit for bit.
__global__ void __launch_bounds__(TR_BLOCK) natac_center_cov(const int2 *__restrict__ tiles, const int *__restrict__ chunk_len,
                                                             const long long *__restrict__ frag_off, const int *__restrict__ ilen,
                                                             const int *__restrict__ centre, const long long *__restrict__ out_off,
                                                             int lower, int upper, int h, double mult, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_smem[];
    __shared__ long long s_rng[2];
    const int2 t = tiles[blockIdx.x];
    const int chunk = t.x, x0 = t.y;
    const int L = chunk_len[chunk];
    const int n = min(TR_TILE, L - x0);
    const int span = n + 2 * h;
    int *s_p = (int *)tr_smem;                       // [span + 1]
    int *s_tot = s_p + TR_TILE + 2 * h + 1;          // [4]
    const long long a = (long long)x0 - h, b = (long long)x0 + n + h;
    tile_fragments(frag_off, centre, chunk, a, b, s_rng);
    for (int i = threadIdx.x; i <= span; i += TR_BLOCK) s_p[i] = 0;
    __syncthreads();
    const long long fa = s_rng[0], fb = s_rng[1];
    for (long long f = fa + threadIdx.x; f < fb; f += TR_BLOCK) {
        const int len = ilen[f];
        if (len < lower || len >= upper) continue;
        const long long i = centre[f] - a;           // in [0, span) by the search; checked all the same
        if (i >= 0 && i < span) atomicAdd(&s_p[i], 1);
    }
    __syncthreads();
    block_exclusive_scan(s_p, span, s_tot);
    double *o = out + out_off[chunk] + x0;
    for (int x = threadIdx.x; x < n; x += TR_BLOCK) o[x] = (double)(s_p[x + 2 * h + 1] - s_p[x]) * mult;
}

// Tn5 bias track.  seq[seq_off[chunk] .. seq_off[chunk + 1]) holds the L + K - 1 bases under the chunk's L outputs (any case); output x
// of the chunk scores bases x .. x + K - 1.  The tile's n + K - 1 bases are read from global memory once: upper-cased and mapped to the
// index of the PWM row with that letter (nrow: no row, the base adds 0), one byte each in LDS, next to the whole nrow x K table.  Each
// lane then forms its TR_PER outputs from LDS alone, with natac_pwm_score's association -- per row a running sum over k ascending, the
// rows added in order -- so the values are that kernel's bit for bit (a row whose letter does not match adds nothing in either).  The
// row letters must differ from one another (the host checks): a base then has one row at most.
__global__ void __launch_bounds__(TR_BLOCK) natac_pwm_track(const int2 *__restrict__ tiles, const int *__restrict__ chunk_len,
                                                            const long long *__restrict__ seq_off, const unsigned char *__restrict__ seq,
                                                            const long long *__restrict__ out_off, const double *__restrict__ logpwm,
                                                            const unsigned char *__restrict__ nucs, int nrow, int K,
                                                            double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_smem[];
    double *s_tab = (double *)tr_smem;
    unsigned char *s_row = tr_smem + (size_t)nrow * K * sizeof(double);   // [TR_TILE + K - 1]
    const int2 t = tiles[blockIdx.x];
    const int chunk = t.x, x0 = t.y;
    const int L = chunk_len[chunk];
    const int n = min(TR_TILE, L - x0);
    const int span = n + K - 1;                      // x0 + span <= L + K - 1, the chunk's bases
    const unsigned char *s = seq + seq_off[chunk] + x0;
    for (int j = threadIdx.x; j < nrow * K; j += TR_BLOCK) s_tab[j] = logpwm[j];
    for (int i = threadIdx.x; i < span; i += TR_BLOCK) {
        unsigned char c = s[i];
        if (c >= 'a' && c <= 'z') c -= 'a' - 'A';
        int row = nrow;
        for (int r = 0; r < nrow; ++r)
            if (nucs[r] == c) row = r;
        s_row[i] = (unsigned char)row;
    }
    __syncthreads();
    // output x = threadIdx.x + 256 q reads rows x .. x + K - 1; past the tile's n outputs that stays inside the TR_TILE + K - 1 bytes and
    // the sums are dropped
    double acc[TR_PER];
#pragma unroll
    for (int q = 0; q < TR_PER; ++q) acc[q] = 0.0;
    for (int r = 0; r < nrow; ++r) {
        const double *tr = s_tab + r * K;
        double rs[TR_PER];
#pragma unroll
        for (int q = 0; q < TR_PER; ++q) rs[q] = 0.0;
        for (int k = 0; k < K; ++k) {
            const double v = tr[k];
#pragma unroll
            for (int q = 0; q < TR_PER; ++q)
                if (s_row[threadIdx.x + q * TR_BLOCK + k] == r) rs[q] += v;
        }
#pragma unroll
        for (int q = 0; q < TR_PER; ++q) acc[q] += rs[q];
    }
    double *o = out + out_off[chunk] + x0;
#pragma unroll
    for (int q = 0; q < TR_PER; ++q) {
        const int x = threadIdx.x + q * TR_BLOCK;
        if (x < n) o[x] = acc[q];
    }
}

}  // namespace natac_tracks
