// natac_sites.hpp -- the kernels behind `pyatac counts`, `pyatac nucleotide` and `pyatac signal` (pyatac/get_counts.py,
// pyatac/get_nucleotide.py and pyatac/signal_around_sites.py of the reference):
//   natac_region_ranges / natac_region_count_short / natac_region_count_long
//                          fragments with an end inside each of a list of regions of one chromosome (get_counts.py:30-45)
//   natac_site_seq_count   mono- or dinucleotide content of the window around every site of one chromosome (_nucleotideHelper,
//                          get_nucleotide.py:19-38, with chunk.center / chunk.slop and seq.get_sequence / seq_to_mat)
//   natac_site_signal_div / natac_site_signal_rows / natac_site_signal_agg
//                          the track values of the window around every site, transformed per site, and their column sums
//                          (_signalHelper, signal_around_sites.py:24-74)
// Every count is an integer: lanes and waves add 32-bit partial counts, the results are 64-bit, and nothing depends on the order of
// the records, the sites, the blocks or the waves.  The signal sums are float64 and are added in one fixed order, without atomics.
// Behind the kernels: the host's checks of the operands they trust, and the entry points (natac_region_counts, natac_site_seq_counts,
// natac_site_signal).
#pragma once
#include <hip/hip_runtime.h>

#include "natac_pwmfit.hpp"

namespace natac_sites {

constexpr int RC_BLOCK = 256;           // 4 waves
constexpr int RC_SLICE = 2048;          // candidate records per wave slice; a region with more candidates is a "long" region
constexpr int RC_LONG_Y = 16;           // blocks that share the slices of one long region (x 4 waves)

// ---- pyatac counts ---------------------------------------------------------------------------------------------------------------
// A record (pos, tlen) of the chromosome, sorted by pos, is a fragment with left end l = pos + shift, insert size ilen = tlen - trim
// (shift 4, trim 8 with the ATAC offsets; 0, 0 without) and right end r = l + ilen - 1.  It counts for the region [s, e) if
// lower <= ilen < upper and (s <= l < e or s <= r < e).  Every record that can count has s - max(upper, 1) < l < e + max(0, 1 - lower)
// (r >= s needs l >= s - ilen + 1 > s - upper; ilen <= 0 puts r left of l, so l may lie right of the region), and l is monotone in
// pos: the candidates of a region are one contiguous range of records.

// cand_lo[i] = the first candidate record of region i, cand_n[i] = how many follow.  Regions with more than RC_SLICE candidates are
// appended to long_list (in no particular order; *n_long counts them), every other region is counted by natac_region_count_short.
__global__ void __launch_bounds__(RC_BLOCK) natac_region_ranges(const long long *__restrict__ pos, long long nf, long long nr,
                                                                const long long *__restrict__ start, const long long *__restrict__ end,
                                                                int lower, int upper, int shift, long long *__restrict__ cand_lo,
                                                                long long *__restrict__ cand_n, long long *__restrict__ long_list,
                                                                unsigned long long *__restrict__ n_long) {
    const long long below = (long long)(upper > 1 ? upper : 1);              // candidates have l > s - below
    const long long above = lower < 1 ? 1LL - (long long)lower : 0LL;        // and l < e + above
    for (long long i = (long long)blockIdx.x * RC_BLOCK + threadIdx.x; i < nr; i += (long long)gridDim.x * RC_BLOCK) {
        const long long p0 = start[i] - below - shift;                       // pos > p0
        const long long p1 = end[i] + above - shift;                         // pos < p1
        long long lo = 0, hi = nf;                                           // first record with pos > p0
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (pos[mid] > p0) hi = mid; else lo = mid + 1;
        }
        const long long a = lo;
        hi = nf;                                                             // first record with pos >= p1 (not before a)
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (pos[mid] >= p1) hi = mid; else lo = mid + 1;
        }
        const long long n = lo - a;
        cand_lo[i] = a;
        cand_n[i] = n;
        if (n > RC_SLICE) long_list[atomicAdd(n_long, 1ULL)] = i;
    }
}

// THE COUNTING RULE for one record (natac_cellcounts.hpp asks the same function)
__device__ __forceinline__ bool region_record_hit(long long p, long long t, long long s, long long e, int lower, int upper, int shift,
                                                  int trim) {
    const long long n = t - trim;
    const long long l = p + shift;
    const long long r = l + n - 1;
    return n >= lower && n < upper && ((l >= s && l < e) || (r >= s && r < e));
}

// the records [f0, f1) that count for [s, e), over the lanes of one wave: every lane returns the wave's total
__device__ __forceinline__ unsigned long long region_slice_count(const long long *__restrict__ pos, const long long *__restrict__ tlen,
                                                                 long long f0, long long f1, long long s, long long e, int lower,
                                                                 int upper, int shift, int trim, int lane) {
    unsigned long long total = 0;
    for (long long f = f0; f < f1; f += 64) {           // f0, f1 are wave-uniform: every lane takes part in every ballot
        const bool hit = f + lane < f1 && region_record_hit(pos[f + lane], tlen[f + lane], s, e, lower, upper, shift, trim);
        total += (unsigned long long)__popcll(__ballot(hit));
    }
    return total;
}

// one wave per region with at most RC_SLICE candidates: counts[i] = its count.  Long regions are left alone.
__global__ void __launch_bounds__(RC_BLOCK) natac_region_count_short(const long long *__restrict__ pos, const long long *__restrict__ tlen,
                                                                     long long nr, const long long *__restrict__ start,
                                                                     const long long *__restrict__ end,
                                                                     const long long *__restrict__ cand_lo,
                                                                     const long long *__restrict__ cand_n, int lower, int upper, int shift,
                                                                     int trim, unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * (RC_BLOCK / 64);
    for (long long i = (long long)blockIdx.x * (RC_BLOCK / 64) + (threadIdx.x >> 6); i < nr; i += nwaves) {
        const long long n = cand_n[i];
        if (n > RC_SLICE) continue;
        const long long f0 = cand_lo[i];
        const unsigned long long t = region_slice_count(pos, tlen, f0, f0 + n, start[i], end[i], lower, upper, shift, trim, lane);
        if (lane == 0) counts[i] = t;
    }
}

// the long regions: blockIdx.x strides over long_list, the 4 * gridDim.y waves of a row stride over the region's slices of RC_SLICE
// candidates and each adds its slice totals to the region's counter (zero before the launch) with one 64-bit atomic.
__global__ void __launch_bounds__(RC_BLOCK) natac_region_count_long(const long long *__restrict__ pos, const long long *__restrict__ tlen,
                                                                    const long long *__restrict__ start, const long long *__restrict__ end,
                                                                    const long long *__restrict__ cand_lo,
                                                                    const long long *__restrict__ cand_n,
                                                                    const long long *__restrict__ long_list,
                                                                    const unsigned long long *__restrict__ n_long, int lower, int upper,
                                                                    int shift, int trim, unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const long long nl = (long long)*n_long;
    const long long wy = (long long)blockIdx.y * (RC_BLOCK / 64) + (threadIdx.x >> 6);
    const long long ny = (long long)gridDim.y * (RC_BLOCK / 64);
    for (long long k = blockIdx.x; k < nl; k += gridDim.x) {
        const long long i = long_list[k];
        const long long f0 = cand_lo[i], n = cand_n[i];
        const long long s = start[i], e = end[i];
        const long long nslice = (n + RC_SLICE - 1) / RC_SLICE;
        unsigned long long t = 0;
        for (long long sl = wy; sl < nslice; sl += ny) {
            const long long a = f0 + sl * RC_SLICE;
            const long long b = a + RC_SLICE < f0 + n ? a + RC_SLICE : f0 + n;
            t += region_slice_count(pos, tlen, a, b, s, e, lower, upper, shift, trim, lane);
        }
        if (lane == 0 && t) atomicAdd(&counts[i], t);
    }
}

// ---- pyatac nucleotide -----------------------------------------------------------------------------------------------------------
constexpr int SS_BLOCK = 256;           // 4 waves
constexpr int SS_TILE = 512;            // columns per block (blockIdx.y = the column tile): 16 rows x 512 x 4 B = 32 KB of LDS
constexpr int SS_MAX_FLANK = 1 << 19;  // up, down <= 524288: at most 2^20 + 1 columns
constexpr int SS_SEG = 4096;            // sites per block between two flushes: no 32-bit LDS counter passes SS_SEG

// the letter of a window position as the reference sees it, 0..3 = A C G T, 4 = anything else.  On the minus strand the reference
// complements with translate('ACGT' -> 'TGCA') BEFORE it upper-cases (pyatac/seq.py:19-22, 25-34): an upper-case base is complemented,
// a lower-case (soft-masked) base is only upper-cased.
__device__ __forceinline__ unsigned site_base(unsigned ch, bool minus) {
    const unsigned b = natac_pwmfit::base_row(ch);
    return (minus && b < 4u && !(ch & 0x20u)) ? 3u - b : b;
}

// counts[R][K] += the words of the windows of the sites of one chromosome, K = up + down + 1, R = 4 (word 1: rows A C G T) or 16
// (word 2: rows in the order of itertools.product("CGAT", repeat=2)); *n_used += the sites whose window lies inside [0, n).
// A plus site with centre c reads S[j] = seq[c - up + j]; a minus site reads S[j] = seq[c + up - j] (complemented, see site_base);
// column j holds the word S[j .. j + word).  The window is [c - up, c + down + word) on plus, [c - down - word + 1, c + up + 1) on
// minus; a site whose window leaves [0, n) is skipped whole (the reference's clipped window is shorter than K + word - 1 bases).
// Lane layout: a wave is NG groups of CW lanes (CW = min(columns of the tile, 64), NG = 64 / CW); a group takes one site at a time
// and its lanes run along the window, so the bases of a window are read from consecutive addresses and the lanes of a group add to
// different LDS counters.  A block takes segments of SS_SEG sites and flushes its LDS tile into the 64-bit matrix after each.
__global__ void __launch_bounds__(SS_BLOCK) natac_site_seq_count(const unsigned char *__restrict__ seq, long long n, long long ns,
                                                                 const long long *__restrict__ center,
                                                                 const unsigned char *__restrict__ minus, int up, int down, int word,
                                                                 unsigned long long *__restrict__ counts,
                                                                 unsigned long long *__restrict__ n_used) {
    __shared__ unsigned s_cnt[16 * SS_TILE];
    __shared__ unsigned s_n;
    const int K = up + down + 1;
    const int R = word == 2 ? 16 : 4;
    const int col0 = blockIdx.y * SS_TILE;
    const int tw = K - col0 < SS_TILE ? K - col0 : SS_TILE;       // columns of this tile
    const int CW = tw < 64 ? tw : 64;
    const int NG = 64 / CW;
    const int lane = threadIdx.x & 63;
    const int g = lane / CW, c = lane - g * CW;
    const int slot = (threadIdx.x >> 6) * NG + g;                 // this group's first site of a segment
    const int nslot = (SS_BLOCK / 64) * NG;
    const long long d = word - 1;
    for (int i = threadIdx.x; i < R * SS_TILE; i += SS_BLOCK) s_cnt[i] = 0;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const long long nseg = (ns + SS_SEG - 1) / SS_SEG;
    for (long long seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const long long i1 = (seg + 1) * SS_SEG < ns ? (seg + 1) * SS_SEG : ns;
        if (g < NG) {
            for (long long i = seg * SS_SEG + slot; i < i1; i += nslot) {
                const long long ctr = center[i];
                const bool rev = minus != nullptr && minus[i] != 0;
                const long long w0 = rev ? ctr - down - d : ctr - up;
                const long long w1 = rev ? ctr + up + 1 : ctr + down + 1 + d;
                if (w0 < 0 || w1 > n) continue;
                if (blockIdx.y == 0 && c == 0) atomicAdd(&s_n, 1u);
                for (int j = c; j < tw; j += CW) {
                    const long long col = col0 + j;
                    const long long p = rev ? ctr + up - col : ctr - up + col;
                    unsigned row = site_base(seq[p], rev);
                    if (word == 2) {
                        const unsigned b2 = site_base(seq[rev ? p - 1 : p + 1], rev);
                        // A C G T -> its place in "CGAT": 2 0 1 3
                        row = (row < 4u && b2 < 4u) ? 4u * ((0xD2u >> (2u * row)) & 3u) + ((0xD2u >> (2u * b2)) & 3u) : 16u;
                    }
                    if (row < (unsigned)R) atomicAdd(&s_cnt[row * SS_TILE + j], 1u);
                }
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < R * tw; i += SS_BLOCK) {
            const int row = i / tw, j = i - row * tw;
            const unsigned v = s_cnt[row * SS_TILE + j];
            if (v) {
                atomicAdd(&counts[(long long)row * K + col0 + j], (unsigned long long)v);
                s_cnt[row * SS_TILE + j] = 0;
            }
        }
        if (threadIdx.x == 0 && s_n) {
            atomicAdd(n_used, (unsigned long long)s_n);
            s_n = 0;
        }
        __syncthreads();
    }
}

// ---- pyatac signal ---------------------------------------------------------------------------------------------------------------
constexpr int SG_BLOCK = 256;           // 4 waves
constexpr int SG_TILE = 256;            // columns per block (blockIdx.y = the column tile): one column per thread
constexpr int SG_SEG = 64;              // consecutive sites whose column sums make one partial (NATAC_SIGNAL_SEG of natac.h): the
                                        // order of every sum depends on this constant alone, never on the grid
constexpr int SG_EXP = 1, SG_POSITIVE = 2, SG_SCALE = 4;

// column `col` of site i before --scale (_signalHelper, pyatac/signal_around_sites.py:41-56): the row in genomic orientation is `lead`
// zeros, the `len` values from vals[src], zeros up to K; a minus site reads it backwards.  --exp turns the padding into 1 and leaves
// NaN; --positive replaces what compares below 0 (not NaN, not -0.0); under --scale NaN becomes 0 in the row itself.
__device__ __forceinline__ double signal_value(const double *__restrict__ vals, long long src, int len, int lead, bool rev, int K,
                                               int col, int flags) {
    const int rel = (rev ? K - 1 - col : col) - lead;
    double v = (rel >= 0 && rel < len) ? vals[src + rel] : 0.0;
    if (flags & SG_EXP) v = exp(v);
    if ((flags & SG_POSITIVE) && v < 0.0) v = 0.0;
    if ((flags & SG_SCALE) && v != v) v = 0.0;
    return v;
}

// --scale's divisor per site: div[i] = S + (S == 0), S = the sum of |row| (signal_around_sites.py:54-57).  A wave is NG groups of W
// lanes (W = the power of two >= min(K, 64), NG = 64 / W), a group takes one site: lane c adds the columns c, c + W, c + 2W, ... in
// that order, then the group's lanes are added by a butterfly over the lane distances W/2 .. 1.  The order depends on K alone.
__global__ void __launch_bounds__(SG_BLOCK) natac_site_signal_div(const double *__restrict__ vals, long long ns,
                                                                  const long long *__restrict__ src, const int *__restrict__ len,
                                                                  const int *__restrict__ lead, const unsigned char *__restrict__ minus,
                                                                  int K, int flags, double *__restrict__ div) {
    int W = 1;
    while (W < K && W < 64) W <<= 1;
    const int NG = 64 / W;
    const int lane = threadIdx.x & 63;
    const int g = lane / W, c = lane - g * W;
    const long long nwaves = (long long)gridDim.x * (SG_BLOCK / 64);
    const long long wave = (long long)blockIdx.x * (SG_BLOCK / 64) + (threadIdx.x >> 6);
    for (long long i0 = wave * NG; i0 < ns; i0 += nwaves * NG) {       // i0 is wave-uniform: every lane takes part in the butterfly
        const long long i = i0 + g;
        double s = 0.0;
        if (i < ns) {
            const long long so = src[i];
            const int ln = len[i], ld = lead[i];
            const bool rev = minus != nullptr && minus[i] != 0;
            for (int col = c; col < K; col += W) s += fabs(signal_value(vals, so, ln, ld, rev, K, col, flags));
        }
        for (int d = W >> 1; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
        if (i < ns && c == 0) div[i] = s + (s == 0.0 ? 1.0 : 0.0);
    }
}

// mat[i][col] (when mat != NULL) = the transformed row of site i, and part[seg][col] = the sum over the sites of segment seg, NaN as
// 0, added in site order starting from 0.  Segment seg holds the sites [seg * SG_SEG, (seg + 1) * SG_SEG).  Lane layout: a block is NG
// groups of CW threads (CW = the columns of its tile, at most SG_TILE; NG = SG_BLOCK / CW); a group takes one segment and its threads
// run along the window, so every row is read and written at consecutive addresses and a column's sum stays in one register.
__global__ void __launch_bounds__(SG_BLOCK) natac_site_signal_rows(const double *__restrict__ vals, long long ns,
                                                                   const long long *__restrict__ src, const int *__restrict__ len,
                                                                   const int *__restrict__ lead, const unsigned char *__restrict__ minus,
                                                                   int K, int flags, const double *__restrict__ div,
                                                                   double *__restrict__ mat, double *__restrict__ part) {
    const int col0 = blockIdx.y * SG_TILE;
    const int tw = K - col0 < SG_TILE ? K - col0 : SG_TILE;       // columns of this tile
    const int NG = SG_BLOCK / tw;
    const int g = threadIdx.x / tw, col = col0 + (threadIdx.x - g * tw);
    if (g >= NG) return;
    const long long nseg = (ns + SG_SEG - 1) / SG_SEG;
    for (long long seg = (long long)blockIdx.x * NG + g; seg < nseg; seg += (long long)gridDim.x * NG) {
        const long long i1 = (seg + 1) * SG_SEG < ns ? (seg + 1) * SG_SEG : ns;
        double acc = 0.0;
#pragma unroll 4
        for (long long i = seg * SG_SEG; i < i1; ++i) {
            double v = signal_value(vals, src[i], len[i], lead[i], minus != nullptr && minus[i] != 0, K, col, flags);
            if (flags & SG_SCALE) v = v / div[i];
            if (mat != nullptr) mat[i * K + col] = v;
            acc += v != v ? 0.0 : v;
        }
        part[seg * K + col] = acc;
    }
}

// agg[col] = part[0][col] + part[1][col] + ... in segment order, starting from 0
__global__ void __launch_bounds__(SG_BLOCK) natac_site_signal_agg(const double *__restrict__ part, long long nseg, int K,
                                                                  double *__restrict__ agg) {
    const int col = blockIdx.x * SG_BLOCK + threadIdx.x;
    if (col >= K) return;
    double acc = 0.0;
    for (long long seg = 0; seg < nseg; ++seg) acc += part[seg * K + col];
    agg[col] = acc;
}

}  // namespace natac_sites

// ---- the host's checks ------------------------------------------------------------------------------------------------------------
// The kernels here and in natac_cellcounts.hpp and natac_cellqc.hpp search their tables and index counters without looking again: the
// host checks every operand those indices rest on, once per kind.  Each check returns NATAC_OK or the refusal (NATAC_E_ARG).

constexpr long long COORD_LIM = 1LL << 60;      // coordinates far inside int64: start - upper, pos + tlen, x +- flank cannot overflow

// the fragment table of one chromosome: sorted by pos (the FragmentStore's order; the kernels search it), cell (may be null: a table
// without cells) an index into n_cells counters
static int check_fragments(int64_t nf, const int64_t *pos, const int64_t *tlen, const int32_t *cell, int32_t n_cells) {
    for (int64_t i = 0; i < nf; ++i) {
        if (pos[i] < -COORD_LIM || pos[i] > COORD_LIM || tlen[i] < -COORD_LIM || tlen[i] > COORD_LIM)
            return fail(NATAC_E_ARG, "record %lld: pos or tlen out of range", (long long)i);
        if (i && pos[i] < pos[i - 1]) return fail(NATAC_E_ARG, "pos must be non-decreasing (record %lld)", (long long)i);
        if (cell && (cell[i] < 0 || cell[i] >= n_cells))
            return fail(NATAC_E_ARG, "record %lld: cell %d outside [0, %d)", (long long)i, cell[i], n_cells);
    }
    return NATAC_OK;
}

// a table of intervals [start, end), `what` = "region" or "peak"; disjoint_ascending: every interval starts at or behind the end of the
// one before (the peaks, which the kernel searches).  An interval that is both inverted and out of range is reported as out of range
// in such a table and as inverted in the other, as the two always were.
static int check_intervals(const char *what, int64_t n, const int64_t *start, const int64_t *end, bool disjoint_ascending) {
    for (int64_t i = 0; i < n; ++i) {
        const bool far = start[i] < -COORD_LIM || end[i] > COORD_LIM;
        if (end[i] < start[i] && !(far && disjoint_ascending))
            return fail(NATAC_E_ARG, "%s %lld: end %lld < start %lld", what, (long long)i, (long long)end[i], (long long)start[i]);
        if (far) return fail(NATAC_E_ARG, "%s %lld: coordinates out of range", what, (long long)i);
        if (disjoint_ascending && i && start[i] < end[i - 1])
            return fail(NATAC_E_ARG, "%ss must be disjoint and ascending (%s %lld starts at %lld, before the end %lld of the one before)", what,
                        what, (long long)i, (long long)start[i], (long long)end[i - 1]);
    }
    return NATAC_OK;
}

// the centres of a site table the kernel searches
static int check_site_centres(int64_t ns, const int64_t *centre) {
    for (int64_t i = 0; i < ns; ++i) {
        if (centre[i] < -COORD_LIM || centre[i] > COORD_LIM) return fail(NATAC_E_ARG, "site %lld: centre out of range", (long long)i);
        if (i && centre[i] < centre[i - 1]) return fail(NATAC_E_ARG, "site centres must be ascending (site %lld)", (long long)i);
    }
    return NATAC_OK;
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------

// hits[i] = the records that count for region i (hits[nr]: natac_region_ranges' number of long regions, zeroed by the caller); cand_lo and
// cand_n are left for whoever walks the candidates again.  Queued on the call's stream, failures stay in its latch.
static void region_hits(DeviceCall &dc, natac_ctx *c, const long long *d_pos, const long long *d_tlen, long long nf, long long nr,
                        const long long *d_s, const long long *d_e, int lower, int upper, int shift, int trim, long long *d_lo,
                        long long *d_n, long long *d_long, unsigned long long *d_hits) {
    using namespace natac_sites;
    if (dc.ok()) {
        const unsigned bx = (unsigned)std::min<long long>((nr + RC_BLOCK - 1) / RC_BLOCK, 4096);
        hipLaunchKernelGGL(natac_region_ranges, dim3(bx), dim3(RC_BLOCK), 0, c->stream, d_pos, nf, nr, d_s, d_e, lower, upper, shift, d_lo,
                           d_n, d_long, d_hits + nr);
        dc.launched();
    }
    if (dc.ok()) {
        const unsigned bx = (unsigned)std::min<long long>((nr + RC_BLOCK / 64 - 1) / (RC_BLOCK / 64), 8192);
        hipLaunchKernelGGL(natac_region_count_short, dim3(bx), dim3(RC_BLOCK), 0, c->stream, d_pos, d_tlen, nr, d_s, d_e, d_lo, d_n, lower,
                           upper, shift, trim, d_hits);
        dc.launched();
    }
    if (dc.ok()) {
        // the number of long regions stays on the device: a fixed grid, idle when there is none
        const unsigned bx = (unsigned)std::min<long long>(nr, 128);
        hipLaunchKernelGGL(natac_region_count_long, dim3(bx, RC_LONG_Y), dim3(RC_BLOCK), 0, c->stream, d_pos, d_tlen, d_s, d_e, d_lo, d_n,
                           d_long, d_hits + nr, lower, upper, shift, trim, d_hits);
        dc.launched();
    }
}

extern "C" {

int natac_region_counts(natac_ctx *c, int64_t nf, const int64_t *pos, const int64_t *tlen, int64_t nr, const int64_t *start,
                        const int64_t *end, int lower, int upper, int atac, int64_t *counts, double *kernel_ms) {
    if (!c) return fail(NATAC_E_ARG, "null argument");
    if (nf < 0 || nr < 0) return fail(NATAC_E_ARG, "negative size");
    if ((nf > 0 && (!pos || !tlen)) || (nr > 0 && (!start || !end || !counts))) return fail(NATAC_E_ARG, "null argument");
    if (upper <= lower) return fail(NATAC_E_ARG, "upper (%d) <= lower (%d)", upper, lower);
    if (nf >= (1LL << 40) || nr >= (1LL << 40)) return fail(NATAC_E_ARG, "too many records or regions in one call");
    if (kernel_ms) *kernel_ms = 0;
    if (const int rc = check_intervals("region", nr, start, end, false)) return rc;
    if (const int rc = check_fragments(nf, pos, tlen, nullptr, 0)) return rc;
    for (int64_t i = 0; i < nr; ++i) counts[i] = 0;
    if (nr == 0 || nf == 0) return NATAC_OK;
    DeviceCall dc(c, "region_counts");
    const long long *d_pos = dc.upload((const long long *)pos, (size_t)nf), *d_tlen = dc.upload((const long long *)tlen, (size_t)nf);
    const long long *d_s = dc.upload((const long long *)start, (size_t)nr), *d_e = dc.upload((const long long *)end, (size_t)nr);
    long long *d_lo = dc.alloc<long long>((size_t)nr), *d_n = dc.alloc<long long>((size_t)nr), *d_long = dc.alloc<long long>((size_t)nr);
    unsigned long long *d_out = dc.zeroed<unsigned long long>((size_t)nr + 1);      // counts[nr], then the number of long regions
    dc.time_begin(kernel_ms);
    region_hits(dc, c, d_pos, d_tlen, nf, nr, d_s, d_e, lower, upper, atac ? 4 : 0, atac ? 8 : 0, d_lo, d_n, d_long, d_out);
    dc.time_end();
    dc.fetch(counts, d_out, (size_t)nr);
    return dc.finish();
}

int natac_site_seq_counts(natac_ctx *c, const uint8_t *seq, int64_t n, int64_t ns, const int64_t *center, const uint8_t *minus, int up,
                          int down, int word, int64_t *counts, int64_t *n_used, double *kernel_ms) {
    using namespace natac_sites;
    if (!c || !counts || !n_used) return fail(NATAC_E_ARG, "null argument");
    if (n < 0 || ns < 0) return fail(NATAC_E_ARG, "negative size");
    if (word != 1 && word != 2) return fail(NATAC_E_ARG, "word length must be 1 or 2 (got %d)", word);
    if (up < 0 || down < 0 || up > SS_MAX_FLANK || down > SS_MAX_FLANK)
        return fail(NATAC_E_ARG, "up and down must be in [0, %d] (got %d, %d)", SS_MAX_FLANK, up, down);
    if ((n > 0 && !seq) || (ns > 0 && !center)) return fail(NATAC_E_ARG, "null argument");
    if (ns >= (1LL << 40)) return fail(NATAC_E_ARG, "too many sites in one call");
    const int K = up + down + 1, R = word == 2 ? 16 : 4;
    if (kernel_ms) *kernel_ms = 0;
    // the kernel trusts the centres: every window it reads is checked against [0, n) from a centre inside it
    for (int64_t i = 0; i < ns; ++i)
        if (center[i] < 0 || center[i] >= n)
            return fail(NATAC_E_ARG, "site %lld: centre %lld outside the sequence [0, %lld)", (long long)i, (long long)center[i], (long long)n);
    for (long long i = 0; i < (long long)R * K; ++i) counts[i] = 0;
    *n_used = 0;
    if (ns == 0) return NATAC_OK;
    DeviceCall dc(c, "site_seq_counts");
    const size_t nout = (size_t)R * K + 1;      // counts[R x K], then n_used
    const unsigned char *d_seq = dc.upload((const unsigned char *)seq, (size_t)n);
    const long long *d_c = dc.upload((const long long *)center, (size_t)ns);
    const unsigned char *d_m = minus ? dc.upload((const unsigned char *)minus, (size_t)ns) : nullptr;
    unsigned long long *d_out = dc.zeroed<unsigned long long>(nout);
    std::vector<unsigned long long> h(nout);
    dc.time_begin(kernel_ms);
    if (dc.ok()) {
        const unsigned bx = (unsigned)std::min<long long>((ns + SS_SEG - 1) / SS_SEG, 1024);
        hipLaunchKernelGGL(natac_site_seq_count, dim3(bx, (unsigned)((K + SS_TILE - 1) / SS_TILE)), dim3(SS_BLOCK), 0, c->stream, d_seq,
                           (long long)n, (long long)ns, d_c, d_m, up, down, word, d_out, d_out + (nout - 1));
        dc.launched();
    }
    dc.time_end();
    dc.fetch(h.data(), d_out, nout);
    const int rc = dc.finish();
    if (rc) return rc;
    for (size_t i = 0; i + 1 < nout; ++i) counts[i] = (int64_t)h[i];
    *n_used = (int64_t)h[nout - 1];
    return NATAC_OK;
}

int natac_site_signal(natac_ctx *c, const double *vals, int64_t n_vals, int64_t ns, const int64_t *src, const int32_t *len,
                      const int32_t *lead, const uint8_t *minus, int K, int flags, double *mat, double *agg, double *kernel_ms) {
    using namespace natac_sites;
    static_assert(SG_SEG == NATAC_SIGNAL_SEG, "the segment length is part of the documented summation order");
    if (!c || !agg) return fail(NATAC_E_ARG, "null argument");
    if (n_vals < 0 || ns < 0) return fail(NATAC_E_ARG, "negative size");
    if (K < 1 || K > 2 * SS_MAX_FLANK + 1) return fail(NATAC_E_ARG, "K must be in [1, %d] (got %d)", 2 * SS_MAX_FLANK + 1, K);
    if (flags & ~(SG_EXP | SG_POSITIVE | SG_SCALE)) return fail(NATAC_E_ARG, "flags must be a sum of 1 (exp), 2 (positive), 4 (scale) (got %d)", flags);
    if ((n_vals > 0 && !vals) || (ns > 0 && (!src || !len || !lead))) return fail(NATAC_E_ARG, "null argument");
    if (ns >= (1LL << 40)) return fail(NATAC_E_ARG, "too many sites in one call");
    if (kernel_ms) *kernel_ms = 0;
    // the kernels trust their operands: every read is vals[src + r] with 0 <= r < len
    for (int64_t i = 0; i < ns; ++i) {
        if (len[i] < 0 || lead[i] < 0) return fail(NATAC_E_ARG, "site %lld: negative len (%d) or lead (%d)", (long long)i, len[i], lead[i]);
        if ((int64_t)lead[i] + len[i] > K)
            return fail(NATAC_E_ARG, "site %lld: lead %d + len %d exceed the %d columns", (long long)i, lead[i], len[i], K);
        if (src[i] < 0 || src[i] > n_vals || len[i] > n_vals - src[i])
            return fail(NATAC_E_ARG, "site %lld: values [%lld, %lld + %d) outside [0, %lld)", (long long)i, (long long)src[i], (long long)src[i],
                        len[i], (long long)n_vals);
    }
    for (int j = 0; j < K; ++j) agg[j] = 0;
    if (ns == 0) return NATAC_OK;
    const long long nseg = (ns + SG_SEG - 1) / SG_SEG;
    DeviceCall dc(c, "site_signal");
    const double *d_v = dc.upload(vals, (size_t)n_vals);
    const long long *d_src = dc.upload((const long long *)src, (size_t)ns);
    const int *d_len = dc.upload(len, (size_t)ns), *d_lead = dc.upload(lead, (size_t)ns);
    const unsigned char *d_m = minus ? dc.upload((const unsigned char *)minus, (size_t)ns) : nullptr;
    double *d_div = (flags & SG_SCALE) ? dc.alloc<double>((size_t)ns) : nullptr;
    double *d_mat = mat ? dc.alloc<double>((size_t)ns * K) : nullptr;
    double *d_part = dc.alloc<double>((size_t)nseg * K), *d_agg = dc.alloc<double>((size_t)K);
    dc.time_begin(kernel_ms);
    if (dc.ok() && (flags & SG_SCALE)) {
        int W = 1;                          // the kernel's group width: 64 / W sites per wave
        while (W < K && W < 64) W <<= 1;
        const long long per_block = (SG_BLOCK / 64) * (64 / W);
        const unsigned bx = (unsigned)std::min<long long>((ns + per_block - 1) / per_block, 8192);
        hipLaunchKernelGGL(natac_site_signal_div, dim3(bx), dim3(SG_BLOCK), 0, c->stream, d_v, (long long)ns, d_src, d_len, d_lead, d_m, K,
                           flags, d_div);
        dc.launched();
    }
    if (dc.ok()) {
        const int ng = SG_BLOCK / std::min(K, SG_TILE);      // segments per block in the widest tile
        const unsigned bx = (unsigned)std::min<long long>((nseg + ng - 1) / ng, 65535);
        hipLaunchKernelGGL(natac_site_signal_rows, dim3(bx, (unsigned)((K + SG_TILE - 1) / SG_TILE)), dim3(SG_BLOCK), 0, c->stream, d_v,
                           (long long)ns, d_src, d_len, d_lead, d_m, K, flags, d_div, d_mat, d_part);
        dc.launched();
    }
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_site_signal_agg, dim3((unsigned)((K + SG_BLOCK - 1) / SG_BLOCK)), dim3(SG_BLOCK), 0, c->stream, d_part, nseg,
                           K, d_agg);
        dc.launched();
    }
    dc.time_end();
    if (mat) dc.fetch(mat, d_mat, (size_t)ns * K);
    dc.fetch(agg, d_agg, (size_t)K);
    return dc.finish();
}

}  // extern "C"
