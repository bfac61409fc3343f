// natac_peakcall.hpp -- the kernels behind `pyatac peaks` (this package's own command: the reference has no peak caller): the enriched
// regions of one chromosome from its position-sorted fragments (natac_enriched_regions, include/natac.h states the rule).
//
// A chromosome is worked through in segments of at most `seg` bases (NATAC_PEAKS_SEGMENT, default PK_SEGMENT) so that no dense array is
// ever as long as the chromosome.  Working memory per base of a segment (plus its halos, at most 2 * large bases): the insertion histogram
// 4 B, its prefix sum 8 B, the verdict 1 B and the verdicts' prefix sum 8 B = 21 B; 88 MB at the default segment of 4 Mi bases.
//
// Sweep 1, per segment [s0, s1), dense range [d0, d1) = [s0 - large, s1 + large) clipped to the chromosome:
//   pk_hist      the insertion histogram of [d0, d1).  The host has the sorted pos and the smallest and largest tlen of the call, so it
//                finds by two searches the contiguous records whose l or r can lie in [d0, d1); one thread per such record, 32-bit atomics.
//   dev_scan     C = the exclusive prefix sum (natac_runtime.hpp), so that every clipped window count is one difference.
//   pk_verdict   per base of the segment: p from two prefix reads; a base with p < min_pileup (nearly all of them) is done; the others
//                read four more and the two table entries.  The verdict is a byte.
//   dev_scan     V = the prefix sum of the verdicts: "no significant base in [x - max_gap - 1, x)" is one difference.
//   pk_starts    a significant base with none in the max_gap + 1 bases before it starts a region.  Where that window leaves the segment
//                the carried `last significant base so far` answers for the part outside, so no halo depends on max_gap.  Every start is
//                appended (one atomic) with the last significant base before it, searched in V: that is the end of the region before.
//   pk_carry     one thread: the segment's last significant base and its number of them go to the carried scalars.
// The starts come back unordered, so the host sorts the pairs by start; with the carried last significant base behind the last start they
// are the regions, and the host drops those shorter than min_length.  The append buffer starts at a guess; a sweep that overflows it
// still counts, and is run again with a buffer of the counted size: no cap on the number of regions.
// Sweep 2, per segment that meets a kept region, halo half_width: pk_hist, dev_scan, then per piece (region cut to the segment) the
// largest p with its first and last base, as two packed 64-bit keys (p << 32 | 2^31 - 1 - x, p << 32 | x): a wave per piece of at most
// PK_SHORT_MAX bases (pk_summit_short), a workgroup per longer one (pk_summit_long, its waves reduce on their own).  The keys of a region
// are joined over its pieces, lanes and waves by 64-bit atomicMax: exact in any order, and that is how a region across segment borders is
// stitched.  The host takes summit = (a + b) / 2 from the keys.
// Last, pk_local: a wave per region counts the insertions within half_width, small and large of the summit from the records that can
// reach it (the same two searches, in pos on the device), summed with shuffles: p, s and g at the summit without a dense array.
// Only integer arithmetic and integer atomics: the result is a pure function of the inputs and the same for every segment size.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <utility>
#include <vector>

#include "natac_sites.hpp"

namespace natac_peakcall {

typedef unsigned long long u64;

constexpr long long PK_SEGMENT = 1LL << 22;     // NATAC_PEAKS_SEGMENT_DEFAULT: bases per segment, 21 B each
constexpr int PK_MAX_WINDOW = 50000;            // NATAC_PEAKS_MAX_WINDOW: the largest half-width of a window
constexpr int PK_BLOCK = 256;                   // four waves
constexpr int PK_SHORT_MAX = 2048;              // NATAC_PEAKS_SHORT_MAX: the longest piece one wave takes (32 bases a lane)
constexpr long long PK_FIRST_CAPACITY = 4096;   // NATAC_PEAKS_FIRST_CAPACITY: region starts the first sweep has room for

// one thread per record of [i0, i1): its insertions inside [d0, d1) (a part of the chromosome) into hist[x - d0]
__global__ void __launch_bounds__(PK_BLOCK) pk_hist(const long long *__restrict__ pos, const long long *__restrict__ tlen, long long i0,
                                                    long long i1, long long d0, long long d1, unsigned *__restrict__ hist) {
    for (long long i = i0 + (long long)blockIdx.x * PK_BLOCK + threadIdx.x; i < i1; i += (long long)gridDim.x * PK_BLOCK) {
        const long long l = pos[i] + 4, r = pos[i] + tlen[i] - 5;
        if (l >= d0 && l < d1) atomicAdd(&hist[l - d0], 1u);
        if (r >= d0 && r < d1) atomicAdd(&hist[r - d0], 1u);
    }
}

// C_w(x) over the dense range [d0, d1): C[j] = the insertions in [d0, d0 + j).  The caller's range holds x - w .. x + w but for the
// chromosome's ends, so the two clips are the rule's clips.
__device__ __forceinline__ unsigned pk_window(const u64 *__restrict__ C, long long d0, long long d1, long long x, int w) {
    const long long hi = x + w + 1 < d1 ? x + w + 1 : d1, lo = x - w > d0 ? x - w : d0;
    return (unsigned)(C[hi - d0] - C[lo - d0]);
}

// flag[j] = base s0 + j is significant, j < m
__global__ void __launch_bounds__(PK_BLOCK) pk_verdict(const u64 *__restrict__ C, long long d0, long long d1, long long s0, long long m,
                                                       int h, int S, int L, unsigned min_pileup, int n_table,
                                                       const int *__restrict__ thr_small, const int *__restrict__ thr_large,
                                                       unsigned char *__restrict__ flag) {
    const long long j = (long long)blockIdx.x * PK_BLOCK + threadIdx.x;
    if (j >= m) return;
    const long long x = s0 + j;
    const unsigned p = pk_window(C, d0, d1, x, h);
    bool sig = false;
    if (p >= min_pileup) {
        const int k = p < (unsigned)(n_table - 1) ? (int)p : n_table - 1;
        const int ts = thr_small[k], tl = thr_large[k];
        sig = ts >= 0 && tl >= 0 && pk_window(C, d0, d1, x, S) <= (unsigned)ts && pk_window(C, d0, d1, x, L) <= (unsigned)tl;
    }
    flag[j] = sig ? 1 : 0;
}

// the smallest y in [0, hi) with V[y + 1] >= v (V is non-decreasing; V[hi] >= v): the base that brings the count of verdicts to v
__device__ __forceinline__ long long pk_reach(const u64 *__restrict__ V, long long hi, u64 v) {
    long long lo = 0;
    --hi;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (V[mid + 1] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// state[0] = the last significant base before this segment (-1: none yet), state[1] = the starts found so far, state[2] = the
// significant bases so far.  A start goes to slot state[1]++ if that is below cap.
__global__ void __launch_bounds__(PK_BLOCK) pk_starts(const unsigned char *__restrict__ flag, const u64 *__restrict__ V, long long s0,
                                                      long long m, long long gap1, long long *__restrict__ state, long long cap,
                                                      long long *__restrict__ start, long long *__restrict__ prev_end) {
    const long long j = (long long)blockIdx.x * PK_BLOCK + threadIdx.x;
    if (j >= m || !flag[j]) return;
    const long long x = s0 + j, last = state[0];
    const u64 before = V[j];                                     // significant bases in [s0, x)
    bool head;
    if (j >= gap1) head = before == V[j - gap1];
    else head = before == 0 && (last < 0 || last < x - gap1);    // (last == -1: none at all)
    if (!head) return;
    const long long pe = before ? s0 + pk_reach(V, j, before) : last;
    const long long slot = (long long)atomicAdd((u64 *)&state[1], 1ULL);
    if (slot < cap) {
        start[slot] = x;
        prev_end[slot] = pe;
    }
}

__global__ void pk_carry(const u64 *__restrict__ V, long long s0, long long m, long long *__restrict__ state) {
    if (threadIdx.x || blockIdx.x) return;
    const u64 n = V[m];
    if (n) {
        state[0] = s0 + pk_reach(V, m, n);
        state[2] += (long long)n;
    }
}

// the bases [a0, a1) of one region, lane `t` of `stride` takes every stride-th: the largest p with its first and last base as packed keys
__device__ __forceinline__ void pk_piece(const u64 *__restrict__ C, long long d0, long long d1, int h, long long a0, long long a1, int t,
                                         int stride, u64 *__restrict__ key_first, u64 *__restrict__ key_last) {
    unsigned best = 0;
    long long fa = -1, lb = -1;
    for (long long x = a0 + t; x < a1; x += stride) {
        const unsigned p = pk_window(C, d0, d1, x, h);
        if (fa < 0 || p > best) { best = p; fa = lb = x; }
        else if (p == best) lb = x;
    }
    u64 ka = fa < 0 ? 0ULL : ((u64)best << 32) | (u64)(0x7fffffffLL - fa);
    u64 kb = fa < 0 ? 0ULL : ((u64)best << 32) | (u64)lb;
    for (int off = 32; off > 0; off >>= 1) {
        const u64 oa = __shfl_xor(ka, off), ob = __shfl_xor(kb, off);
        ka = oa > ka ? oa : ka;
        kb = ob > kb ? ob : kb;
    }
    if ((threadIdx.x & 63) == 0 && ka) {
        atomicMax(key_first, ka);
        atomicMax(key_last, kb);
    }
}

// a wave per region of [r0, r1): its piece inside [s0, s1), if that is at most PK_SHORT_MAX bases
__global__ void __launch_bounds__(PK_BLOCK) pk_summit_short(const u64 *__restrict__ C, long long d0, long long d1, int h, long long s0,
                                                            long long s1, const long long *__restrict__ start,
                                                            const long long *__restrict__ end, long long r0, long long r1,
                                                            u64 *__restrict__ key_first, u64 *__restrict__ key_last) {
    const long long i = r0 + (long long)blockIdx.x * (PK_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= r1) return;                                         // wave-uniform
    const long long a0 = start[i] > s0 ? start[i] : s0, a1 = end[i] < s1 ? end[i] : s1;
    if (a1 - a0 > PK_SHORT_MAX) return;
    pk_piece(C, d0, d1, h, a0, a1, threadIdx.x & 63, 64, key_first + i, key_last + i);
}

// a workgroup per listed region: its piece inside [s0, s1) (the host lists the regions whose piece is longer than PK_SHORT_MAX)
__global__ void __launch_bounds__(PK_BLOCK) pk_summit_long(const u64 *__restrict__ C, long long d0, long long d1, int h, long long s0,
                                                           long long s1, const long long *__restrict__ start,
                                                           const long long *__restrict__ end, const long long *__restrict__ list,
                                                           u64 *__restrict__ key_first, u64 *__restrict__ key_last) {
    const long long i = list[blockIdx.x];
    const long long a0 = start[i] > s0 ? start[i] : s0, a1 = end[i] < s1 ? end[i] : s1;
    pk_piece(C, d0, d1, h, a0, a1, threadIdx.x, PK_BLOCK, key_first + i, key_last + i);
}

// first index in [0, n) with a[i] >= v (n if none)
__device__ __forceinline__ long long pk_lower(const long long *__restrict__ a, long long n, long long v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a wave per region: the insertions of the chromosome [0, n) within h, within S and within L of its summit (the summit is the middle of
// the first and the last highest base and need not be one of them).  off_lo / off_hi: an insertion of a record at pos lies in
// [pos + off_lo, pos + off_hi] (from the call's smallest and largest tlen)
__global__ void __launch_bounds__(PK_BLOCK) pk_local(const long long *__restrict__ pos, const long long *__restrict__ tlen, long long nf,
                                                     long long n, long long off_lo, long long off_hi, int h, int S, int L,
                                                     const long long *__restrict__ summit, long long nr, int *__restrict__ pileup,
                                                     int *__restrict__ n_small, int *__restrict__ n_large) {
    const long long i = (long long)blockIdx.x * (PK_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= nr) return;                                         // wave-uniform
    const int lane = threadIdx.x & 63;
    const long long c = summit[i];
    const long long i0 = pk_lower(pos, nf, c - L - off_hi), i1 = pk_lower(pos, nf, c + L - off_lo + 1);
    unsigned ch = 0, cs = 0, cl = 0;
    for (long long k = i0 + lane; k < i1; k += 64) {
        const long long l = pos[k] + 4, r = pos[k] + tlen[k] - 5;
        const long long dl = l > c ? l - c : c - l, dr = r > c ? r - c : c - r;
        if (l >= 0 && l < n) { ch += dl <= h; cs += dl <= S; cl += dl <= L; }
        if (r >= 0 && r < n) { ch += dr <= h; cs += dr <= S; cl += dr <= L; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        ch += __shfl_xor(ch, off);
        cs += __shfl_xor(cs, off);
        cl += __shfl_xor(cl, off);
    }
    if (lane == 0) {
        pileup[i] = (int)ch;
        n_small[i] = (int)cs;
        n_large[i] = (int)cl;
    }
}

// what both sweeps share: the records that can reach a dense range, its histogram and prefix sum
struct Reach {
    natac_ctx *c;
    DeviceCall &dc;
    const int64_t *pos;              // host
    long long nf, off_lo, off_hi;
    const long long *d_pos, *d_tlen;
    unsigned *d_hist;
    u64 *d_C;
    // C[0 .. d1 - d0] of the dense range [d0, d1)
    void prefix(long long d0, long long d1) {
        const long long nd = d1 - d0;
        dc.zero(d_hist, (size_t)nd);
        const long long i0 = std::lower_bound(pos, pos + nf, (int64_t)(d0 - off_hi)) - pos;
        const long long i1 = std::lower_bound(pos, pos + nf, (int64_t)(d1 - off_lo)) - pos;
        if (i1 > i0 && dc.ok()) {
            const unsigned bx = (unsigned)std::min<long long>((i1 - i0 + PK_BLOCK - 1) / PK_BLOCK, 1 << 16);
            hipLaunchKernelGGL(pk_hist, dim3(bx), dim3(PK_BLOCK), 0, c->stream, d_pos, d_tlen, i0, i1, d0, d1, d_hist);
            dc.launched();
        }
        dev_scan(c, d_hist, nd, d_C, dc);
    }
};

static long long segment_size() {
    if (const char *e = getenv("NATAC_PEAKS_SEGMENT")) {
        const long long v = atoll(e);
        if (v >= 1 && v <= (1LL << 28)) return v;
    }
    return PK_SEGMENT;
}

}  // namespace natac_peakcall

// ---- entry point -----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_enriched_regions(natac_ctx *c, int64_t nf, const int64_t *pos, const int64_t *tlen, int64_t chrom_len, int half_width, int small,
                           int large, int max_gap, int min_length, int min_pileup, int32_t n_table, const int32_t *thr_small,
                           const int32_t *thr_large, int64_t *n_regions, int64_t capacity, int64_t *start, int64_t *end, int64_t *summit,
                           int32_t *pileup, int32_t *n_small, int32_t *n_large, int64_t *n_found, int64_t *n_significant,
                           double *kernel_ms) {
    using namespace natac_peakcall;
    static_assert(PK_SEGMENT == NATAC_PEAKS_SEGMENT_DEFAULT && PK_MAX_WINDOW == NATAC_PEAKS_MAX_WINDOW && PK_SHORT_MAX == NATAC_PEAKS_SHORT_MAX &&
                      PK_FIRST_CAPACITY == NATAC_PEAKS_FIRST_CAPACITY,
                  "the kernels' sizes are in natac.h");
    if (!c || !n_regions) return fail(NATAC_E_ARG, "null argument");
    if (nf < 0 || capacity < 0) return fail(NATAC_E_ARG, "negative size");
    if (nf > 0 && (!pos || !tlen)) return fail(NATAC_E_ARG, "null argument");
    if (capacity > 0 && (!start || !end || !summit || !pileup || !n_small || !n_large)) return fail(NATAC_E_ARG, "null argument");
    if (!thr_small || !thr_large) return fail(NATAC_E_ARG, "null table");
    if (n_table < 2) return fail(NATAC_E_ARG, "n_table must be at least 2 (got %d)", (int)n_table);
    if (chrom_len < 1 || chrom_len >= (1LL << 31)) return fail(NATAC_E_ARG, "chrom_len must be in [1, 2^31) (got %lld)", (long long)chrom_len);
    if (nf >= (1LL << 30)) return fail(NATAC_E_ARG, "too many records in one call");
    if (half_width < 1 || small < half_width || large < small || large > NATAC_PEAKS_MAX_WINDOW)
        return fail(NATAC_E_ARG, "1 <= half_width <= small <= large <= %d must hold (got %d, %d, %d)", NATAC_PEAKS_MAX_WINDOW, half_width, small,
                    large);
    if (max_gap < 0) return fail(NATAC_E_ARG, "max_gap must not be negative (got %d)", max_gap);
    if (min_length < 1) return fail(NATAC_E_ARG, "min_length must be at least 1 (got %d)", min_length);
    if (min_pileup < 1) return fail(NATAC_E_ARG, "min_pileup must be at least 1 (got %d)", min_pileup);
    if (const int rc = check_fragments(nf, pos, tlen, nullptr, 0)) return rc;
    // an insertion of a record at pos lies in [pos + off_lo, pos + off_hi]: l = pos + 4, r = pos + tlen - 5
    long long off_lo = 4, off_hi = 4;
    for (int64_t i = 0; i < nf; ++i) {
        off_lo = std::min<long long>(off_lo, tlen[i] - 5);
        off_hi = std::max<long long>(off_hi, tlen[i] - 5);
    }
    const long long n = chrom_len, seg = segment_size(), gap1 = (long long)max_gap + 1;
    auto done = [&](long long kept, long long found, long long nsig) {
        *n_regions = kept;
        if (n_found) *n_found = found;
        if (n_significant) *n_significant = nsig;
        return NATAC_OK;
    };
    if (kernel_ms) *kernel_ms = 0;       // behind the checks: a refused call leaves every output as it was
    if (nf == 0) return done(0, 0, 0);

    DeviceCall dc(c, "enriched_regions");
    const long long *d_pos = dc.upload((const long long *)pos, (size_t)nf), *d_tlen = dc.upload((const long long *)tlen, (size_t)nf);
    const int *d_ts = dc.upload((const int *)thr_small, (size_t)n_table), *d_tl = dc.upload((const int *)thr_large, (size_t)n_table);
    const long long m_max = std::min(seg, n), nd_max = std::min(n, m_max + 2LL * large);
    Reach reach{c, dc, pos, (long long)nf, off_lo, off_hi, d_pos, d_tlen, dc.alloc<unsigned>((size_t)nd_max), dc.alloc<u64>((size_t)nd_max + 1)};
    unsigned char *d_flag = dc.alloc<unsigned char>((size_t)m_max);
    u64 *d_V = dc.alloc<u64>((size_t)m_max + 1);
    long long *d_state = dc.alloc<long long>(3);
    dc.time_begin(kernel_ms);

    // sweep 1: the region starts, each with the end of the region before
    long long cap = PK_FIRST_CAPACITY, state[3] = {-1, 0, 0};
    std::vector<long long> h_start, h_prev;
    for (;;) {                                           // at most twice: the second buffer has the counted size
        long long *d_start = dc.alloc<long long>((size_t)cap), *d_prev = dc.alloc<long long>((size_t)cap);
        const long long init[3] = {-1, 0, 0};
        dc.send(d_state, init, 3);
        for (long long s0 = 0; s0 < n && dc.ok(); s0 += seg) {
            const long long s1 = std::min(n, s0 + seg), m = s1 - s0, d0 = std::max(0LL, s0 - large), d1 = std::min(n, s1 + large);
            reach.prefix(d0, d1);
            if (!dc.ok()) break;
            const unsigned bx = (unsigned)((m + PK_BLOCK - 1) / PK_BLOCK);
            hipLaunchKernelGGL(pk_verdict, dim3(bx), dim3(PK_BLOCK), 0, c->stream, reach.d_C, d0, d1, s0, m, half_width, small, large,
                               (unsigned)min_pileup, (int)n_table, d_ts, d_tl, d_flag);
            dc.launched();
            dev_scan(c, d_flag, m, d_V, dc);
            if (!dc.ok()) break;
            hipLaunchKernelGGL(pk_starts, dim3(bx), dim3(PK_BLOCK), 0, c->stream, d_flag, d_V, s0, m, gap1, d_state, cap, d_start, d_prev);
            hipLaunchKernelGGL(pk_carry, dim3(1), dim3(64), 0, c->stream, d_V, s0, m, d_state);
            dc.launched();
        }
        dc.fetch(state, d_state, 3);
        if (const int rc = dc.sync()) return rc;        // (the init array above has been read by now)
        if (state[1] <= cap) {
            h_start.resize((size_t)state[1]);
            h_prev.resize((size_t)state[1]);
            dc.fetch(h_start.data(), d_start, (size_t)state[1]);
            dc.fetch(h_prev.data(), d_prev, (size_t)state[1]);
            if (const int rc = dc.sync()) return rc;
            break;
        }
        cap = state[1];                                  // counted: the second sweep has room for all of them
    }
    const long long found = state[1], nsig = state[2];
    // the regions, ascending: [start, last significant base before the next start + 1), shorter than min_length dropped
    std::vector<std::pair<long long, long long>> ev((size_t)found);
    for (long long i = 0; i < found; ++i) ev[(size_t)i] = {h_start[(size_t)i], h_prev[(size_t)i]};
    std::sort(ev.begin(), ev.end());
    std::vector<long long> r_start, r_end;
    for (long long i = 0; i < found; ++i) {
        const long long a = ev[(size_t)i].first, b = (i + 1 < found ? ev[(size_t)i + 1].second : state[0]) + 1;
        if (b - a >= min_length) {
            r_start.push_back(a);
            r_end.push_back(b);
        }
    }
    const long long kept = (long long)r_start.size();
    if (kept == 0 || kept > capacity) {                  // too many for the caller's arrays: they stay as they were, the count says so
        dc.time_end();
        if (const int rc = dc.finish()) return rc;
        return done(kept, found, nsig);
    }

    // sweep 2: the largest pileup of every region with its first and last base
    const long long *d_rs = dc.upload(r_start.data(), (size_t)kept), *d_re = dc.upload(r_end.data(), (size_t)kept);
    u64 *d_keys = dc.zeroed<u64>(2 * (size_t)kept);
    std::vector<long long> long_list, seg_r0, seg_r1, seg_l0;       // per segment: its regions [r0, r1) and its long pieces from l0
    {
        long long r0 = 0;
        for (long long s0 = 0; s0 < n; s0 += seg) {
            const long long s1 = std::min(n, s0 + seg);
            while (r0 < kept && r_end[(size_t)r0] <= s0) ++r0;
            long long r1 = r0;
            seg_l0.push_back((long long)long_list.size());
            while (r1 < kept && r_start[(size_t)r1] < s1) {
                if (std::min(r_end[(size_t)r1], s1) - std::max(r_start[(size_t)r1], s0) > PK_SHORT_MAX) long_list.push_back(r1);
                ++r1;
            }
            seg_r0.push_back(r0);
            seg_r1.push_back(r1);
        }
        seg_l0.push_back((long long)long_list.size());
    }
    const long long *d_long = dc.upload(long_list.data(), long_list.size());
    size_t k = 0;
    for (long long s0 = 0; s0 < n && dc.ok(); s0 += seg, ++k) {
        const long long r0 = seg_r0[k], r1 = seg_r1[k], n_long = seg_l0[k + 1] - seg_l0[k];
        if (r1 == r0) continue;
        const long long s1 = std::min(n, s0 + seg), d0 = std::max(0LL, s0 - half_width), d1 = std::min(n, s1 + half_width);
        reach.prefix(d0, d1);
        if (!dc.ok()) break;
        if (r1 - r0 > n_long) {
            const unsigned bx = (unsigned)((r1 - r0 + PK_BLOCK / 64 - 1) / (PK_BLOCK / 64));
            hipLaunchKernelGGL(pk_summit_short, dim3(bx), dim3(PK_BLOCK), 0, c->stream, reach.d_C, d0, d1, half_width, s0, s1, d_rs, d_re, r0, r1,
                               d_keys, d_keys + kept);
        }
        if (n_long)
            hipLaunchKernelGGL(pk_summit_long, dim3((unsigned)n_long), dim3(PK_BLOCK), 0, c->stream, reach.d_C, d0, d1, half_width, s0, s1, d_rs,
                               d_re, d_long + seg_l0[k], d_keys, d_keys + kept);
        dc.launched();
    }
    std::vector<u64> keys(2 * (size_t)kept);
    dc.fetch(keys.data(), d_keys, 2 * (size_t)kept);
    if (const int rc = dc.sync()) return rc;
    std::vector<long long> r_summit((size_t)kept);
    for (long long i = 0; i < kept; ++i) {
        const long long a = 0x7fffffffLL - (long long)(keys[(size_t)i] & 0xffffffffULL), b = (long long)(keys[(size_t)(kept + i)] & 0xffffffffULL);
        r_summit[(size_t)i] = (a + b) / 2;
    }

    // the three counts at every summit
    const long long *d_summit = dc.upload(r_summit.data(), (size_t)kept);
    int *d_loc = dc.alloc<int>(3 * (size_t)kept);
    if (dc.ok()) {
        const unsigned bx = (unsigned)((kept + PK_BLOCK / 64 - 1) / (PK_BLOCK / 64));
        hipLaunchKernelGGL(pk_local, dim3(bx), dim3(PK_BLOCK), 0, c->stream, d_pos, d_tlen, (long long)nf, n, off_lo, off_hi, half_width, small,
                           large, d_summit, kept, d_loc, d_loc + kept, d_loc + 2 * kept);
        dc.launched();
    }
    dc.time_end();
    std::vector<int> loc(3 * (size_t)kept);
    dc.fetch(loc.data(), d_loc, 3 * (size_t)kept);
    if (const int rc = dc.finish()) return rc;
    for (long long i = 0; i < kept; ++i) {
        start[i] = r_start[(size_t)i];
        end[i] = r_end[(size_t)i];
        summit[i] = r_summit[(size_t)i];
        pileup[i] = loc[(size_t)i];
        n_small[i] = loc[(size_t)(kept + i)];
        n_large[i] = loc[(size_t)(2 * kept + i)];
    }
    return done(kept, found, nsig);
}

}  // extern "C"
