// natac_motifs.hpp -- the kernels behind `pyatac motifs` (this package's own command: the reference has no motif scanner): the sites of
// many integer position weight matrices in the scan intervals of one chromosome, both strands, and the window-by-motif match counts
// (natac_motif_scan, include/natac.h states the rule).
//
//   mt_pack     one thread per 64 bases: the chromosome as 2 bits a base (A C G T = 0 1 2 3, two 64-bit words of 32 bases) and one
//               validity bit a base = "is one of ACGTacgt AND lies in a scan interval".  Scan intervals never abut (the host merged
//               them), so a motif window is scored exactly when its W validity bits are all set: no interval is looked at again.
//   mt_scan     the hot loop.  The host lists the 64-base tiles that meet a scan interval; MT_RUN_TILES consecutive entries of the list
//               are a run, and one wave takes one run for one motif group (at most MT_GROUP motifs, at most MT_LDS_DWORDS dwords of
//               tables, which the workgroup copies to LDS once).  A lane is one window start: it holds its next 64 bases in four
//               registers and the length of its valid stretch, and walks the columns of one motif after the other, four at a time (the
//               tables are padded with zero columns to a multiple of four, so the walk has no tail).  The scores of a column are
//               wave-uniform, the base is the lane's: a look-up touches four (eight) consecutive dwords, conflict-free.
//               Two accumulator arms, chosen per motif on the host:
//                 packed  one dword holds (S[j][b] - min_j) in its low half and (S[W-1-j][3-b] - min_{W-1-j}) in its high half.  Both
//                         halves are sums of non-negative terms; the host takes this arm only when sum_j (max_j - min_j) <= 65535, so
//                         neither half can carry and ONE 32-bit add advances both strands.  score = half + sum_j min_j.
//                 wide    two int32 tables (forward, reverse complement), two reads and two adds per column.
//               Per (tile, group) the wave leaves a 64-bit mask of the motifs with a hit there, per (motif, run) the number of hits.
//   dev_scan    the prefix sum of the counts in (motif, run) order: where every run's hits of every motif go.  Its total is *n_hits.
//   mt_fill     a wave per (run, group) again, but only the (tile, motif) pairs of the masks are scored again -- about 2 * 64 * p of
//               them at a p-value of p -- and their hits are written at the run's offset, lanes in order, `+` before `-`: the arrays are
//               sorted by (motif, start, strand) as they are filled.  Nothing is appended atomically and nothing is sorted.
//   mt_counts   one thread per (window, motif): two binary searches in that motif's stretch of the sorted starts.
// Only integer arithmetic, and no atomics at all: the result is a pure function of the inputs.
// Device memory: 1 + 3/8 bytes per base, 12 bytes per (motif, run), 8 bytes per (tile, group), 17 bytes per hit, 4 per (window, motif).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <utility>
#include <vector>

#include "natac_runtime.hpp"

namespace natac_motifs {

typedef unsigned long long u64;

constexpr int MT_MAX_WIDTH = 64;          // NATAC_MOTIF_MAX_WIDTH: a lane holds 64 bases
constexpr int MT_MAX_MOTIFS = 4096;       // NATAC_MOTIF_MAX_MOTIFS
constexpr int MT_TILE = 64;               // NATAC_MOTIF_TILE: window starts per wave step
constexpr int MT_RUN_TILES = 16;          // NATAC_MOTIF_RUN_TILES: listed tiles per run (the unit of the hit counts)
constexpr int MT_GROUP = 64;              // NATAC_MOTIF_GROUP: motifs per group (one bit each in a tile's hit mask)
constexpr int MT_CHUNK = 4;               // columns per step of the column walk: a motif's table is padded to a multiple of it
constexpr int MT_LDS_DWORDS = 8192;       // the most table dwords of a group: 32 KiB of LDS (a launch takes what its largest group needs)
constexpr int MT_BLOCK = 256;             // four waves, four runs
constexpr int MT_WAVES = MT_BLOCK / 64;
constexpr long long MT_MAX_CELLS = 1LL << 27;   // (motif, run) counters of one call; longer calls take longer runs

struct Motif {
    int w;          // columns
    int wide;       // 0: packed arm, 1: wide arm
    int off;        // first dword of its table inside its group's tables
    int thr;        // packed: T - sum of column minima clipped to [0, 65536]; wide: T
    int base;       // packed: the sum of the column minima; wide: 0
};

// ---- the sequence ------------------------------------------------------------------------------------------------------------
// word k of `valid` covers bases [64 k, 64 k + 64); words 2 k and 2 k + 1 of `code` its two halves.  nw words are written; those at
// and behind the chromosome's end are zero (a lane reads one validity word and two code words past its own).
// iv_start / iv_end: the n_iv scan intervals, disjoint, ascending, never abutting.
__global__ void __launch_bounds__(256) mt_pack(const unsigned char *__restrict__ seq, long long n, long long nw,
                                               const long long *__restrict__ iv_start, const long long *__restrict__ iv_end, int n_iv,
                                               u64 *__restrict__ code, u64 *__restrict__ valid) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= nw) return;
    const long long x0 = k * 64;
    u64 c[2] = {0, 0}, acgt = 0;
    for (int i = 0; i < 64; ++i) {
        const long long x = x0 + i;
        if (x >= n) break;
        const unsigned ch = seq[x] & 0xdfu;              // upper case
        const unsigned v = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
        if (v < 4u) {
            c[i >> 5] |= (u64)v << (2 * (i & 31));
            acgt |= 1ULL << i;
        }
    }
    // the intervals that meet [x0, x0 + 64): the first with end > x0, then on while start < x0 + 64
    u64 cover = 0;
    int lo = 0, hi = n_iv;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (iv_end[mid] > x0) hi = mid; else lo = mid + 1;
    }
    for (int i = lo; i < n_iv; ++i) {
        const long long a = iv_start[i] - x0, b = iv_end[i] - x0;       // b > 0
        if (a >= 64) break;
        const u64 from = a <= 0 ? ~0ULL : ~0ULL << a, to = b >= 64 ? ~0ULL : (1ULL << b) - 1;
        cover |= from & to;
    }
    code[2 * k] = c[0];
    code[2 * k + 1] = c[1];
    valid[k] = acgt & cover;
}

// ---- what mt_scan and mt_fill share ---------------------------------------------------------------------------------------------
// the next 64 bases of a window start as four registers of 16 and the number of scorable bases from it on (0 .. 64)
struct Lane {
    unsigned b[4];
    int run;
};

__device__ __forceinline__ Lane mt_lane(const u64 *__restrict__ code, const u64 *__restrict__ valid, long long tile, int lane) {
    const long long w0 = 2 * tile + (lane >> 5);
    const int s = 2 * (lane & 31);
    const u64 c0 = code[w0], c1 = code[w0 + 1], c2 = code[w0 + 2];
    const u64 lo = s ? (c0 >> s) | (c1 << (64 - s)) : c0, hi = s ? (c1 >> s) | (c2 << (64 - s)) : c1;
    const u64 v0 = valid[tile], v1 = valid[tile + 1];
    const u64 v = lane ? (v0 >> lane) | (v1 << (64 - lane)) : v0;
    Lane L;
    L.b[0] = (unsigned)lo;
    L.b[1] = (unsigned)(lo >> 32);
    L.b[2] = (unsigned)hi;
    L.b[3] = (unsigned)(hi >> 32);
    L.run = ~v ? __builtin_ctzll(~v) : 64;
    return L;
}

// both strands' scores of one motif at the lane's window start: tab = its table in LDS, its columns padded with zero columns to a
// multiple of MT_CHUNK, so the walk is whole chunks of MT_CHUNK independent reads (a padding column adds 0 whatever base it meets).
// The walk is written out over all of a lane's 64 bases (Walk<C>: the register and the shift of chunk C are constants) and a motif
// leaves it by a wave-uniform branch.
template <int C>
struct Walk {
    static __device__ __forceinline__ void packed(const Lane &L, const unsigned *__restrict__ tab, int w, unsigned &acc) {
        if (MT_CHUNK * C >= w) return;                             // wave-uniform
        const unsigned bits = L.b[C / 4] >> (8 * (C % 4));
        const unsigned *t = tab + 4 * MT_CHUNK * C;
        const unsigned s0 = t[bits & 3u], s1 = t[4 + ((bits >> 2) & 3u)], s2 = t[8 + ((bits >> 4) & 3u)], s3 = t[12 + ((bits >> 6) & 3u)];
        acc += (s0 + s1) + (s2 + s3);
        Walk<C + 1>::packed(L, tab, w, acc);
    }
    static __device__ __forceinline__ void wide(const Lane &L, const unsigned *__restrict__ tab, int w, int &f, int &r) {
        if (MT_CHUNK * C >= w) return;
        const unsigned bits = L.b[C / 4] >> (8 * (C % 4));
        const unsigned *t = tab + 8 * MT_CHUNK * C;
        const unsigned k0 = bits & 3u, k1 = 8 + ((bits >> 2) & 3u), k2 = 16 + ((bits >> 4) & 3u), k3 = 24 + ((bits >> 6) & 3u);
        f += ((int)t[k0] + (int)t[k1]) + ((int)t[k2] + (int)t[k3]);
        r += ((int)t[k0 + 4] + (int)t[k1 + 4]) + ((int)t[k2 + 4] + (int)t[k3 + 4]);
        Walk<C + 1>::wide(L, tab, w, f, r);
    }
};
template <>
struct Walk<MT_MAX_WIDTH / MT_CHUNK> {
    static __device__ __forceinline__ void packed(const Lane &, const unsigned *, int, unsigned &) {}
    static __device__ __forceinline__ void wide(const Lane &, const unsigned *, int, int &, int &) {}
};

__device__ __forceinline__ void mt_score(const Lane &L, const unsigned *__restrict__ tab, int w, int wide, int base, int &fwd, int &rev) {
    if (!wide) {
        unsigned acc = 0;
        Walk<0>::packed(L, tab, w, acc);
        fwd = (int)(acc & 0xffffu) + base;
        rev = (int)(acc >> 16) + base;
    } else {
        fwd = rev = 0;
        Walk<0>::wide(L, tab, w, fwd, rev);
    }
}

// the hits of one motif at the lane's window start
__device__ __forceinline__ void mt_hits(const Lane &L, const unsigned *__restrict__ tabs, const Motif &mo, bool &hp, bool &hm, int &fwd,
                                        int &rev) {
    mt_score(L, tabs + mo.off, mo.w, mo.wide, mo.base, fwd, rev);
    const bool ok = L.run >= mo.w;
    if (mo.wide) {
        hp = ok && fwd >= mo.thr;
        hm = ok && rev >= mo.thr;
    } else {
        hp = ok && fwd - mo.base >= mo.thr;
        hm = ok && rev - mo.base >= mo.thr;
    }
}

// a workgroup's copy of its group's tables (the motifs' five numbers are read by a uniform index: scalar loads)
__device__ __forceinline__ void mt_load_group(const unsigned *__restrict__ tabs, long long tab0, int n_dwords, unsigned *__restrict__ s_tab) {
    for (int i = threadIdx.x; i < n_dwords; i += MT_BLOCK) s_tab[i] = tabs[tab0 + i];
    __syncthreads();
}

// ---- the hot loop: a wave per (run, group) ----------------------------------------------------------------------------------------
// tiles[n_tiles]: the listed tiles; run r = entries [r * rt, (r + 1) * rt).  grp_first[g] .. grp_first[g + 1]: the motifs of group g,
// grp_tab[g] .. grp_tab[g + 1]: its table dwords.  mask[t * n_groups + g] (t an index into the list) and cnt[m * n_runs + r] are written
// for every t, g, m and r.
__global__ void __launch_bounds__(MT_BLOCK) mt_scan(const u64 *__restrict__ code, const u64 *__restrict__ valid,
                                                    const int *__restrict__ tiles, long long n_tiles, int rt, long long n_runs,
                                                    const Motif *__restrict__ motifs, const int *__restrict__ grp_first,
                                                    const long long *__restrict__ grp_tab, const unsigned *__restrict__ tabs, int n_groups,
                                                    u64 *__restrict__ mask, unsigned *__restrict__ cnt) {
    extern __shared__ unsigned s_tab[];
    const int g = blockIdx.y, m0 = grp_first[g], gm = grp_first[g + 1] - m0;
    mt_load_group(tabs, grp_tab[g], (int)(grp_tab[g + 1] - grp_tab[g]), s_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * MT_WAVES + wave;
    if (r >= n_runs) return;                                       // wave-uniform, behind the only barrier
    unsigned my_cnt = 0;                                            // lane i: the hits of the group's motif i in this run
    const long long t0 = r * rt, t1 = t0 + rt < n_tiles ? t0 + rt : n_tiles;
    for (long long t = t0; t < t1; ++t) {
        const Lane L = mt_lane(code, valid, tiles[t], lane);
        u64 hit_motifs = 0;
        if (__ballot(L.run > 0)) {
            for (int i = 0; i < gm; ++i) {
                bool hp, hm;
                int fwd, rev;
                mt_hits(L, s_tab, motifs[m0 + i], hp, hm, fwd, rev);
                const u64 bp = __ballot(hp), bm = __ballot(hm);
                if (bp | bm) {                                      // rare: about 2 * 64 * p of the steps
                    hit_motifs |= 1ULL << i;
                    if (lane == i) my_cnt += (unsigned)(__popcll(bp) + __popcll(bm));
                }
            }
        }
        if (lane == 0) mask[t * n_groups + g] = hit_motifs;
    }
    if (lane < gm) cnt[(long long)(m0 + lane) * n_runs + r] = my_cnt;
}

// ---- the hits, in place: a wave per (run, group), only the marked (tile, motif) pairs ----------------------------------------------
// off[m * n_runs + r]: where the hits of motif m in run r begin (the prefix sum of cnt)
__global__ void __launch_bounds__(MT_BLOCK) mt_fill(const u64 *__restrict__ code, const u64 *__restrict__ valid,
                                                    const int *__restrict__ tiles, long long n_tiles, int rt, long long n_runs,
                                                    const Motif *__restrict__ motifs, const int *__restrict__ grp_first,
                                                    const long long *__restrict__ grp_tab, const unsigned *__restrict__ tabs, int n_groups,
                                                    const u64 *__restrict__ mask, const u64 *__restrict__ off, int *__restrict__ h_motif,
                                                    long long *__restrict__ h_start, unsigned char *__restrict__ h_strand,
                                                    int *__restrict__ h_score) {
    extern __shared__ unsigned s_tab[];
    const int g = blockIdx.y, m0 = grp_first[g], gm = grp_first[g + 1] - m0;
    mt_load_group(tabs, grp_tab[g], (int)(grp_tab[g + 1] - grp_tab[g]), s_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * MT_WAVES + wave;
    if (r >= n_runs) return;
    u64 my_off = lane < gm ? off[(long long)(m0 + lane) * n_runs + r] : 0;   // lane i: where the next hit of the group's motif i goes
    const long long t0 = r * rt, t1 = t0 + rt < n_tiles ? t0 + rt : n_tiles;
    const u64 below = lane ? ~0ULL >> (64 - lane) : 0ULL;           // the lanes before this one
    for (long long t = t0; t < t1; ++t) {
        u64 todo = mask[t * n_groups + g];                          // wave-uniform
        if (!todo) continue;
        const long long tile = tiles[t];
        const Lane L = mt_lane(code, valid, tile, lane);
        while (todo) {
            const int i = __builtin_ctzll(todo);
            todo &= todo - 1;
            bool hp, hm;
            int fwd, rev;
            mt_hits(L, s_tab, motifs[m0 + i], hp, hm, fwd, rev);
            const u64 bp = __ballot(hp), bm = __ballot(hm);
            const u64 o = __shfl(my_off, i) + (u64)(__popcll(bp & below) + __popcll(bm & below));
            if (hp) {
                h_motif[o] = m0 + i;
                h_start[o] = tile * MT_TILE + lane;
                h_strand[o] = 0;
                h_score[o] = fwd;
            }
            if (hm) {
                const u64 o2 = o + (hp ? 1 : 0);
                h_motif[o2] = m0 + i;
                h_start[o2] = tile * MT_TILE + lane;
                h_strand[o2] = 1;
                h_score[o2] = rev;
            }
            if (lane == i) my_off += (u64)(__popcll(bp) + __popcll(bm));
        }
    }
}

// ---- counts[i * n_motifs + m] = the hits of motif m with w_start[i] <= x and x + W_m <= w_end[i] --------------------------------------
// m_off[m] .. m_off[m + 1]: motif m's stretch of h_start (ascending; both strands of a site are entries of their own)
__global__ void __launch_bounds__(256) mt_counts(const long long *__restrict__ w_start, const long long *__restrict__ w_end, long long n_windows,
                                                 const int *__restrict__ widths, int n_motifs, const u64 *__restrict__ off, long long n_runs,
                                                 u64 n_hits, const long long *__restrict__ h_start, int *__restrict__ counts) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_windows * n_motifs) return;
    const long long i = k / n_motifs;
    const int m = (int)(k - i * n_motifs);
    const long long a = w_start[i], b = w_end[i] - widths[m];       // a <= x <= b
    const u64 s0 = off[(long long)m * n_runs], s1 = m + 1 < n_motifs ? off[(long long)(m + 1) * n_runs] : n_hits;
    int c = 0;
    if (b >= a && s1 > s0) {
        u64 lo = s0, hi = s1;                                       // first entry with start >= a
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            if (h_start[mid] < a) lo = mid + 1; else hi = mid;
        }
        const u64 first = lo;
        hi = s1;                                                    // first entry with start > b
        while (lo < hi) {
            const u64 mid = lo + ((hi - lo) >> 1);
            if (h_start[mid] <= b) lo = mid + 1; else hi = mid;
        }
        c = (int)(lo - first);
    }
    counts[k] = c;
}

}  // namespace natac_motifs

// ---- entry point -----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_motif_scan(natac_ctx *c, const uint8_t *seq, int64_t n, int64_t n_windows, const int64_t *start, const int64_t *end,
                     int32_t n_motifs, const int32_t *widths, const int32_t *scores, const int32_t *thresholds, int64_t *n_hits,
                     int64_t capacity, int32_t *hit_motif, int64_t *hit_start, uint8_t *hit_strand, int32_t *hit_score, int32_t *counts,
                     double *kernel_ms) {
    using namespace natac_motifs;
    static_assert(MT_MAX_WIDTH == NATAC_MOTIF_MAX_WIDTH && MT_MAX_MOTIFS == NATAC_MOTIF_MAX_MOTIFS && MT_TILE == NATAC_MOTIF_TILE &&
                      MT_RUN_TILES == NATAC_MOTIF_RUN_TILES && MT_GROUP == NATAC_MOTIF_GROUP,
                  "the kernels' sizes are in natac.h");
    static_assert(8 * MT_MAX_WIDTH <= MT_LDS_DWORDS && MT_MAX_WIDTH % MT_CHUNK == 0 && MT_CHUNK == 4, "the widest wide-arm motif fits a group");
    if (!c || !n_hits) return fail(NATAC_E_ARG, "null argument");
    if (n < 1 || n >= (1LL << 31)) return fail(NATAC_E_ARG, "n must be in [1, 2^31) (got %lld)", (long long)n);
    if (n_windows < 0 || n_motifs < 0 || capacity < 0) return fail(NATAC_E_ARG, "negative size");
    if (n_motifs > MT_MAX_MOTIFS) return fail(NATAC_E_ARG, "at most %d motifs in one call (got %d)", MT_MAX_MOTIFS, (int)n_motifs);
    if (!seq) return fail(NATAC_E_ARG, "null argument");
    if (n_windows > 0 && (!start || !end)) return fail(NATAC_E_ARG, "null argument");
    if (n_motifs > 0 && (!widths || !scores || !thresholds)) return fail(NATAC_E_ARG, "null argument");
    if (capacity > 0 && (!hit_motif || !hit_start || !hit_strand || !hit_score)) return fail(NATAC_E_ARG, "null argument");
    if (n_windows > 0 && n_motifs > 0 && !counts) return fail(NATAC_E_ARG, "null argument");
    if (n_windows > 0 && n_motifs > 0 && n_windows > (1LL << 38) / n_motifs) return fail(NATAC_E_ARG, "too many windows in one call");
    for (int64_t i = 0; i < n_windows; ++i)
        if (start[i] < 0 || end[i] < start[i] || end[i] > n)
            return fail(NATAC_E_ARG, "window %lld [%lld, %lld) outside [0, %lld)", (long long)i, (long long)start[i], (long long)end[i],
                        (long long)n);
    // the motifs: their tables, arms and groups
    std::vector<Motif> mo((size_t)n_motifs);
    std::vector<int> grp_first(1, 0);
    std::vector<long long> grp_tab(1, 0);
    std::vector<unsigned> tabs;
    {
        long long col0 = 0;
        int in_group = 0, group_dwords = 0;
        for (int m = 0; m < n_motifs; ++m) {
            const int w = widths[m];
            if (w < 1 || w > MT_MAX_WIDTH) return fail(NATAC_E_ARG, "motif %d: width must be in [1, %d] (got %d)", m, MT_MAX_WIDTH, w);
            const int32_t *S = scores + 4 * col0;
            long long lo_sum = 0, hi_sum = 0;
            int cmin[MT_MAX_WIDTH];
            for (int j = 0; j < w; ++j) {
                const int32_t *s = S + 4 * j;
                const int mn = std::min(std::min(s[0], s[1]), std::min(s[2], s[3])), mx = std::max(std::max(s[0], s[1]), std::max(s[2], s[3]));
                cmin[j] = mn;
                lo_sum += mn;
                hi_sum += mx;
            }
            if (lo_sum < INT_MIN || hi_sum > INT_MAX)
                return fail(NATAC_E_ARG, "motif %d: its score sums [%lld, %lld] leave int32", m, lo_sum, hi_sum);
            const int wide = hi_sum - lo_sum > 65535 ? 1 : 0, wp = (w + MT_CHUNK - 1) / MT_CHUNK * MT_CHUNK, dwords = (wide ? 8 : 4) * wp;
            if (in_group == MT_GROUP || group_dwords + dwords > MT_LDS_DWORDS) {
                grp_first.push_back(m);
                grp_tab.push_back((long long)tabs.size());
                in_group = group_dwords = 0;
            }
            Motif &M = mo[(size_t)m];
            M.w = w;
            M.wide = wide;
            M.off = group_dwords;
            const long long T = thresholds[m];
            if (wide) {
                M.thr = (int)T;
                M.base = 0;
                for (int j = 0; j < w; ++j) {
                    for (int b = 0; b < 4; ++b) tabs.push_back((unsigned)S[4 * j + b]);
                    for (int b = 0; b < 4; ++b) tabs.push_back((unsigned)S[4 * (w - 1 - j) + (3 - b)]);
                }
                tabs.resize(tabs.size() + (size_t)8 * (wp - w), 0u);
            } else {
                M.thr = (int)std::min<long long>(std::max<long long>(T - lo_sum, 0), 65536);
                M.base = (int)lo_sum;
                for (int j = 0; j < w; ++j)
                    for (int b = 0; b < 4; ++b)
                        tabs.push_back((unsigned)(S[4 * j + b] - cmin[j]) | ((unsigned)(S[4 * (w - 1 - j) + (3 - b)] - cmin[w - 1 - j]) << 16));
                tabs.resize(tabs.size() + (size_t)4 * (wp - w), 0u);
            }
            ++in_group;
            group_dwords += dwords;
            col0 += w;
        }
        grp_first.push_back((int)n_motifs);
        grp_tab.push_back((long long)tabs.size());
    }
    const int n_groups = (int)grp_first.size() - 1;
    long long lds_dwords = 1;
    for (int g = 0; g < n_groups; ++g) lds_dwords = std::max(lds_dwords, grp_tab[(size_t)g + 1] - grp_tab[(size_t)g]);
    const unsigned lds_bytes = (unsigned)(4 * lds_dwords);
    // behind the checks: a refused call leaves every output as it was
    *n_hits = 0;
    if (kernel_ms) *kernel_ms = 0;
    const long long n_cells = (long long)n_windows * n_motifs;
    for (long long k = 0; k < n_cells; ++k) counts[k] = 0;
    if (n_windows == 0 || n_motifs == 0) return NATAC_OK;

    // the scan intervals: the windows merged where they overlap or abut; the tiles that meet one
    std::vector<std::pair<long long, long long>> wv;
    for (int64_t i = 0; i < n_windows; ++i)
        if (end[i] > start[i]) wv.push_back({start[i], end[i]});
    std::sort(wv.begin(), wv.end());
    std::vector<long long> iv_s, iv_e;
    for (const auto &p : wv) {
        if (!iv_e.empty() && p.first <= iv_e.back()) iv_e.back() = std::max(iv_e.back(), p.second);
        else { iv_s.push_back(p.first); iv_e.push_back(p.second); }
    }
    std::vector<int> tiles;
    for (size_t k = 0; k < iv_s.size(); ++k) {
        long long t = iv_s[k] / MT_TILE;
        const long long t_last = (iv_e[k] - 1) / MT_TILE;
        if (!tiles.empty() && tiles.back() >= t) t = (long long)tiles.back() + 1;
        for (; t <= t_last; ++t) tiles.push_back((int)t);
    }
    const long long n_tiles = (long long)tiles.size();
    if (n_tiles == 0) return NATAC_OK;
    long long rt = MT_RUN_TILES, max_cells = MT_MAX_CELLS;
    if (const char *e = getenv("NATAC_MOTIF_MAX_COUNTERS")) {        // tests: longer runs on small inputs
        const long long v = atoll(e);
        if (v >= 1 && v <= MT_MAX_CELLS) max_cells = v;
    }
    while (rt < n_tiles && ((n_tiles + rt - 1) / rt) * n_motifs > max_cells) rt *= 2;
    const long long n_runs = (n_tiles + rt - 1) / rt, n_cnt = n_runs * n_motifs;
    const long long nw = (n + 63) / 64 + 2;

    DeviceCall dc(c, "motif_scan");
    const unsigned char *d_seq = dc.upload((const unsigned char *)seq, (size_t)n);
    const long long *d_ivs = dc.upload(iv_s.data(), iv_s.size()), *d_ive = dc.upload(iv_e.data(), iv_e.size());
    const long long *d_ws = dc.upload((const long long *)start, (size_t)n_windows), *d_we = dc.upload((const long long *)end, (size_t)n_windows);
    const int *d_tiles = dc.upload(tiles.data(), tiles.size()), *d_widths = dc.upload((const int *)widths, (size_t)n_motifs);
    const Motif *d_mo = dc.upload(mo.data(), mo.size());
    const int *d_gf = dc.upload(grp_first.data(), grp_first.size());
    const long long *d_gt = dc.upload(grp_tab.data(), grp_tab.size());
    const unsigned *d_tabs = dc.upload(tabs.data(), tabs.size());
    u64 *d_code = dc.alloc<u64>(2 * (size_t)nw), *d_valid = dc.alloc<u64>((size_t)nw);
    u64 *d_mask = dc.alloc<u64>((size_t)n_tiles * n_groups), *d_off = dc.alloc<u64>((size_t)n_cnt + 1);
    unsigned *d_cnt = dc.alloc<unsigned>((size_t)n_cnt);
    int *d_counts = dc.alloc<int>((size_t)n_cells);
    dc.time_begin(kernel_ms);
    const dim3 grid((unsigned)((n_runs + MT_WAVES - 1) / MT_WAVES), (unsigned)n_groups);
    if (dc.ok()) {
        hipLaunchKernelGGL(mt_pack, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, c->stream, d_seq, (long long)n, nw, d_ivs, d_ive,
                           (int)iv_s.size(), d_code, d_valid);
        hipLaunchKernelGGL(mt_scan, grid, dim3(MT_BLOCK), lds_bytes, c->stream, d_code, d_valid, d_tiles, n_tiles, (int)rt, n_runs, d_mo, d_gf, d_gt,
                           d_tabs, n_groups, d_mask, d_cnt);
        dc.launched();
    }
    dev_scan(c, d_cnt, n_cnt, d_off, dc);
    u64 total = 0;
    dc.fetch(&total, d_off + n_cnt, 1);
    if (const int rc = dc.sync()) return rc;
    if (total > 0) {
        int *d_hm = dc.alloc<int>((size_t)total), *d_hsc = dc.alloc<int>((size_t)total);
        long long *d_hs = dc.alloc<long long>((size_t)total);
        unsigned char *d_hst = dc.alloc<unsigned char>((size_t)total);
        if (dc.ok()) {
            hipLaunchKernelGGL(mt_fill, grid, dim3(MT_BLOCK), lds_bytes, c->stream, d_code, d_valid, d_tiles, n_tiles, (int)rt, n_runs, d_mo, d_gf, d_gt,
                               d_tabs, n_groups, d_mask, d_off, d_hm, d_hs, d_hst, d_hsc);
            hipLaunchKernelGGL(mt_counts, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, c->stream, d_ws, d_we, (long long)n_windows,
                               d_widths, (int)n_motifs, d_off, n_runs, total, d_hs, d_counts);
            dc.launched();
        }
        dc.time_end();
        dc.fetch(counts, d_counts, (size_t)n_cells);
        if ((long long)total <= capacity) {              // too many for the caller's arrays: they stay as they were, the count says so
            dc.fetch(hit_motif, d_hm, (size_t)total);
            dc.fetch(hit_start, d_hs, (size_t)total);
            dc.fetch(hit_strand, d_hst, (size_t)total);
            dc.fetch(hit_score, d_hsc, (size_t)total);
        }
    } else {
        dc.time_end();
    }
    if (const int rc = dc.finish()) return rc;
    *n_hits = (int64_t)total;
    return NATAC_OK;
}

}  // extern "C"
