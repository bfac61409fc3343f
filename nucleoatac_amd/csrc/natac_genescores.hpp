// natac_genescores.hpp -- the kernels behind `pyatac genescores` (this package's own command: the reference has no such tool): the
// gene-by-cell matrix of distance-weighted insertion sums of one chromosome, CSR with one row per gene (natac_gene_cell_scores,
// include/natac.h states the rule), and the host-only launch plan (natac_gene_cell_scores_plan).
//
// A gene is a window [win_lo, win_hi) around a body [body_lo, body_hi).  An insertion x of a record that passes the size filter counts
// when win_lo <= x < win_hi; its distance d is 0 inside the body, body_lo - x to the left of it and x - body_hi + 1 to the right, and it
// adds weight[d] to entry (gene, cell).  That rule is gs_record_weights, the one function every kernel here asks.
//
// The candidates of a row are one contiguous range of records: natac_sites.hpp's natac_region_ranges with start = win_lo, end = win_hi
// and the ATAC shift.  gs_count_hits gives every row its number of counting insertions h (one wave per row); the entry checks
// h * max(weight) < 2^31 on the host, so that no 32-bit sum below can wrap, and picks every row's arm (gs_plan):
//   gs_rows_wave    h <= short_max (at most 64: one key per lane): one wave per row.  The (cell, weight) pairs are gathered through 2 x 64
//                   words of LDS per wave, sorted by cell by a bitonic network over the lanes with the weight travelling along; run heads
//                   come from one ballot and a run's sum from a segmented cross-lane scan.
//   gs_rows_table   every other row: one workgroup of 256 threads per (row, cell tile) with a grid stride.  The tile's cells have one
//                   32-bit counter each in LDS (at most 16,384: 64 KiB, two workgroups a CU), zeroed once per workgroup.  The threads walk
//                   the row's candidates with a workgroup stride and add a record's weights with an integer LDS atomic; then every thread
//                   scans its contiguous run of the tile's words, a block scan of the non-zero counts places the (cell, value) pairs in
//                   ascending order, and zeros go back as the words are read.
// Both kernels run twice, a count pass (fill == 0: the pairs of every (row, tile) are counted) and, after a scan of those counts, a fill
// pass that writes the pairs at their place in col / val.  There is no staging area: a row of a 200 kb window reaches most cells, and a
// staging area sized by min(h, n_cells) a row would hold 5,000 genes x 10,000 cells x 8 bytes for one chromosome; walking a row's
// candidates a second time reads some hundred KiB that the first walk left in the L2.
// Integers only: no floating point, no global atomics on the sums, no scratch.  A row's layout is fixed by the cell order, not by the
// order of records, waves or workgroups: the result is a pure function of the inputs under every short_max and tile.
// Behind the kernels: the plan and the entry points.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "natac_sites.hpp"

namespace natac_gs {

typedef unsigned long long u64;

constexpr int GS_WG = 256;                  // 4 waves
constexpr int GS_SHORT_MAX = 64;            // NATAC_GENESCORES_SHORT_CAP: one key per lane
constexpr int GS_TILE_CAP = 16384;          // NATAC_GENESCORES_TILE_CAP: 64 KiB of 32-bit counters
constexpr int GS_MIN_TILE = 16;
constexpr int GS_MAX_WEIGHT = 1 << 20;      // NATAC_GENESCORES_MAX_WEIGHT
constexpr int GS_MAX_NW = (1 << 20) + 1;
constexpr int GS_SHIFT = 4, GS_TRIM = 8;    // the ATAC offsets
constexpr unsigned GS_PAD = 0xffffffffu;    // sorts behind every cell index

struct GsArgs {
    const long long *pos, *tlen;   // [n_frags]
    const int *cell;               // [n_frags]
    const long long *win_lo, *win_hi, *body_lo, *body_hi;      // [n_genes]
    const long long *cand_lo, *cand_n;                         // [n_genes]: natac_region_ranges
    const int *weight;             // [n_w]
    int lower, upper;
};

__device__ __forceinline__ u64 gs_lanes_below(int lane) { return (1ULL << lane) - 1ULL; }

// THE RULE for one insertion x: its weight, 0 when it does not count (every weight of the table is at least 1)
template <bool LOOKUP>
__device__ __forceinline__ int gs_insertion_weight(long long x, long long wl, long long wh, long long bs, long long be,
                                                   const int *__restrict__ weight) {
    if (x < wl || x >= wh) return 0;
    if (!LOOKUP) return 1;
    const long long d = x < bs ? bs - x : (x >= be ? x - be + 1 : 0);
    return weight[d];
}

// THE RULE for one record (pos p, tlen t): the weights of its two insertions l = p + 4 and r = l + ilen - 1, ilen = t - 8; both 0 when
// the size filter drops the record.  LOOKUP == false answers 1 for an insertion that counts (the counting pass).
template <bool LOOKUP>
__device__ __forceinline__ void gs_record_weights(long long p, long long t, long long wl, long long wh, long long bs, long long be, int lower,
                                                  int upper, const int *__restrict__ weight, int &w_left, int &w_right) {
    const long long n = t - GS_TRIM, l = p + GS_SHIFT, r = l + n - 1;
    const bool sized = n >= lower && n < upper;
    w_left = sized ? gs_insertion_weight<LOOKUP>(l, wl, wh, bs, be, weight) : 0;
    w_right = sized ? gs_insertion_weight<LOOKUP>(r, wl, wh, bs, be, weight) : 0;
}

// hits[i] = the counting insertions of row i: one wave per row
__global__ void __launch_bounds__(GS_WG) gs_count_hits(GsArgs A, long long nr, u64 *__restrict__ hits) {
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * (GS_WG / 64);
    for (long long i = (long long)blockIdx.x * (GS_WG / 64) + (threadIdx.x >> 6); i < nr; i += nwaves) {
        const long long f0 = A.cand_lo[i], f1 = f0 + A.cand_n[i];
        const long long wl = A.win_lo[i], wh = A.win_hi[i], bs = A.body_lo[i], be = A.body_hi[i];
        u64 n = 0;
        for (long long f = f0 + lane; f < f1; f += 64) {
            int a, b;
            gs_record_weights<false>(A.pos[f], A.tlen[f], wl, wh, bs, be, A.lower, A.upper, A.weight, a, b);
            n += (u64)(a + b);
        }
        for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
        if (lane == 0) hits[i] = n;
    }
}

// ---- short arm: rows of 1 .. short_max hits, one wave each ----
// fill == 0: cnt[i * n_tiles] = the row's pairs.  fill != 0: the pairs go to col / val at off[i * n_tiles].
__global__ void __launch_bounds__(GS_WG) gs_rows_wave(GsArgs A, long long nr, const u64 *__restrict__ hits, int short_max, int n_tiles, int fill,
                                                      u64 *__restrict__ cnt, const u64 *__restrict__ off, int *__restrict__ col,
                                                      int *__restrict__ val) {
    __shared__ unsigned s_key[GS_WG / 64][64], s_wt[GS_WG / 64][64];
    const int lane = threadIdx.x & 63;
    volatile unsigned *keys = s_key[threadIdx.x >> 6], *wts = s_wt[threadIdx.x >> 6];     // this wave's own words
    const long long nwaves = (long long)gridDim.x * (GS_WG / 64);
    for (long long i = (long long)blockIdx.x * (GS_WG / 64) + (threadIdx.x >> 6); i < nr; i += nwaves) {
        const u64 h = hits[i];
        if (h == 0 || h > (u64)short_max) continue;
        const long long f0 = A.cand_lo[i], f1 = f0 + A.cand_n[i];
        const long long wl = A.win_lo[i], wh = A.win_hi[i], bs = A.body_lo[i], be = A.body_hi[i];
        unsigned base = 0;
        for (long long f = f0; f < f1; f += 64) {           // wave-uniform bounds: every lane takes part in every ballot
            int a = 0, b = 0;
            unsigned c = 0;
            if (f + lane < f1) {
                gs_record_weights<true>(A.pos[f + lane], A.tlen[f + lane], wl, wh, bs, be, A.lower, A.upper, A.weight, a, b);
                c = (unsigned)A.cell[f + lane];
            }
            const u64 ma = __ballot(a != 0), mb = __ballot(b != 0), below = gs_lanes_below(lane);
            unsigned r = base + (unsigned)__popcll(ma & below) + (unsigned)__popcll(mb & below);
            if (a != 0) {
                if (r < 64u) { keys[r] = c; wts[r] = (unsigned)a; }
                ++r;
            }
            if (b != 0 && r < 64u) { keys[r] = c; wts[r] = (unsigned)b; }
            base += (unsigned)__popcll(ma) + (unsigned)__popcll(mb);
        }
        __builtin_amdgcn_wave_barrier();
        unsigned key = (u64)lane < h ? keys[lane] : GS_PAD;
        unsigned w = (u64)lane < h ? wts[lane] : 0u;
        __builtin_amdgcn_wave_barrier();                    // the next row writes the same words
        for (int k = 2; k <= 64; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const unsigned ok = (unsigned)__shfl_xor((int)key, j), ow = (unsigned)__shfl_xor((int)w, j);
                const bool up = (lane & k) == 0, low = (lane & j) == 0;
                const bool take = (low == up) ? !(key < ok) : !(key > ok);      // equal keys: both lanes take the other's pair
                key = take ? ok : key;
                w = take ? ow : w;
            }
        const unsigned prev = (unsigned)__shfl_up((int)key, 1);
        const bool head = (u64)lane < h && (lane == 0 || key != prev);
        const u64 hm = __ballot(head);
        // the start of this lane's run, then an inclusive scan that never reaches below it
        const int start = 63 - __builtin_clzll((hm & (gs_lanes_below(lane) | (1ULL << lane))) | 1ULL);
        unsigned sum = w;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = (unsigned)__shfl_up((int)sum, o);
            if (lane - o >= start) sum += v;
        }
        const u64 rest = lane < 63 ? hm >> (lane + 1) : 0ULL;
        const int next = rest ? lane + 1 + __builtin_ctzll(rest) : (int)h;     // where the next run starts
        const unsigned total = (unsigned)__shfl((int)sum, (next - 1) & 63);
        if (!fill) {
            if (lane == 0) cnt[i * n_tiles] = (u64)__popcll(hm);
        } else if (head) {
            const u64 o = off[i * n_tiles] + (u64)__popcll(hm & gs_lanes_below(lane));
            col[o] = (int)key;
            val[o] = (int)total;
        }
    }
}

// ---- table arm: the rows of list[n_list], one workgroup per (row, tile) with a grid stride ----
// s_tab[tile] is the dynamic LDS.  fill == 0: cnt[row * n_tiles + t] = the pairs of the tile.  fill != 0: they go to off[row * n_tiles + t].
__global__ void __launch_bounds__(GS_WG) gs_rows_table(GsArgs A, const long long *__restrict__ list, long long n_list, int n_cells, int tile,
                                                       int n_tiles, int fill, u64 *__restrict__ cnt, const u64 *__restrict__ off,
                                                       int *__restrict__ col, int *__restrict__ val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_lds[];
    unsigned *s_tab = (unsigned *)gs_lds;
    __shared__ unsigned s_w[GS_WG / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = tile >= GS_WG ? tile / GS_WG : 1;       // words of a thread's run (tile is a power of two)
    const int w0 = tid * per, w1 = min(w0 + per, tile);     // w0 >= tile: a thread without words
    for (int q = tid; q < tile; q += GS_WG) s_tab[q] = 0;
    __syncthreads();
    const long long items = n_list * n_tiles;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {                 // workgroup-uniform
        const long long i = list[it / n_tiles];
        const int t = (int)(it % n_tiles);
        const int c0 = t * tile, c1 = min(n_cells, c0 + tile);
        const long long f0 = A.cand_lo[i], f1 = f0 + A.cand_n[i];
        const long long wl = A.win_lo[i], wh = A.win_hi[i], bs = A.body_lo[i], be = A.body_hi[i];
        for (long long f = f0 + tid; f < f1; f += GS_WG) {
            const int c = A.cell[f];
            if (c < c0 || c >= c1) continue;
            int a, b;
            gs_record_weights<true>(A.pos[f], A.tlen[f], wl, wh, bs, be, A.lower, A.upper, A.weight, a, b);
            if (a + b) atomicAdd(&s_tab[c - c0], (unsigned)(a + b));
        }
        __syncthreads();
        unsigned n = 0;
        for (int q = w0; q < w1; ++q) {
            n += s_tab[q] != 0;
            if (!fill) s_tab[q] = 0;
        }
        unsigned inc = n;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = (unsigned)__shfl_up((int)inc, o);
            if (lane >= o) inc += v;
        }
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        if (!fill) {
            if (tid == 0) cnt[i * n_tiles + t] = (u64)s_w[0] + s_w[1] + s_w[2] + s_w[3];
        } else {
            u64 o = off[i * n_tiles + t] + (inc - n);
            for (int q = 0; q < wv; ++q) o += s_w[q];
            for (int q = w0; q < w1; ++q) {
                const unsigned v = s_tab[q];
                if (v) {
                    col[o] = c0 + q;
                    val[o] = (int)v;
                    ++o;
                    s_tab[q] = 0;
                }
            }
        }
        __syncthreads();                                    // zeros and s_w before the next item
    }
}

// how a call launches: what natac_gene_cell_scores runs and natac_gene_cell_scores_plan reports
struct GsPlan {
    int short_max;                 // rows of at most this many hits take the short arm
    int tile, n_tiles;             // cells of a table tile (a power of two) and ceil(n_cells / tile)
    int wg;                        // threads of a workgroup
    long long lds;                 // dynamic LDS of a table workgroup, bytes: 4 tile
    int grid;                      // the most workgroups the table kernel is launched with
};

static int gs_env(const char *name, long long lo, long long hi, int dflt) {
    if (const char *e = getenv(name)) {
        const long long v = atoll(e);
        if (v >= lo && v <= hi) return (int)v;
    }
    return dflt;
}

// for n_cells cells and n_cu compute units.  The default tile is the least power of two that holds all cells, between one word a thread
// and the cap: a small matrix leaves the LDS to more workgroups.
static void gs_plan(long long n_cells, int n_cu, GsPlan *p) {
    p->short_max = gs_env("NATAC_GENESCORES_SHORT_MAX", 1, GS_SHORT_MAX, GS_SHORT_MAX);
    int dflt = GS_WG;
    while (dflt < GS_TILE_CAP && dflt < n_cells) dflt <<= 1;
    p->tile = gs_env("NATAC_GENESCORES_TILE", GS_MIN_TILE, GS_TILE_CAP, dflt);
    if (p->tile & (p->tile - 1)) p->tile = dflt;            // not a power of two: not taken
    p->n_tiles = (int)((n_cells + p->tile - 1) / p->tile);
    p->wg = GS_WG;
    p->lds = (long long)p->tile * 4;
    p->grid = 8 * n_cu;
}

}  // namespace natac_gs

// ---- entry points ----------------------------------------------------------------------------------------------------------------
extern "C" {

int natac_gene_cell_scores(natac_ctx *c, int64_t nf, const int64_t *pos, const int64_t *tlen, const int32_t *cell, int32_t n_cells, int64_t ng,
                           const int64_t *win_lo, const int64_t *win_hi, const int64_t *body_lo, const int64_t *body_hi, int32_t n_w,
                           const int32_t *weight, int lower, int upper, int64_t *row_ptr, int64_t cap, int32_t *col, int32_t *val,
                           int64_t *hits, int64_t *arm_rows, double *kernel_ms) {
    using namespace natac_gs;
    static_assert(GS_SHORT_MAX == NATAC_GENESCORES_SHORT_CAP && GS_TILE_CAP == NATAC_GENESCORES_TILE_CAP &&
                      GS_MAX_WEIGHT == NATAC_GENESCORES_MAX_WEIGHT,
                  "the limits are in natac.h");
    if (!c || !row_ptr || !weight) return fail(NATAC_E_ARG, "null argument");
    if (nf < 0 || ng < 0 || cap < 0) return fail(NATAC_E_ARG, "negative size");
    if ((nf > 0 && (!pos || !tlen || !cell)) || (ng > 0 && (!win_lo || !win_hi || !body_lo || !body_hi))) return fail(NATAC_E_ARG, "null argument");
    if (!col != !val || (!col && cap != 0)) return fail(NATAC_E_ARG, "col and val go together; a sizing call passes neither and cap 0");
    if (n_cells < 1 || n_cells > NATAC_SPLIT_MAX_BARCODES) return fail(NATAC_E_ARG, "n_cells must be in [1, %d] (got %d)", NATAC_SPLIT_MAX_BARCODES, n_cells);
    if (lower < 0 || upper <= lower || upper > 50000) return fail(NATAC_E_ARG, "0 <= lower < upper <= 50000 (got lower %d, upper %d)", lower, upper);
    if (n_w < 1 || n_w > GS_MAX_NW) return fail(NATAC_E_ARG, "n_w must be in [1, %d] (got %d)", GS_MAX_NW, n_w);
    if (nf >= (1LL << 40) || ng >= (1LL << 40)) return fail(NATAC_E_ARG, "too many records or genes in one call");
    long long w_max = 0;
    for (int32_t d = 0; d < n_w; ++d) {
        if (weight[d] < 1 || weight[d] > GS_MAX_WEIGHT) return fail(NATAC_E_ARG, "weight[%d] = %d outside [1, %d]", d, weight[d], GS_MAX_WEIGHT);
        w_max = std::max<long long>(w_max, weight[d]);
    }
    for (int64_t i = 0; i < ng; ++i) {
        if (win_lo[i] < -COORD_LIM || win_hi[i] > COORD_LIM) return fail(NATAC_E_ARG, "gene %lld: coordinates out of range", (long long)i);
        if (!(win_lo[i] <= body_lo[i] && body_lo[i] <= body_hi[i] && body_hi[i] <= win_hi[i]))
            return fail(NATAC_E_ARG, "gene %lld: win_lo <= body_lo <= body_hi <= win_hi does not hold (%lld, %lld, %lld, %lld)", (long long)i,
                        (long long)win_lo[i], (long long)body_lo[i], (long long)body_hi[i], (long long)win_hi[i]);
        if (body_lo[i] - win_lo[i] >= n_w || win_hi[i] - body_hi[i] >= n_w)
            return fail(NATAC_E_ARG, "gene %lld: the window reaches %lld bases left and %lld right of the body, the table has %d weights", (long long)i,
                        (long long)(body_lo[i] - win_lo[i]), (long long)(win_hi[i] - body_hi[i]), n_w);
    }
    if (const int rc = check_fragments(nf, pos, tlen, cell, n_cells)) return rc;
    if (kernel_ms) *kernel_ms = 0;
    if (ng == 0 || nf == 0) {
        for (int64_t i = 0; i <= ng; ++i) row_ptr[i] = 0;
        if (hits) std::fill(hits, hits + ng, (int64_t)0);
        if (arm_rows) arm_rows[0] = arm_rows[1] = 0;
        return NATAC_OK;
    }
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device);     // 256 stands if the query fails
    GsPlan plan;
    gs_plan(n_cells, n_cu, &plan);
    const int T = plan.n_tiles;
    if ((unsigned __int128)ng * (unsigned)T >= ((unsigned __int128)1 << 40)) return fail(NATAC_E_ARG, "too many (gene, tile) pairs in one call");

    DeviceCall dc(c, "gene_cell_scores");
    GsArgs A;
    A.pos = dc.upload((const long long *)pos, (size_t)nf);
    A.tlen = dc.upload((const long long *)tlen, (size_t)nf);
    A.cell = dc.upload((const int *)cell, (size_t)nf);
    A.win_lo = dc.upload((const long long *)win_lo, (size_t)ng);
    A.win_hi = dc.upload((const long long *)win_hi, (size_t)ng);
    A.body_lo = dc.upload((const long long *)body_lo, (size_t)ng);
    A.body_hi = dc.upload((const long long *)body_hi, (size_t)ng);
    A.weight = dc.upload((const int *)weight, (size_t)n_w);
    A.lower = lower;
    A.upper = upper;
    long long *d_lo = dc.alloc<long long>((size_t)ng), *d_n = dc.alloc<long long>((size_t)ng), *d_long = dc.alloc<long long>((size_t)ng);
    u64 *d_hits = dc.zeroed<u64>((size_t)ng + 1);           // hits[ng], then natac_region_ranges' long-region count (not used here)
    A.cand_lo = d_lo;
    A.cand_n = d_n;
    const unsigned bx_wave = (unsigned)std::min<long long>((ng + GS_WG / 64 - 1) / (GS_WG / 64), 16384);
    dc.time_begin(kernel_ms);
    // (1) candidates and hits per row
    if (dc.ok()) {
        const unsigned bx = (unsigned)std::min<long long>((ng + natac_sites::RC_BLOCK - 1) / natac_sites::RC_BLOCK, 4096);
        hipLaunchKernelGGL(natac_sites::natac_region_ranges, dim3(bx), dim3(natac_sites::RC_BLOCK), 0, c->stream, A.pos, (long long)nf, (long long)ng,
                           A.win_lo, A.win_hi, lower, upper, GS_SHIFT, d_lo, d_n, d_long, d_hits + ng);
        hipLaunchKernelGGL(gs_count_hits, dim3(bx_wave), dim3(GS_WG), 0, c->stream, A, (long long)ng, d_hits);
        dc.launched();
    }
    std::vector<u64> h_hits((size_t)ng);
    dc.fetch(h_hits.data(), d_hits, (size_t)ng);
    if (const int rc = dc.sync()) return rc;
    // (2) the one bound that needs the device, and every row's arm
    std::vector<long long> table_rows;
    long long n_short = 0;
    for (int64_t i = 0; i < ng; ++i) {
        const u64 h = h_hits[(size_t)i];
        if ((unsigned __int128)h * (unsigned __int128)w_max >= ((unsigned __int128)1 << 31))
            return fail(NATAC_E_ARG, "gene %lld: %llu insertions count and the largest weight is %lld: an entry could reach 2^31", (long long)i, h, w_max);
        if (h > (u64)plan.short_max) table_rows.push_back(i);
        else if (h > 0) ++n_short;
    }
    const long long n_items = (long long)ng * T;
    u64 *d_cnt = dc.zeroed<u64>((size_t)n_items);
    u64 *d_off = dc.alloc<u64>((size_t)n_items + 1);
    const long long *d_list = table_rows.empty() ? nullptr : dc.upload(table_rows.data(), table_rows.size());
    const unsigned bx_table = (unsigned)std::min<long long>((long long)table_rows.size() * T, plan.grid);
    if (!table_rows.empty() && plan.lds >= 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)gs_rows_table, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
    auto pass = [&](int fill, int *d_col, int *d_val) {
        if (!dc.ok()) return;
        if (n_short)
            hipLaunchKernelGGL(gs_rows_wave, dim3(bx_wave), dim3(GS_WG), 0, c->stream, A, (long long)ng, d_hits, plan.short_max, T, fill, d_cnt, d_off,
                               d_col, d_val);
        if (!table_rows.empty())
            hipLaunchKernelGGL(gs_rows_table, dim3(bx_table), dim3(GS_WG), (size_t)plan.lds, c->stream, A, d_list, (long long)table_rows.size(),
                               (int)n_cells, plan.tile, T, fill, d_cnt, d_off, d_col, d_val);
        dc.launched();
    };
    // (3) the count pass, and row_ptr = every T-th element of the scan of the (row, tile) counts
    pass(0, nullptr, nullptr);
    dev_scan(c, d_cnt, n_items, d_off, dc);
    std::vector<u64> h_off((size_t)n_items + 1);
    dc.fetch(h_off.data(), d_off, (size_t)n_items + 1);
    if (const int rc = dc.sync()) return rc;
    for (int64_t i = 0; i <= ng; ++i) row_ptr[i] = (int64_t)h_off[(size_t)i * T];
    if (hits) std::copy(h_hits.begin(), h_hits.end(), (u64 *)hits);
    if (arm_rows) {
        arm_rows[0] = n_short;
        arm_rows[1] = (int64_t)table_rows.size();
    }
    const int64_t nnz = row_ptr[ng];
    if (!col || nnz > cap) {
        dc.time_end();
        const int rc = dc.finish();
        if (rc) return rc;
        if (!col) return NATAC_OK;                          // the sizing call
        return fail(NATAC_E_ARG, "cap %lld is less than the %lld entries of the matrix", (long long)cap, (long long)nnz);
    }
    // (4) the fill pass
    int *d_col = dc.alloc<int>((size_t)nnz), *d_val = dc.alloc<int>((size_t)nnz);
    if (nnz) pass(1, d_col, d_val);
    dc.time_end();
    dc.fetch(col, d_col, (size_t)nnz);
    dc.fetch(val, d_val, (size_t)nnz);
    return dc.finish();
}

int natac_gene_cell_scores_plan(int64_t n_genes, int32_t n_cells, int64_t table_rows, int32_t n_cu, int32_t *short_max, int32_t *tile,
                                int32_t *n_tiles, int32_t *wg, int64_t *lds_bytes, int32_t *grid) {
    using namespace natac_gs;
    if (!short_max || !tile || !n_tiles || !wg || !lds_bytes || !grid) return fail(NATAC_E_ARG, "null argument");
    if (n_genes < 1 || n_genes >= (1LL << 40) || n_cells < 1 || n_cells > NATAC_SPLIT_MAX_BARCODES || table_rows < 0 || table_rows > n_genes ||
        n_cu < 1)
        return fail(NATAC_E_ARG, "natac_gene_cell_scores_plan: n_genes in [1, 2^40), n_cells in [1, %d], table_rows in [0, n_genes], n_cu >= 1",
                    NATAC_SPLIT_MAX_BARCODES);
    GsPlan p;
    gs_plan(n_cells, n_cu, &p);
    *short_max = p.short_max;
    *tile = p.tile;
    *n_tiles = p.n_tiles;
    *wg = p.wg;
    *lds_bytes = p.lds;
    *grid = (int32_t)std::min<long long>(table_rows * p.n_tiles, p.grid);
    return NATAC_OK;
}

}  // extern "C"
