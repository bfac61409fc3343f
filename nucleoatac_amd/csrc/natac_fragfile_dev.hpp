// natac_fragfile_dev.hpp -- BGZF fragment file -> fragment arrays on the GPU.
//
// The members are found, staged and inflated exactly as for a BAM (natac_bam_dev.hpp: walk_chain, two pinned staging buffers,
// bamdev_inflate with its CRC check).  What follows the inflate differs: a window's inflated bytes are TEXT, and a line may start
// anywhere and straddle any number of members, so nothing here works per member.  On the window's contiguous text:
//   (a) frag_count_nl / frag_scan / frag_line_starts: every lane loads 16 bytes and builds a newline mask; the per-tile counts are
//       scanned and become the offsets at which the lanes write the line starts.
//   (b) frag_parse: one lane per line runs natac_fragio::parse_line (the host decoder's own classifier) and compares the line's
//       chromosome field byte-wise with the previous data line's: a difference starts a RUN.
//   (c) frag_compact: a scan over (is data, starts a run) gives every data line its output slot and its run; start / end are
//       written in file order, and per run its first slot, the offset and length of its name and its largest end.
// The host reads the few run names back (frag_gather_names), maps them to chromosome ids with the host decoder's dictionary (this is
// where a chromosome that comes back gets its old id) and appends.  The bytes behind a window's last '\n' are carried to the front
// of the next window.  Every device read is bounded by the window's length n, whatever the text holds.
// Splitting by cell barcode (natac_frag_split_device; decode_device with a SplitJob) keeps (a) and runs its own kernels behind it:
//   (b') frag_split_parse: frag_parse with natac_fragio::split_line, so every data line also gets its group (or -1) from the barcode
//        table, and the exact per-barcode counts grow by one integer atomic per set of lanes of a wave that share a barcode.
//   (c') frag_split_compact: the run tables over ALL data lines as in (c), and every line's run instead of the compacted start / end.
//   (d') frag_split_hist / frag_scan / frag_split_scatter: a stable partition of the window's assigned lines by group.  One wave owns a
//        tile of PART_LINES consecutive lines; the per-tile counts, stored group-major, scan into every (group, tile)'s first output
//        slot; the wave then walks its tile in file order, 64 lines a round, and gives the lanes of a group consecutive slots in lane
//        order.  The counts of every (group, run) segment come from the same histogram.  Integers only: nothing depends on order.
//   The host gets start / end of the assigned lines only, in group-major order, and the segment counts, and appends segment by segment.
// Discovering the cells (natac_frag_cells_device; decode_device with a CellsJob) keeps (a) too and needs no runs: cells_parse, rounds of
// cells_claim / cells_verify, cells_number / cells_adopt and cells_count build the barcode table from the file itself (see CellsJob below).
// The host decoder answers instead (the caller runs it) for: a malformed line or a damaged file (so both paths give the same message
// by construction), a window without any line end, more than MAX_RUNS runs in a window, a HIP failure;
// when splitting also for a line without a barcode field (malformed), a table of more than SPLIT_DEV_MAX_BARCODES barcodes and more than
// SPLIT_MAX_SEGMENTS groups x runs in a window; when discovering cells for a line without a barcode field, a full table (more than half
// the slots taken: more than SPLIT_DEV_MAX_BARCODES cells with the default size) and more than 268,435,455 lines in a window.
#pragma once
#include "natac_bam_dev.hpp"
#include "natac_fragfile.hpp"

namespace natac_fragdev {

using natac_bamdev::Chain;
using natac_bamdev::DevBuf;
using natac_bamdev::Member;
typedef unsigned long long u64;

constexpr int TILE_T = 256;                 // lanes per workgroup
constexpr int TILE_B = 16 * TILE_T;         // text bytes per workgroup in (a)
constexpr unsigned int MAX_RUNS = 65536;    // per window
constexpr int PART_T = 64;                  // one wave per partition tile: no barrier between the waves of a tile is ever needed
constexpr int PART_LINES = 8192;            // lines per partition tile: 10 M lines are ~1,200 tiles, x 255 groups ~311 k counters to scan
constexpr u64 SPLIT_MAX_SEGMENTS = 1u << 20;            // groups x runs per window (include/natac.h states it)
constexpr long long SPLIT_DEV_MAX_BARCODES = 1 << 22;   // the table on the device: <= 32 MiB of slots, <= 1 GiB of bytes

// exclusive prefix sum of v over the workgroup (blockDim.x a multiple of 64, at most 1024); *total = the workgroup's sum
__device__ __forceinline__ u64 block_excl_scan(u64 v, u64 *total) {
    __shared__ u64 wsum[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    __syncthreads();                        // (a second call in one kernel: the sums of the first are no longer read)
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    u64 before = 0, all = 0;
    for (int k = 0; k < nw; ++k) { const u64 s = wsum[k]; if (k < w) before += s; all += s; }
    *total = all;
    return before + inc - v;
}

// newline mask of the 16 bytes at `base` (a multiple of 16; the buffer is readable up to the next multiple of 16 behind n)
__device__ __forceinline__ unsigned int nl_mask16(const unsigned char *__restrict__ data, u64 base, u64 n) {
    if (base >= n) return 0u;
    const uint4 q = *(const uint4 *)(data + base);
    const unsigned int w[4] = {q.x, q.y, q.z, q.w};
    unsigned int m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) m |= (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) == 10u ? 1u : 0u) << k;
    if (n - base < 16) m &= (1u << (unsigned int)(n - base)) - 1u;
    return m;
}

__global__ void __launch_bounds__(TILE_T) frag_count_nl(const unsigned char *__restrict__ data, u64 n, u64 *__restrict__ tile_cnt) {
    const u64 base = ((u64)blockIdx.x * TILE_T + threadIdx.x) * 16;
    u64 total;
    block_excl_scan((u64)__popc(nl_mask16(data, base, n)), &total);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

// exclusive scan of a[0, count) in place, one workgroup of 1024 (count is a number of TILES or of workgroups: a few hundred thousand
// at most); *total = the sum.  Values that pack two 32-bit counters scan as two sums.
__global__ void __launch_bounds__(1024) frag_scan(u64 *__restrict__ a, u64 count, u64 *__restrict__ total) {
    const u64 per = (count + 1023) / 1024, lo = min(count, per * threadIdx.x), hi = min(count, lo + per);
    u64 s = 0;
    for (u64 i = lo; i < hi; ++i) s += a[i];
    u64 all;
    u64 run = block_excl_scan(s, &all);
    for (u64 i = lo; i < hi; ++i) { const u64 v = a[i]; a[i] = run; run += v; }
    if (threadIdx.x == 0) *total = all;
}

// ls[1 + k] = offset behind the k-th '\n' (ls[0] = 0 is the host's); cap = number of '\n' counted
__global__ void __launch_bounds__(TILE_T) frag_line_starts(const unsigned char *__restrict__ data, u64 n, const u64 *__restrict__ tile_off, u64 cap,
                                                           u64 *__restrict__ ls) {
    const u64 base = ((u64)blockIdx.x * TILE_T + threadIdx.x) * 16;
    unsigned int m = nl_mask16(data, base, n);
    u64 total;
    u64 k = tile_off[blockIdx.x] + block_excl_scan((u64)__popc(m), &total);
    while (m) {
        const int b = __ffs(m) - 1;
        m &= m - 1;
        if (k < cap) ls[1 + k] = base + (u64)b + 1;
        ++k;
    }
}

// line i = data[ls[i], ls[i + 1] - 1) without the '\r' before its '\n'; open_tail: the last line has no '\n' (ls[n_lines] = n + 1)
__device__ __forceinline__ void line_span(const unsigned char *__restrict__ data, const u64 *__restrict__ ls, u64 i, u64 n_lines, int open_tail, u64 *a, u64 *e) {
    *a = ls[i];
    *e = ls[i + 1] - 1;
    if (!(open_tail && i + 1 == n_lines) && *e > *a && data[*e - 1] == '\r') --*e;
}

// does data line i (at a, chromosome field of nlen bytes) start a run: is there no data line before it, or one of another chromosome
__device__ __forceinline__ bool starts_run(const unsigned char *__restrict__ data, const u64 *__restrict__ ls, u64 i, u64 n_lines, int open_tail, u64 a,
                                           uint32_t nlen) {
    bool differs = true;
    for (u64 j = i; j-- > 0;) {                          // the previous line that is not skipped
        u64 pa, pe;
        line_span(data, ls, j, n_lines, open_tail, &pa, &pe);
        if (pe == pa || data[pa] == '#') continue;
        differs = pe - pa <= nlen || data[pa + nlen] != '\t';
        for (uint32_t k = 0; k < nlen && !differs; ++k) differs = data[pa + k] != data[a + k];
        break;
    }
    return differs;
}

// code[i] = (is data) << 32 | (starts a run); status[0] |= 1 for a malformed line
__global__ void __launch_bounds__(TILE_T) frag_parse(const unsigned char *__restrict__ data, const u64 *__restrict__ ls, u64 n_lines, int open_tail,
                                                     u64 *__restrict__ code, int *__restrict__ start, int *__restrict__ end, unsigned int *__restrict__ name_len,
                                                     u64 *__restrict__ block_sum, int *__restrict__ status) {
    const u64 i = (u64)blockIdx.x * TILE_T + threadIdx.x;
    u64 c = 0;
    if (i < n_lines) {
        u64 a, e;
        line_span(data, ls, i, n_lines, open_tail, &a, &e);
        uint32_t nlen = 0;
        int32_t s = 0, t = 0;
        const int kind = natac_fragio::parse_line(data + a, (size_t)(e - a), &nlen, &s, &t);
        if (kind > natac_fragio::LINE_DATA) atomicOr(&status[0], 1);
        if (kind == natac_fragio::LINE_DATA) {
            const bool differs = starts_run(data, ls, i, n_lines, open_tail, a, nlen);
            c = (1ull << 32) | (differs ? 1ull : 0ull);
            start[i] = s;
            end[i] = t;
            name_len[i] = nlen;
        }
        code[i] = c;
    }
    u64 total;
    block_excl_scan(c, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// block_off = the scanned block_sum.  Data line -> slot d (file order), run r; per run: first slot, name offset / length, largest end
// (SPLIT: line_run[i] = the run of line i, -1 for a line that is no data line, instead of o_start / o_end)
template <bool SPLIT>
__device__ __forceinline__ void compact_body(const u64 *__restrict__ ls, u64 n_lines, const u64 *__restrict__ code, const int *__restrict__ start,
                                             const int *__restrict__ end, const unsigned int *__restrict__ name_len, const u64 *__restrict__ block_off,
                                             u64 n_data, unsigned int n_runs, int *__restrict__ o_start, int *__restrict__ o_end,
                                             u64 *__restrict__ run_first, u64 *__restrict__ run_name, unsigned int *__restrict__ run_nlen,
                                             int *__restrict__ run_max, int *__restrict__ line_run) {
    const u64 i = (u64)blockIdx.x * TILE_T + threadIdx.x;
    const u64 c = i < n_lines ? code[i] : 0ull;
    u64 total;
    const u64 ex = block_off[blockIdx.x] + block_excl_scan(c, &total);
    const u64 d = ex >> 32;
    const unsigned int r = (unsigned int)(ex & 0xffffffffull) + (unsigned int)(c & 1ull) - 1u;      // a data line's run (the first data line starts run 0)
    const bool is_data = (c >> 32) != 0 && d < n_data && r < n_runs;
    int en = 0;
    if constexpr (SPLIT) { if (i < n_lines) line_run[i] = is_data ? (int)r : -1; }
    if (is_data) {
        en = end[i];
        if constexpr (!SPLIT) {
            o_start[d] = start[i];
            o_end[d] = en;
        }
        if (c & 1ull) { run_first[r] = d; run_name[r] = ls[i]; run_nlen[r] = name_len[i]; }
    }
    // largest end per run: one atomic per wave where the wave's data lines share a run (nearly every wave of a sorted file)
    const u64 m = __ballot(is_data);
    if (m == 0) return;
    const int lead = __ffsll((long long)m) - 1;
    const unsigned int r0 = __shfl(r, lead, 64);
    if (__ballot(is_data && r != r0) == 0) {
        int v = en;
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) v = max(v, __shfl_xor(v, k, 64));
        if ((int)(threadIdx.x & 63) == lead) atomicMax(&run_max[r0], v);
    } else if (is_data) atomicMax(&run_max[r], en);
}

__global__ void __launch_bounds__(TILE_T) frag_compact(const u64 *__restrict__ ls, u64 n_lines, const u64 *__restrict__ code, const int *__restrict__ start,
                                                       const int *__restrict__ end, const unsigned int *__restrict__ name_len, const u64 *__restrict__ block_off,
                                                       u64 n_data, unsigned int n_runs, int *__restrict__ o_start, int *__restrict__ o_end,
                                                       u64 *__restrict__ run_first, u64 *__restrict__ run_name, unsigned int *__restrict__ run_nlen,
                                                       int *__restrict__ run_max) {
    compact_body<false>(ls, n_lines, code, start, end, name_len, block_off, n_data, n_runs, o_start, o_end, run_first, run_name, run_nlen, run_max, nullptr);
}

// ---- the split by barcode ----
// the lanes of this wave that are `valid` and hold the same key (its low nbits); 0 for a lane that is not valid.  Every lane of the wave calls it.
__device__ __forceinline__ u64 wave_peers(unsigned int key, bool valid, int nbits) {
    u64 m = __ballot(valid);
    for (int b = 0; b < nbits; ++b) {
        const bool bit = (key >> b) & 1u;
        const u64 set = __ballot(bit);
        m &= bit ? set : ~set;
    }
    return valid ? m : 0ull;
}

// frag_parse by natac_fragio::split_line.  grp[i] = the group of line i, -1 for a line that is no data line or is unassigned.  bc_count
// lives across windows; bc_bits = the bits an index into the table takes.  Text is read inside the line's span (so inside [0, n)), the
// table inside its sizes (barcode_lookup).
__global__ void __launch_bounds__(TILE_T) frag_split_parse(const unsigned char *__restrict__ data, const u64 *__restrict__ ls, u64 n_lines, int open_tail,
                                                           natac_fragio::SplitTable tb, int bc_bits, u64 *__restrict__ code, int *__restrict__ start,
                                                           int *__restrict__ end, unsigned int *__restrict__ name_len, int *__restrict__ grp,
                                                           u64 *__restrict__ bc_count, u64 *__restrict__ block_sum, int *__restrict__ status) {
    const u64 i = (u64)blockIdx.x * TILE_T + threadIdx.x;
    u64 c = 0;
    int32_t bc = -1;
    if (i < n_lines) {
        u64 a, e;
        line_span(data, ls, i, n_lines, open_tail, &a, &e);
        uint32_t nlen = 0;
        int32_t s = 0, t = 0;
        const int kind = natac_fragio::split_line(data + a, (size_t)(e - a), tb, &nlen, &s, &t, &bc);
        if (kind > natac_fragio::LINE_DATA) atomicOr(&status[0], 1);
        if (kind == natac_fragio::LINE_DATA) {
            const bool differs = starts_run(data, ls, i, n_lines, open_tail, a, nlen);
            c = (1ull << 32) | (differs ? 1ull : 0ull);
            start[i] = s;
            end[i] = t;
            name_len[i] = nlen;
        } else bc = -1;
        if (bc >= (int32_t)tb.n_barcodes) bc = -1;
        code[i] = c;
        grp[i] = bc >= 0 ? tb.group[bc] : -1;
    }
    // one integer atomic per set of lanes that share a barcode (duplicate lines, one cell's neighbouring fragments)
    const u64 peers = wave_peers((unsigned int)bc, bc >= 0, bc_bits);
    if (bc >= 0 && (int)(threadIdx.x & 63) == __ffsll((long long)peers) - 1) atomicAdd(&bc_count[bc], (u64)__popcll(peers));
    u64 total;
    block_excl_scan(c, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TILE_T) frag_split_compact(const u64 *__restrict__ ls, u64 n_lines, const u64 *__restrict__ code, const int *__restrict__ end,
                                                             const unsigned int *__restrict__ name_len, const u64 *__restrict__ block_off, u64 n_data,
                                                             unsigned int n_runs, u64 *__restrict__ run_first, u64 *__restrict__ run_name,
                                                             unsigned int *__restrict__ run_nlen, int *__restrict__ run_max, int *__restrict__ line_run) {
    compact_body<true>(ls, n_lines, code, nullptr, end, name_len, block_off, n_data, n_runs, nullptr, nullptr, run_first, run_name, run_nlen, run_max, line_run);
}

// is line i an assigned data line: its group in g, its run in r
__device__ __forceinline__ bool split_line_of(const int *__restrict__ grp, const int *__restrict__ line_run, u64 i, u64 hi, int G, unsigned int n_runs, int *g,
                                              int *r) {
    *g = -1;
    *r = -1;
    if (i >= hi) return false;
    *g = grp[i];
    *r = line_run[i];
    return *g >= 0 && *g < G && *r >= 0 && (unsigned int)*r < n_runs;
}

// One wave per tile of PART_LINES lines.  tile_hist[g * n_tiles + tile] = the tile's lines of group g (group-major: its scan is the output
// order); seg_cnt[g * n_runs + r] += the tile's lines of group g in run r -- from the histogram where the tile lies in one run (nearly
// every tile of a sorted file), else one atomic per set of lanes that share (group, run).
__global__ void __launch_bounds__(PART_T) frag_split_hist(const int *__restrict__ grp, const int *__restrict__ line_run, u64 n_lines, int G, unsigned int n_runs,
                                                          u64 n_tiles, u64 *__restrict__ tile_hist, unsigned int *__restrict__ seg_cnt) {
    __shared__ unsigned int hist[256];
    const int lane = threadIdx.x;
    for (int k = lane; k < 256; k += PART_T) hist[k] = 0u;
    __syncthreads();
    const u64 lo = (u64)blockIdx.x * PART_LINES, hi = min(n_lines, lo + (u64)PART_LINES);
    int rmin = 0x7fffffff, rmax = -1;
    for (u64 base = lo; base < hi; base += PART_T) {
        int g, r;
        if (split_line_of(grp, line_run, base + lane, hi, G, n_runs, &g, &r)) {
            atomicAdd(&hist[g], 1u);
            rmin = min(rmin, r);
            rmax = max(rmax, r);
        }
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        rmin = min(rmin, __shfl_xor(rmin, k, 64));
        rmax = max(rmax, __shfl_xor(rmax, k, 64));
    }
    __syncthreads();
    for (int k = lane; k < G; k += PART_T) tile_hist[(u64)k * n_tiles + blockIdx.x] = (u64)hist[k];
    if (rmax < 0) return;                                // no assigned line in this tile
    if (rmin == rmax) {
        for (int k = lane; k < G; k += PART_T)
            if (hist[k]) atomicAdd(&seg_cnt[(u64)k * n_runs + (unsigned int)rmin], hist[k]);
        return;
    }
    for (u64 base = lo; base < hi; base += PART_T) {     // the tile spans runs: (group, run) is a key of 8 + 16 bits (MAX_RUNS)
        int g, r;
        const bool valid = split_line_of(grp, line_run, base + lane, hi, G, n_runs, &g, &r);
        const u64 peers = wave_peers(((unsigned int)r << 8) | ((unsigned int)g & 0xffu), valid, 24);
        if (valid && lane == __ffsll((long long)peers) - 1) atomicAdd(&seg_cnt[(u64)g * n_runs + (unsigned int)r], (unsigned int)__popcll(peers));
    }
}

// tile_off = the scanned tile_hist.  The wave walks its tile in file order, 64 lines a round: the lanes of one group take consecutive
// slots behind the group's running offset, in lane order, so every group keeps file order (a stable partition).
__global__ void __launch_bounds__(PART_T) frag_split_scatter(const int *__restrict__ grp, const int *__restrict__ line_run, const int *__restrict__ start,
                                                             const int *__restrict__ end, u64 n_lines, int G, unsigned int n_runs, u64 n_tiles,
                                                             const u64 *__restrict__ tile_off, u64 n_assigned, int *__restrict__ o_start,
                                                             int *__restrict__ o_end) {
    __shared__ u64 next[256];
    const int lane = threadIdx.x;
    for (int k = lane; k < 256; k += PART_T) next[k] = k < G ? tile_off[(u64)k * n_tiles + blockIdx.x] : 0ull;
    __syncthreads();
    const u64 lo = (u64)blockIdx.x * PART_LINES, hi = min(n_lines, lo + (u64)PART_LINES);
    for (u64 base = lo; base < hi; base += PART_T) {     // (the trip count is the same for every lane)
        int g, r;
        const bool valid = split_line_of(grp, line_run, base + lane, hi, G, n_runs, &g, &r);
        const u64 peers = wave_peers((unsigned int)g, valid, 8);
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        const u64 off = valid ? next[g] : 0ull;
        __syncthreads();
        if (valid && rank == 0) next[g] = off + (u64)__popcll(peers);
        __syncthreads();
        const u64 d = off + (u64)rank;
        if (valid && d < n_assigned) {
            o_start[d] = start[base + lane];
            o_end[d] = end[base + lane];
        }
    }
}

// names[r * 256 ...] = the name of run r (at most 255 bytes: parse_line's rule), read inside [0, n)
__global__ void __launch_bounds__(64) frag_gather_names(const unsigned char *__restrict__ data, u64 n, const u64 *__restrict__ run_name,
                                                        const unsigned int *__restrict__ run_nlen, unsigned int n_runs, unsigned char *__restrict__ names) {
    const unsigned int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= n_runs) return;
    const u64 a = run_name[r];
    const unsigned int len = min(run_nlen[r], 255u);
    for (unsigned int k = 0; k < len && a + k < n; ++k) names[(u64)r * 256 + k] = data[a + k];
}

// ---- discovering the cells (natac_frag_cells_device) ----
// The table is built from the file, on the device, and lives across windows: slot[n_slots] (64-bit words), the arena of the known cells'
// barcodes with off[n_cells + 1] into it, and cnt[n_cells][3] (n_frag, n_nfr, n_mono).  A slot word is
//   CELLS_EMPTY;  or k < 2^32: the slot belongs to cell k (its bytes are in the arena);  or CELLS_CLAIM | round << 32 | line: claimed in
//   THIS window by that line of the window, whose barcode lies in the window's text.
// atomicMin orders them: a cell's word is below every claim (it is never displaced), a claim of an earlier round is below every claim of
// a later one (a slot that was won stays won), and inside a round the smallest line wins, whatever the dispatch order.
// Per window, behind (a):
//   cells_parse: one lane per line runs natac_fragio::barcode_line and takes the barcode's span, length, size class and home slot.
//   rounds of cells_claim / cells_verify, two launches each, until the device counter of unresolved lines reads zero.  In round r every
//     unresolved line stands at the r-th slot of its probe sequence.  cells_claim: it claims the slot unless a cell or a smaller claim
//     holds it.  cells_verify (behind the kernel boundary every claim of the round is in): it compares its barcode, byte for byte, with
//     the slot's owner's -- in the arena, or in the text of the winning line -- and is resolved to the slot when they are equal (the
//     winner itself is), else it moves one slot on.  Nothing waits inside a kernel; the rounds are bounded by CELLS_MAX_ROUNDS and by the
//     slot count (then the host path answers: the table is full).
//   cells_number / frag_scan / cells_adopt: the winners are the first lines of the barcodes new in this window; a scan over that flag in
//     line order gives cell = cells known before + rank (first appearance in FILE order, no sort) and the barcode's place in the arena;
//     the winner copies its bytes there and turns its slot's word into the cell.
//   cells_count: every resolved line reads its cell from its slot; the three counters grow by one integer atomic per set of lanes of a
//     wave that share a cell.
// FIXED SIZE: the table does not grow.  It has 2^23 slots (NATAC_CELLS_DEV_SLOTS = another power of two: tests) and holds at most half as
// many cells -- 4,194,304, SPLIT_DEV_MAX_BARCODES -- so an empty slot always exists and probe sequences stay short; beyond that the host
// path answers.  Every read of the text lies inside a line's span (so inside [0, n)), every read of the arena inside its fill.
constexpr u64 CELLS_EMPTY = ~0ull, CELLS_CLAIM = 1ull << 60;
constexpr unsigned int CELLS_NONE = 0xffffffffu, CELLS_FAILED = 0xfffffffeu, CELLS_RESOLVED = 0x80000000u;      // probe[i] below n_slots: unresolved, at that slot
constexpr unsigned int CELLS_MAX_ROUNDS = 4096;         // (the longest probe sequence of 4 M keys in 8 M slots is a few dozen slots)
constexpr u64 CELLS_MAX_LINES = 1ull << 28;             // per window: a line fits the 32 bits of a claim, new cells and their bytes one packed scan
constexpr int CELLS_F_MALFORMED = 1, CELLS_F_FULL = 2, CELLS_F_BROKEN = 4;
enum { CELLS_S_DATA = 0, CELLS_S_UNASSIGNED = 1, CELLS_S_UNRESOLVED = 2, CELLS_S_NEW = 3, CELLS_S_FLAGS = 4, CELLS_S_WORDS = 8 };      // words of the state block

// meta[i] = the barcode's length (1-255; 0: no data line of a cell) | size class << 9; probe[i] = its home slot, or CELLS_NONE
__global__ void __launch_bounds__(TILE_T) cells_parse(const unsigned char *__restrict__ data, const u64 *__restrict__ ls, u64 n_lines, int open_tail,
                                                      int nfr_upper, int mono_upper, unsigned int home_mask, u64 *__restrict__ bc_at,
                                                      unsigned int *__restrict__ meta, unsigned int *__restrict__ probe, u64 *__restrict__ state) {
    const u64 i = (u64)blockIdx.x * TILE_T + threadIdx.x;
    u64 c = 0;                                           // (is data) << 32 | (is unassigned)
    if (i < n_lines) {
        u64 a, e;
        line_span(data, ls, i, n_lines, open_tail, &a, &e);
        int32_t s = 0, t = 0;
        size_t at = 0, len = 0;
        uint32_t nlen = 0;
        const int kind = natac_fragio::barcode_line(data + a, (size_t)(e - a), &nlen, &s, &t, &at, &len);
        if (kind > natac_fragio::LINE_DATA) atomicOr(&state[CELLS_S_FLAGS], (u64)CELLS_F_MALFORMED);
        unsigned int m = 0, pr = CELLS_NONE;
        if (kind == natac_fragio::LINE_DATA) {
            const bool cell = len >= 1 && len <= 255;
            c = (1ull << 32) | (cell ? 0ull : 1ull);
            if (cell) {
                m = (unsigned int)len | ((unsigned int)natac_fragio::cells_size_class(s, t, nfr_upper, mono_upper) << 9);
                pr = natac_fragio::barcode_hash(data + a + at, len) & home_mask;
            }
        }
        bc_at[i] = a + (u64)at;
        meta[i] = m;
        probe[i] = pr;
    }
    u64 total;
    block_excl_scan(c, &total);
    if (threadIdx.x == 0 && total) {
        atomicAdd(&state[CELLS_S_DATA], total >> 32);
        if (total & 0xffffffffull) atomicAdd(&state[CELLS_S_UNASSIGNED], total & 0xffffffffull);
    }
}

// One atomicMin per set of lanes of a wave that stand at the same slot (its lowest lane holds the smallest line), and none where the word
// already is a cell or a smaller claim: the word only ever decreases, so a stale look costs an atomic and never a claim.
__global__ void __launch_bounds__(TILE_T) cells_claim(const unsigned int *__restrict__ probe, u64 n_lines, u64 *slot, unsigned int n_slots, int slot_bits,
                                                      unsigned int round) {
    const u64 i = (u64)blockIdx.x * TILE_T + threadIdx.x;
    const unsigned int s = i < n_lines ? probe[i] : CELLS_NONE;
    const u64 mine = CELLS_CLAIM | ((u64)round << 32) | i;
    bool want = false;
    if (s < n_slots) want = __hip_atomic_load(&slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine;
    if (__ballot(want) == 0) return;                     // (the same for every lane of the wave)
    const u64 peers = wave_peers(s, want, slot_bits);
    if (want && (int)(threadIdx.x & 63) == __ffsll((long long)peers) - 1) atomicMin(&slot[s], mine);
}

// is the barcode of line i (len bytes at `at` of the text) the slot's owner's: 1 yes, 0 no, -1 the word or the tables are out of range
__device__ __forceinline__ int cells_same(const unsigned char *__restrict__ data, u64 n, const u64 *__restrict__ bc_at, const unsigned int *__restrict__ meta,
                                          u64 n_lines, u64 i, u64 at, unsigned int len, u64 v, const unsigned char *__restrict__ arena,
                                          const u64 *__restrict__ off, u64 n_known, u64 fill) {
    const unsigned char *q;
    u64 qlen;
    if (v < (1ull << 32)) {                              // a cell known before this window
        if (v >= n_known) return -1;
        const u64 a = off[v], b = off[v + 1];
        if (a > b || b > fill) return -1;
        q = arena + a;
        qlen = b - a;
    } else {                                             // a line of this window
        const u64 j = v & 0xffffffffull;
        if (v == CELLS_EMPTY || !(v & CELLS_CLAIM) || j >= n_lines) return -1;
        if (j == i) return 1;
        qlen = meta[j] & 0x1ffu;
        if (qlen == 0 || bc_at[j] + qlen > n) return -1;
        q = data + bc_at[j];
    }
    if (qlen != len) return 0;
    for (unsigned int k = 0; k < len; ++k)
        if (q[k] != data[at + k]) return 0;
    return 1;
}

__global__ void __launch_bounds__(TILE_T) cells_verify(const unsigned char *__restrict__ data, u64 n, const u64 *__restrict__ bc_at,
                                                       const unsigned int *__restrict__ meta, unsigned int *__restrict__ probe, u64 n_lines,
                                                       const u64 *__restrict__ slot, unsigned int n_slots, const unsigned char *__restrict__ arena,
                                                       const u64 *__restrict__ off, u64 n_known, u64 fill, unsigned int round, u64 *__restrict__ state) {
    const u64 i = (u64)blockIdx.x * TILE_T + threadIdx.x;
    bool again = false;
    if (i < n_lines) {
        const unsigned int s = probe[i];
        if (s < n_slots) {
            const int same = cells_same(data, n, bc_at, meta, n_lines, i, bc_at[i], meta[i] & 0x1ffu, slot[s], arena, off, n_known, fill);
            if (same == 1) probe[i] = CELLS_RESOLVED | s;
            else if (same == 0 && round + 1u < n_slots && round + 1u < CELLS_MAX_ROUNDS) {
                probe[i] = (s + 1u) & (n_slots - 1u);
                again = true;
            } else {
                probe[i] = CELLS_FAILED;
                atomicOr(&state[CELLS_S_FLAGS], (u64)(same == 0 ? CELLS_F_FULL : CELLS_F_BROKEN));
            }
        }
    }
    const u64 m = __ballot(again);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(&state[CELLS_S_UNRESOLVED], (u64)__popcll(m));
}

// (is the first line of a barcode new in this window) << 36 | its barcode's length: 2^28 lines of 255 bytes fit the low 36 bits
__device__ __forceinline__ u64 cells_new_code(const unsigned int *__restrict__ probe, const unsigned int *__restrict__ meta, const u64 *slot,
                                              unsigned int n_slots, u64 n_lines, u64 i, unsigned int *s) {
    if (i >= n_lines) return 0;
    const unsigned int p = probe[i];
    *s = p & ~CELLS_RESOLVED;
    if (!(p & CELLS_RESOLVED) || *s >= n_slots) return 0;
    const u64 v = __hip_atomic_load(&slot[*s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == CELLS_EMPTY || !(v & CELLS_CLAIM) || (v & 0xffffffffull) != i) return 0;
    return (1ull << 36) | (u64)(meta[i] & 0x1ffu);
}

__global__ void __launch_bounds__(TILE_T) cells_number(const unsigned int *__restrict__ probe, const unsigned int *__restrict__ meta, const u64 *slot,
                                                       unsigned int n_slots, u64 n_lines, u64 *__restrict__ block_sum) {
    unsigned int s;
    u64 total;
    block_excl_scan(cells_new_code(probe, meta, slot, n_slots, n_lines, (u64)blockIdx.x * TILE_T + threadIdx.x, &s), &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// block_off = the scanned block_sum.  The winner of a slot is cell n_known + its rank: its bytes go to the arena behind `fill`, and its
// slot's word becomes the cell.  Only the winner writes its slot; another line of the barcode that looks at the word sees the claim or the
// cell, and neither names it.
__global__ void __launch_bounds__(TILE_T) cells_adopt(const unsigned char *__restrict__ data, const u64 *__restrict__ bc_at, const unsigned int *__restrict__ probe,
                                                      const unsigned int *__restrict__ meta, u64 *slot, unsigned int n_slots, u64 n_lines,
                                                      const u64 *__restrict__ block_off, u64 n_known, u64 n_new, u64 fill, u64 new_bytes,
                                                      unsigned char *__restrict__ arena, u64 *__restrict__ off) {
    const u64 i = (u64)blockIdx.x * TILE_T + threadIdx.x;
    unsigned int s = 0;
    const u64 c = cells_new_code(probe, meta, slot, n_slots, n_lines, i, &s);
    u64 total;
    const u64 ex = block_off[blockIdx.x] + block_excl_scan(c, &total);
    const u64 rank = ex >> 36, at = ex & ((1ull << 36) - 1ull), len = c & 0x1ffull;
    if (c == 0 || rank >= n_new || at + len > new_bytes) return;
    for (u64 k = 0; k < len; ++k) arena[fill + at + k] = data[bc_at[i] + k];
    off[n_known + rank + 1] = fill + at + len;
    __hip_atomic_store(&slot[s], n_known + rank, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TILE_T) cells_count(const unsigned int *__restrict__ probe, const unsigned int *__restrict__ meta, const u64 *__restrict__ slot,
                                                      unsigned int n_slots, u64 n_lines, u64 n_cells, int cell_bits, u64 *__restrict__ cnt,
                                                      u64 *__restrict__ state) {
    const u64 i = (u64)blockIdx.x * TILE_T + threadIdx.x;
    u64 cell = 0;
    int cls = 2;
    bool valid = false;
    if (i < n_lines && (probe[i] & CELLS_RESOLVED) && probe[i] < CELLS_FAILED) {
        const unsigned int s = probe[i] & ~CELLS_RESOLVED;
        if (s < n_slots) {
            cell = slot[s];
            cls = (int)(meta[i] >> 9);
            valid = cell < n_cells;
        }
        if (!valid) atomicOr(&state[CELLS_S_FLAGS], (u64)CELLS_F_BROKEN);
    }
    const u64 peers = wave_peers((unsigned int)cell, valid, cell_bits), nfr = __ballot(valid && cls == 0), mono = __ballot(valid && cls == 1);
    if (valid && (int)(threadIdx.x & 63) == __ffsll((long long)peers) - 1) {
        atomicAdd(&cnt[3 * cell], (u64)__popcll(peers));
        if (peers & nfr) atomicAdd(&cnt[3 * cell + 1], (u64)__popcll(peers & nfr));
        if (peers & mono) atomicAdd(&cnt[3 * cell + 2], (u64)__popcll(peers & mono));
    }
}

// What a discovery adds to decode_device: the table on the device and the per-window work behind the line index.
struct CellsJob {
    int nfr_upper = 147, mono_upper = 294;
    natac_fragio::Cells *out = nullptr;
    unsigned int n_slots = 1u << 23, hash_mask = 0xffffffffu;
    int slot_bits = 23;
    u64 n_cells = 0, fill = 0;
    DevBuf slot, arena, off, cnt, state, bc_at, meta, probe, bsum;

    void configure() {
        if (const char *e = getenv("NATAC_CELLS_DEV_SLOTS")) {
            const long long v = atoll(e);
            if (v >= 16 && v <= (1ll << 26) && (v & (v - 1)) == 0) n_slots = (unsigned int)v;
        }
        slot_bits = 0;
        while ((1u << slot_bits) < n_slots) ++slot_bits;
        if (const char *e = getenv("NATAC_SPLIT_HASH_BITS")) { const int b = atoi(e); if (b >= 0 && b < 32) hash_mask = (1u << b) - 1u; }
    }

#define CELLS_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipGetLastError(); return std::string(#expr) + ": " + hipGetErrorString(e_); } } while (0)
    // "" or what stops the device path
    std::string start(hipStream_t stream) {
        configure();
        CELLS_HIP(slot.reserve((size_t)n_slots * sizeof(u64)));
        CELLS_HIP(state.reserve(CELLS_S_WORDS * sizeof(u64)));
        CELLS_HIP(off.reserve(4096 * sizeof(u64)));
        CELLS_HIP(arena.reserve(65536));
        CELLS_HIP(cnt.reserve(3 * 4096 * sizeof(u64)));
        CELLS_HIP(hipMemsetAsync(slot.p, 0xff, (size_t)n_slots * sizeof(u64), stream));          // CELLS_EMPTY
        CELLS_HIP(hipMemsetAsync(state.p, 0, CELLS_S_WORDS * sizeof(u64), stream));
        CELLS_HIP(hipMemsetAsync(off.p, 0, sizeof(u64), stream));                                 // off[0]
        return std::string();
    }

    // the lines of one window (ls[n_lines + 1] into data[0, n))
    std::string window(const unsigned char *data, u64 n, const u64 *ls, u64 n_lines, int open_tail, hipStream_t stream) {
        if (n_lines >= CELLS_MAX_LINES) return "more than 268,435,455 lines in a window";
        const u64 blocks = (n_lines + TILE_T - 1) / TILE_T;
        CELLS_HIP(bc_at.reserve((size_t)n_lines * sizeof(u64)));
        CELLS_HIP(meta.reserve((size_t)n_lines * sizeof(unsigned int)));
        CELLS_HIP(probe.reserve((size_t)n_lines * sizeof(unsigned int)));
        CELLS_HIP(bsum.reserve((size_t)blocks * sizeof(u64)));
        u64 *st = (u64 *)state.p;
        CELLS_HIP(hipMemsetAsync(st + CELLS_S_UNRESOLVED, 0, 2 * sizeof(u64), stream));          // (the flags stay: any of them ends the device path)
        hipLaunchKernelGGL(cells_parse, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, data, ls, n_lines, open_tail, nfr_upper, mono_upper,
                           hash_mask & (n_slots - 1u), (u64 *)bc_at.p, (unsigned int *)meta.p, (unsigned int *)probe.p, st);
        u64 h[3] = {0, 0, 0};                            // unresolved, new, flags
        for (unsigned int round = 0;; ++round) {
            if (round) CELLS_HIP(hipMemsetAsync(st + CELLS_S_UNRESOLVED, 0, sizeof(u64), stream));
            hipLaunchKernelGGL(cells_claim, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const unsigned int *)probe.p, n_lines, (u64 *)slot.p, n_slots,
                               slot_bits, round);
            hipLaunchKernelGGL(cells_verify, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, data, n, (const u64 *)bc_at.p, (const unsigned int *)meta.p,
                               (unsigned int *)probe.p, n_lines, (const u64 *)slot.p, n_slots, (const unsigned char *)arena.p, (const u64 *)off.p, n_cells,
                               fill, round, st);
            CELLS_HIP(hipMemcpyAsync(h, st + CELLS_S_UNRESOLVED, sizeof h, hipMemcpyDeviceToHost, stream));
            CELLS_HIP(hipStreamSynchronize(stream));
            if (h[2] & CELLS_F_MALFORMED) return "a malformed line";
            if (h[2] & CELLS_F_BROKEN) return "the cell table is out of range";
            if (h[2] & CELLS_F_FULL) return "the cell table is full";
            if (h[0] == 0) break;
            if (h[0] > n_lines || round + 1u >= CELLS_MAX_ROUNDS) return "the cell table is full";
        }
        hipLaunchKernelGGL(cells_number, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const unsigned int *)probe.p, (const unsigned int *)meta.p,
                           (const u64 *)slot.p, n_slots, n_lines, (u64 *)bsum.p);
        hipLaunchKernelGGL(frag_scan, dim3(1), dim3(1024), 0, stream, (u64 *)bsum.p, blocks, st + CELLS_S_NEW);
        CELLS_HIP(hipMemcpyAsync(h, st + CELLS_S_NEW, sizeof(u64), hipMemcpyDeviceToHost, stream));
        CELLS_HIP(hipStreamSynchronize(stream));
        const u64 n_new = h[0] >> 36, new_bytes = h[0] & ((1ull << 36) - 1ull);
        if (n_new > n_lines || new_bytes > 255 * n_new) return "counts out of range";
        if (n_cells + n_new > n_slots / 2) return "the cell table is full";
        if (n_new) {
            CELLS_HIP(arena.reserve((size_t)(fill + new_bytes), (size_t)fill, stream));
            CELLS_HIP(off.reserve((size_t)(n_cells + n_new + 1) * sizeof(u64), (size_t)(n_cells + 1) * sizeof(u64), stream));
            CELLS_HIP(cnt.reserve((size_t)(n_cells + n_new) * 3 * sizeof(u64), (size_t)n_cells * 3 * sizeof(u64), stream));
            CELLS_HIP(hipMemsetAsync((u64 *)cnt.p + 3 * n_cells, 0, (size_t)n_new * 3 * sizeof(u64), stream));
            hipLaunchKernelGGL(cells_adopt, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, data, (const u64 *)bc_at.p, (const unsigned int *)probe.p,
                               (const unsigned int *)meta.p, (u64 *)slot.p, n_slots, n_lines, (const u64 *)bsum.p, n_cells, n_new, fill, new_bytes,
                               (unsigned char *)arena.p, (u64 *)off.p);
            n_cells += n_new;
            fill += new_bytes;
        }
        int cell_bits = 1;
        while (cell_bits < 32 && (1ull << cell_bits) < n_cells) ++cell_bits;
        hipLaunchKernelGGL(cells_count, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const unsigned int *)probe.p, (const unsigned int *)meta.p,
                           (const u64 *)slot.p, n_slots, n_lines, n_cells, cell_bits, (u64 *)cnt.p, st);
        CELLS_HIP(hipGetLastError());
        return std::string();
    }

    // the table comes to the host once, behind the last window
    std::string finish(hipStream_t stream) {
        u64 h[CELLS_S_WORDS];
        std::vector<u64> h_off((size_t)n_cells + 1), h_cnt((size_t)n_cells * 3);
        out->bytes.resize((size_t)fill);
        CELLS_HIP(hipMemcpyAsync(h, state.p, sizeof h, hipMemcpyDeviceToHost, stream));
        CELLS_HIP(hipMemcpyAsync(h_off.data(), off.p, h_off.size() * sizeof(u64), hipMemcpyDeviceToHost, stream));
        if (n_cells) CELLS_HIP(hipMemcpyAsync(h_cnt.data(), cnt.p, h_cnt.size() * sizeof(u64), hipMemcpyDeviceToHost, stream));
        if (fill) CELLS_HIP(hipMemcpyAsync(out->bytes.data(), arena.p, (size_t)fill, hipMemcpyDeviceToHost, stream));
        CELLS_HIP(hipStreamSynchronize(stream));
        if (h[CELLS_S_FLAGS] != 0) return "the cell table is out of range";
        out->off.assign(h_off.begin(), h_off.end());
        out->n_frag.resize((size_t)n_cells); out->n_nfr.resize((size_t)n_cells); out->n_mono.resize((size_t)n_cells);
        u64 assigned = 0;
        for (size_t k = 0; k < (size_t)n_cells; ++k) {
            if (h_off[k + 1] <= h_off[k] || h_off[k + 1] - h_off[k] > 255 || h_off[k + 1] > fill) return "the cell table is out of range";
            out->n_frag[k] = (int64_t)h_cnt[3 * k];
            out->n_nfr[k] = (int64_t)h_cnt[3 * k + 1];
            out->n_mono[k] = (int64_t)h_cnt[3 * k + 2];
            assigned += h_cnt[3 * k];
        }
        if (h_off[(size_t)n_cells] != fill || assigned + h[CELLS_S_UNASSIGNED] != h[CELLS_S_DATA]) return "the cell table is out of range";
        out->n_data = (int64_t)h[CELLS_S_DATA];
        out->n_unassigned = (int64_t)h[CELLS_S_UNASSIGNED];
        return std::string();
    }
#undef CELLS_HIP
};

// what a split adds to decode_device: the table, the builder both paths share and the per-barcode counts (table->group.size() of them)
struct SplitJob {
    const natac_fragio::SplitTableHost *table;
    natac_fragio::SplitBuilder *sb;
    std::vector<int64_t> bc_count;
};

// Returns the same object as natac_fragio::decode, or nullptr: the host decoder answers (`why` says what stopped the device path).
// With `split` the returned object is empty (a token of success): the groups are in split->sb, the counts in split->bc_count.
// With `cells` likewise: the table is in cells->out.
inline natac_bamio::Bam *decode_device(const char *path, hipStream_t stream, std::string &why, size_t window_bytes = (size_t)1 << 30,
                                       SplitJob *split = nullptr, CellsJob *cells = nullptr) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) { why = std::string("cannot open ") + path; return nullptr; }
    struct stat sb;
    if (fstat(fd, &sb) != 0) { close(fd); why = "cannot size the file"; return nullptr; }
    const u64 fsize = (u64)sb.st_size;
    window_bytes = std::max<size_t>(window_bytes, (size_t)4096);
    const size_t STAGE = (size_t)std::min<u64>((u64)32 << 20, std::max<u64>(fsize, 4096));      // two small pinned buffers: natac_bam_dev.hpp says why
    unsigned char *stage[2] = {nullptr, nullptr};
    hipEvent_t staged[2] = {nullptr, nullptr};
    natac_bamio::Bam *bam = new natac_bamio::Bam();
    natac_fragio::Builder bd(bam);
    DevBuf d_raw, d_mem, d_data[2], d_status, d_queue, d_crc, d_tile, d_ls, d_code, d_start, d_end, d_nlen, d_bsum, d_total, d_ostart, d_oend, d_rfirst,
        d_rname, d_rnlen, d_rmax, d_names, d_tb_bytes, d_tb_off, d_tb_group, d_tb_slot, d_bcc, d_grp, d_lrun, d_thist, d_seg;
    natac_fragio::SplitTable dev_tb{};
    int bc_bits = 1, G = 0;
    std::vector<unsigned int> h_seg;
    std::vector<int> run_chrom;
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};
    std::vector<Member> mem;
    std::vector<int> h_start, h_end, h_rmax;
    std::vector<u64> h_rfirst;
    std::vector<unsigned int> h_rnlen;
    std::vector<unsigned char> h_names;
    std::vector<int64_t> pos, tlen;
    int cur_buf = 0;
    Chain chain;
    std::thread walker(natac_bamdev::walk_chain, fd, fsize, &chain);
    auto cleanup = [&]() {
        if (walker.joinable()) walker.join();
        for (int i = 0; i < 3; ++i) if (aux[i]) { (void)hipStreamSynchronize(aux[i]); (void)hipStreamDestroy(aux[i]); }
        (void)hipStreamSynchronize(stream);
        for (int i = 0; i < 2; ++i) { if (stage[i]) (void)hipHostFree(stage[i]); if (staged[i]) (void)hipEventDestroy(staged[i]); }
        close(fd);
    };
    auto give_up = [&](const std::string &msg) -> natac_bamio::Bam * { why = msg; delete bam; cleanup(); return nullptr; };
#define FRAGDEV_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipGetLastError(); return give_up(std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
    for (int i = 0; i < 2; ++i) {
        FRAGDEV_HIP(hipHostMalloc((void **)&stage[i], STAGE, hipHostMallocDefault));
        FRAGDEV_HIP(hipEventCreateWithFlags(&staged[i], hipEventDisableTiming));
    }
    for (int i = 0; i < 3; ++i) FRAGDEV_HIP(hipStreamCreateWithFlags(&aux[i], hipStreamNonBlocking));
    FRAGDEV_HIP(d_status.reserve(4 * sizeof(int)));
    FRAGDEV_HIP(d_total.reserve(4 * sizeof(u64)));
    if (cells) { const std::string stop = cells->start(stream); if (!stop.empty()) return give_up(stop); }
    if (split) {                                         // the table goes up once
        const natac_fragio::SplitTableHost &t = *split->table;
        G = t.n_groups;
        while (bc_bits < 32 && ((size_t)1 << bc_bits) < t.group.size()) ++bc_bits;
        FRAGDEV_HIP(d_tb_bytes.reserve(t.bytes.size()));
        FRAGDEV_HIP(d_tb_off.reserve(t.off.size() * sizeof(uint32_t)));
        FRAGDEV_HIP(d_tb_group.reserve(t.group.size() * sizeof(int32_t)));
        FRAGDEV_HIP(d_tb_slot.reserve(t.slot.size() * sizeof(uint32_t)));
        FRAGDEV_HIP(d_bcc.reserve(t.group.size() * sizeof(u64)));
        FRAGDEV_HIP(hipMemcpyAsync(d_tb_bytes.p, t.bytes.data(), t.bytes.size(), hipMemcpyHostToDevice, stream));
        FRAGDEV_HIP(hipMemcpyAsync(d_tb_off.p, t.off.data(), t.off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        FRAGDEV_HIP(hipMemcpyAsync(d_tb_group.p, t.group.data(), t.group.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        FRAGDEV_HIP(hipMemcpyAsync(d_tb_slot.p, t.slot.data(), t.slot.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        FRAGDEV_HIP(hipMemsetAsync(d_bcc.p, 0, t.group.size() * sizeof(u64), stream));
        FRAGDEV_HIP(hipStreamSynchronize(stream));
        dev_tb = natac_fragio::SplitTable{(const unsigned char *)d_tb_bytes.p, (const uint32_t *)d_tb_off.p, (const int32_t *)d_tb_group.p,
                                          (const uint32_t *)d_tb_slot.p, (uint32_t)t.group.size(), (uint32_t)t.slot.size(), t.hash_mask};
    }
    {
        std::vector<unsigned int> t8(8 * 256);
        natac_bamdev::crc32_slice8_tables(t8.data());
        FRAGDEV_HIP(d_crc.reserve(t8.size() * sizeof(unsigned int)));
        FRAGDEV_HIP(hipMemcpyAsync(d_crc.p, t8.data(), t8.size() * sizeof(unsigned int), hipMemcpyHostToDevice, stream));
        FRAGDEV_HIP(hipStreamSynchronize(stream));      // t8 is a local
    }
    int n_cu = 256;
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
    }
    const bool timing = getenv("NATAC_FRAG_DEV_TIMING") != nullptr;
    double t_read = 0, t_scan = 0, t_inflate = 0, t_lines = 0, t_parse = 0, t_out = 0;
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t0 = now();
    auto lap = [&](double &acc) { const double t = now(); acc += t - t0; t0 = t; };
    u64 pend = 0;          // carried bytes at the front of d_data[cur_buf]
    u64 win_start = 0;     // file offset of the window = start of its first member
    size_t m0 = 0;         // its first member in the chain
    for (;;) {
        // ---- the members of this window: as many as fit window_bytes (at least one), once the chain walk has got that far
        size_t m1 = m0;
        u64 win_end = win_start;
        {
            std::unique_lock<std::mutex> lk(chain.mu);
            chain.cv.wait(lk, [&]() { return chain.done || (!chain.ends.empty() && chain.ends.back() >= win_start + window_bytes); });
            if (!chain.error.empty()) { const std::string e = chain.error; lk.unlock(); return give_up(e); }
            while (m1 < chain.ends.size() && (m1 == m0 || chain.ends[m1] <= win_start + window_bytes)) ++m1;
            mem.assign(chain.members.begin() + (long)m0, chain.members.begin() + (long)m1);
            if (m1 > m0) win_end = chain.ends[m1 - 1];
        }
        if (mem.empty()) break;                                         // the whole chain is done
        u64 n = pend;
        for (auto &mb : mem) { mb.coff -= win_start; mb.uoff = n; n += mb.isize; }
        const int M = (int)mem.size();
        const size_t o = (size_t)(win_end - win_start);
        lap(t_scan);
        // ---- upload (the read of one staging buffer next to the copy of the other) + inflate of the members that have arrived
        FRAGDEV_HIP(d_raw.reserve(o + 64));
        FRAGDEV_HIP(d_mem.reserve(mem.size() * sizeof(Member)));
        FRAGDEV_HIP(d_data[cur_buf].reserve((size_t)n + 64, (size_t)pend, stream));      // the carry at the front stays
        unsigned char *data = (unsigned char *)d_data[cur_buf].p;
        const size_t SUBWIN = (size_t)256 << 20;
        const int max_launches = (int)(o / SUBWIN) + 2;
        FRAGDEV_HIP(d_queue.reserve((size_t)max_launches * sizeof(int)));
        FRAGDEV_HIP(hipMemcpyAsync(d_mem.p, mem.data(), mem.size() * sizeof(Member), hipMemcpyHostToDevice, stream));
        FRAGDEV_HIP(hipMemsetAsync(d_status.p, 0, 4 * sizeof(int), stream));
        FRAGDEV_HIP(hipMemsetAsync(d_queue.p, 0, (size_t)max_launches * sizeof(int), stream));
        {
            int which = 0, launched = 0, n_launch = 0;
            size_t since = 0;
            for (size_t at = 0; at < o; which ^= 1) {
                const size_t len = std::min(STAGE, o - at);
                FRAGDEV_HIP(hipEventSynchronize(staged[which]));         // the copy that used this buffer last has finished
                {   // four concurrent preads fill the staging buffer, as for a BAM
                    const int RT = len >= ((size_t)4 << 20) ? 4 : 1;
                    bool bad[4] = {false, false, false, false};
                    auto fill = [&](int t) {
                        size_t a = len * (size_t)t / (size_t)RT;
                        const size_t b = len * ((size_t)t + 1) / (size_t)RT;
                        while (a < b) {
                            const ssize_t r = pread(fd, stage[which] + a, b - a, (off_t)(win_start + at + a));
                            if (r <= 0) { bad[t] = true; return; }
                            a += (size_t)r;
                        }
                    };
                    std::thread th[3];
                    for (int t = 1; t < RT; ++t) th[t - 1] = std::thread(fill, t);
                    fill(0);
                    for (int t = 1; t < RT; ++t) th[t - 1].join();
                    if (bad[0] || bad[1] || bad[2] || bad[3]) return give_up("read error");
                }
                FRAGDEV_HIP(hipMemcpyAsync((unsigned char *)d_raw.p + at, stage[which], len, hipMemcpyHostToDevice, stream));
                FRAGDEV_HIP(hipEventRecord(staged[which], stream));
                at += len;
                since += len;
                if (since >= SUBWIN || at == o) {
                    int upto = launched;                                // members that lie completely inside the uploaded bytes
                    while (upto < M && mem[(size_t)upto].coff + mem[(size_t)upto].csize + 8 <= at) ++upto;
                    if (at == o) upto = M;
                    if (upto > launched) {
                        hipStream_t side = aux[n_launch % 3];
                        FRAGDEV_HIP(hipStreamWaitEvent(side, staged[which], 0));
                        const int cnt = upto - launched;
                        hipLaunchKernelGGL(natac_bamdev::bamdev_inflate, dim3((unsigned)std::min<long long>((cnt + 63) / 64, 3ll * n_cu)), dim3(64), 0, side,
                                           (const unsigned char *)d_raw.p, (const Member *)d_mem.p, launched, upto, data, (int *)d_status.p,
                                           (int *)d_queue.p + n_launch, (const unsigned int *)d_crc.p);
                        launched = upto;
                        ++n_launch;
                        since = 0;
                    }
                }
            }
        }
        lap(t_read);
        for (int i = 0; i < 3; ++i) FRAGDEV_HIP(hipStreamSynchronize(aux[i]));
        int st[2] = {0, 0};
        FRAGDEV_HIP(hipMemcpyAsync(st, d_status.p, sizeof st, hipMemcpyDeviceToHost, stream));
        FRAGDEV_HIP(hipStreamSynchronize(stream));
        if (st[0] != 0) return give_up("a BGZF member does not inflate or fails its CRC-32");
        const bool eof = win_end == fsize;
        win_start = win_end;
        m0 = m1;
        lap(t_inflate);
        u64 cur = 0;                        // the carry into the next window starts here
        if (n > 0) {
            // ---- (a) line index
            const u64 tiles = (n + TILE_B - 1) / TILE_B;
            FRAGDEV_HIP(d_tile.reserve((size_t)tiles * sizeof(u64)));
            hipLaunchKernelGGL(frag_count_nl, dim3((unsigned)tiles), dim3(TILE_T), 0, stream, (const unsigned char *)data, n, (u64 *)d_tile.p);
            hipLaunchKernelGGL(frag_scan, dim3(1), dim3(1024), 0, stream, (u64 *)d_tile.p, tiles, (u64 *)d_total.p);
            u64 n_nl = 0;
            unsigned char last_byte = 0;
            FRAGDEV_HIP(hipMemcpyAsync(&n_nl, d_total.p, sizeof n_nl, hipMemcpyDeviceToHost, stream));
            FRAGDEV_HIP(hipMemcpyAsync(&last_byte, data + n - 1, 1, hipMemcpyDeviceToHost, stream));
            FRAGDEV_HIP(hipStreamSynchronize(stream));
            if (n_nl > n) return give_up("line count out of range");
            const int open_tail = eof && last_byte != '\n' ? 1 : 0;        // a last line without '\n' is a line
            const u64 n_lines = n_nl + (u64)open_tail;
            if (n_lines == 0) return give_up("a window without a line end (a line longer than a window)");
            {
                FRAGDEV_HIP(d_ls.reserve((size_t)(n_lines + 2) * sizeof(u64)));
                u64 *ls = (u64 *)d_ls.p;
                const u64 zero = 0, behind = n + 1;
                FRAGDEV_HIP(hipMemcpyAsync(ls, &zero, sizeof zero, hipMemcpyHostToDevice, stream));
                hipLaunchKernelGGL(frag_line_starts, dim3((unsigned)tiles), dim3(TILE_T), 0, stream, (const unsigned char *)data, n, (const u64 *)d_tile.p, n_nl, ls);
                if (open_tail) FRAGDEV_HIP(hipMemcpyAsync(ls + n_lines, &behind, sizeof behind, hipMemcpyHostToDevice, stream));
                FRAGDEV_HIP(hipMemcpyAsync(&cur, ls + n_nl, sizeof cur, hipMemcpyDeviceToHost, stream));
                lap(t_lines);
                if (cells) {                             // ---- discovery: the table grows by this window's lines (CellsJob)
                    FRAGDEV_HIP(hipStreamSynchronize(stream));
                    if (cur > n) return give_up("counts out of range");
                    const std::string stop = cells->window((const unsigned char *)data, n, (const u64 *)ls, n_lines, open_tail, stream);
                    if (!stop.empty()) return give_up(stop);
                    if (open_tail) cur = n;
                    lap(t_parse);
                } else {
                    // ---- (b) parse
                    const u64 blocks = (n_lines + TILE_T - 1) / TILE_T;
                    FRAGDEV_HIP(d_code.reserve((size_t)n_lines * sizeof(u64)));
                    FRAGDEV_HIP(d_start.reserve((size_t)n_lines * sizeof(int)));
                    FRAGDEV_HIP(d_end.reserve((size_t)n_lines * sizeof(int)));
                    FRAGDEV_HIP(d_nlen.reserve((size_t)n_lines * sizeof(unsigned int)));
                    FRAGDEV_HIP(d_bsum.reserve((size_t)blocks * sizeof(u64)));
                    if (split) {
                        FRAGDEV_HIP(d_grp.reserve((size_t)n_lines * sizeof(int)));
                        hipLaunchKernelGGL(frag_split_parse, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const unsigned char *)data, (const u64 *)ls, n_lines,
                                           open_tail, dev_tb, bc_bits, (u64 *)d_code.p, (int *)d_start.p, (int *)d_end.p, (unsigned int *)d_nlen.p, (int *)d_grp.p,
                                           (u64 *)d_bcc.p, (u64 *)d_bsum.p, (int *)d_status.p);
                    } else
                        hipLaunchKernelGGL(frag_parse, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const unsigned char *)data, (const u64 *)ls, n_lines,
                                           open_tail, (u64 *)d_code.p, (int *)d_start.p, (int *)d_end.p, (unsigned int *)d_nlen.p, (u64 *)d_bsum.p,
                                           (int *)d_status.p);
                    hipLaunchKernelGGL(frag_scan, dim3(1), dim3(1024), 0, stream, (u64 *)d_bsum.p, blocks, (u64 *)d_total.p + 1);
                    u64 packed = 0;
                    FRAGDEV_HIP(hipMemcpyAsync(&packed, (u64 *)d_total.p + 1, sizeof packed, hipMemcpyDeviceToHost, stream));
                    FRAGDEV_HIP(hipMemcpyAsync(st, d_status.p, sizeof st, hipMemcpyDeviceToHost, stream));
                    FRAGDEV_HIP(hipStreamSynchronize(stream));
                    if (st[0] != 0) return give_up("a malformed line");
                    const u64 n_data = packed >> 32, n_runs = packed & 0xffffffffull;
                    if (n_data > n_lines || n_runs > n_data || cur > n) return give_up("counts out of range");
                    if (n_runs > MAX_RUNS) return give_up("more than 65,536 chromosome runs in a window");
                    if (split && n_runs * (u64)G > SPLIT_MAX_SEGMENTS) return give_up("more than 1,048,576 groups x chromosome runs in a window");
                    if (open_tail) cur = n;
                    lap(t_parse);
                    // ---- (c) compaction, the run names, and the append on the host
                    if (n_data && split) {
                        FRAGDEV_HIP(d_rfirst.reserve((size_t)n_runs * sizeof(u64)));
                        FRAGDEV_HIP(d_rname.reserve((size_t)n_runs * sizeof(u64)));
                        FRAGDEV_HIP(d_rnlen.reserve((size_t)n_runs * sizeof(unsigned int)));
                        FRAGDEV_HIP(d_rmax.reserve((size_t)n_runs * sizeof(int)));
                        FRAGDEV_HIP(d_names.reserve((size_t)n_runs * 256));
                        FRAGDEV_HIP(d_lrun.reserve((size_t)n_lines * sizeof(int)));
                        const u64 n_tiles = (n_lines + PART_LINES - 1) / PART_LINES, n_seg = n_runs * (u64)G;
                        FRAGDEV_HIP(d_thist.reserve((size_t)(n_tiles * (u64)G) * sizeof(u64)));
                        FRAGDEV_HIP(d_seg.reserve((size_t)n_seg * sizeof(unsigned int)));
                        FRAGDEV_HIP(hipMemsetAsync(d_rmax.p, 0, (size_t)n_runs * sizeof(int), stream));
                        FRAGDEV_HIP(hipMemsetAsync(d_rfirst.p, 0, (size_t)n_runs * sizeof(u64), stream));
                        FRAGDEV_HIP(hipMemsetAsync(d_rnlen.p, 0, (size_t)n_runs * sizeof(unsigned int), stream));
                        FRAGDEV_HIP(hipMemsetAsync(d_rname.p, 0, (size_t)n_runs * sizeof(u64), stream));
                        FRAGDEV_HIP(hipMemsetAsync(d_seg.p, 0, (size_t)n_seg * sizeof(unsigned int), stream));
                        hipLaunchKernelGGL(frag_split_compact, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const u64 *)ls, n_lines, (const u64 *)d_code.p,
                                           (const int *)d_end.p, (const unsigned int *)d_nlen.p, (const u64 *)d_bsum.p, n_data, (unsigned int)n_runs,
                                           (u64 *)d_rfirst.p, (u64 *)d_rname.p, (unsigned int *)d_rnlen.p, (int *)d_rmax.p, (int *)d_lrun.p);
                        hipLaunchKernelGGL(frag_gather_names, dim3((unsigned)((n_runs + 63) / 64)), dim3(64), 0, stream, (const unsigned char *)data, n,
                                           (const u64 *)d_rname.p, (const unsigned int *)d_rnlen.p, (unsigned int)n_runs, (unsigned char *)d_names.p);
                        hipLaunchKernelGGL(frag_split_hist, dim3((unsigned)n_tiles), dim3(PART_T), 0, stream, (const int *)d_grp.p, (const int *)d_lrun.p, n_lines, G,
                                           (unsigned int)n_runs, n_tiles, (u64 *)d_thist.p, (unsigned int *)d_seg.p);
                        hipLaunchKernelGGL(frag_scan, dim3(1), dim3(1024), 0, stream, (u64 *)d_thist.p, n_tiles * (u64)G, (u64 *)d_total.p + 2);
                        u64 n_assigned = 0;
                        FRAGDEV_HIP(hipMemcpyAsync(&n_assigned, (u64 *)d_total.p + 2, sizeof n_assigned, hipMemcpyDeviceToHost, stream));
                        h_rfirst.resize(n_runs); h_rnlen.resize(n_runs); h_rmax.resize(n_runs); h_names.resize((size_t)n_runs * 256); h_seg.resize((size_t)n_seg);
                        FRAGDEV_HIP(hipMemcpyAsync(h_rfirst.data(), d_rfirst.p, (size_t)n_runs * sizeof(u64), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_rnlen.data(), d_rnlen.p, (size_t)n_runs * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_rmax.data(), d_rmax.p, (size_t)n_runs * sizeof(int), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_names.data(), d_names.p, (size_t)n_runs * 256, hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_seg.data(), d_seg.p, (size_t)n_seg * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipStreamSynchronize(stream));
                        if (n_assigned > n_data) return give_up("counts out of range");
                        if (n_assigned) {                    // unassigned lines stay on the device
                            FRAGDEV_HIP(d_ostart.reserve((size_t)n_assigned * sizeof(int)));
                            FRAGDEV_HIP(d_oend.reserve((size_t)n_assigned * sizeof(int)));
                            hipLaunchKernelGGL(frag_split_scatter, dim3((unsigned)n_tiles), dim3(PART_T), 0, stream, (const int *)d_grp.p, (const int *)d_lrun.p,
                                               (const int *)d_start.p, (const int *)d_end.p, n_lines, G, (unsigned int)n_runs, n_tiles, (const u64 *)d_thist.p,
                                               n_assigned, (int *)d_ostart.p, (int *)d_oend.p);
                            h_start.resize(n_assigned); h_end.resize(n_assigned);
                            FRAGDEV_HIP(hipMemcpyAsync(h_start.data(), d_ostart.p, (size_t)n_assigned * sizeof(int), hipMemcpyDeviceToHost, stream));
                            FRAGDEV_HIP(hipMemcpyAsync(h_end.data(), d_oend.p, (size_t)n_assigned * sizeof(int), hipMemcpyDeviceToHost, stream));
                            FRAGDEV_HIP(hipStreamSynchronize(stream));
                        }
                        run_chrom.resize(n_runs);
                        for (size_t r = 0; r < (size_t)n_runs; ++r) {
                            const u64 a = h_rfirst[r], b = r + 1 < (size_t)n_runs ? h_rfirst[r + 1] : n_data;
                            if (a >= b || b > n_data || h_rnlen[r] == 0 || h_rnlen[r] > 255) return give_up("run table out of range");
                            run_chrom[r] = split->sb->chrom(std::string((const char *)h_names.data() + r * 256, h_rnlen[r]), h_rmax[r], (int64_t)(b - a));
                        }
                        u64 at = 0;                          // the segments, group-major as the partition wrote them
                        for (int g = 0; g < G; ++g)
                            for (size_t r = 0; r < (size_t)n_runs; ++r) {
                                const u64 cnt = h_seg[(size_t)g * (size_t)n_runs + r];
                                if (cnt > n_assigned - at) return give_up("segment table out of range");
                                for (u64 k = at; k < at + cnt; ++k) split->sb->append(g, run_chrom[r], h_start[(size_t)k], h_end[(size_t)k]);
                                at += cnt;
                            }
                        if (at != n_assigned) return give_up("segment table out of range");
                    } else if (n_data) {
                        FRAGDEV_HIP(d_ostart.reserve((size_t)n_data * sizeof(int)));
                        FRAGDEV_HIP(d_oend.reserve((size_t)n_data * sizeof(int)));
                        FRAGDEV_HIP(d_rfirst.reserve((size_t)n_runs * sizeof(u64)));
                        FRAGDEV_HIP(d_rname.reserve((size_t)n_runs * sizeof(u64)));
                        FRAGDEV_HIP(d_rnlen.reserve((size_t)n_runs * sizeof(unsigned int)));
                        FRAGDEV_HIP(d_rmax.reserve((size_t)n_runs * sizeof(int)));
                        FRAGDEV_HIP(d_names.reserve((size_t)n_runs * 256));
                        FRAGDEV_HIP(hipMemsetAsync(d_rmax.p, 0, (size_t)n_runs * sizeof(int), stream));
                        FRAGDEV_HIP(hipMemsetAsync(d_rfirst.p, 0, (size_t)n_runs * sizeof(u64), stream));
                        FRAGDEV_HIP(hipMemsetAsync(d_rnlen.p, 0, (size_t)n_runs * sizeof(unsigned int), stream));
                        FRAGDEV_HIP(hipMemsetAsync(d_rname.p, 0, (size_t)n_runs * sizeof(u64), stream));
                        hipLaunchKernelGGL(frag_compact, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const u64 *)ls, n_lines, (const u64 *)d_code.p,
                                           (const int *)d_start.p, (const int *)d_end.p, (const unsigned int *)d_nlen.p, (const u64 *)d_bsum.p, n_data,
                                           (unsigned int)n_runs, (int *)d_ostart.p, (int *)d_oend.p, (u64 *)d_rfirst.p, (u64 *)d_rname.p,
                                           (unsigned int *)d_rnlen.p, (int *)d_rmax.p);
                        hipLaunchKernelGGL(frag_gather_names, dim3((unsigned)((n_runs + 63) / 64)), dim3(64), 0, stream, (const unsigned char *)data, n,
                                           (const u64 *)d_rname.p, (const unsigned int *)d_rnlen.p, (unsigned int)n_runs, (unsigned char *)d_names.p);
                        h_start.resize(n_data); h_end.resize(n_data);
                        h_rfirst.resize(n_runs); h_rnlen.resize(n_runs); h_rmax.resize(n_runs); h_names.resize((size_t)n_runs * 256);
                        FRAGDEV_HIP(hipMemcpyAsync(h_start.data(), d_ostart.p, (size_t)n_data * sizeof(int), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_end.data(), d_oend.p, (size_t)n_data * sizeof(int), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_rfirst.data(), d_rfirst.p, (size_t)n_runs * sizeof(u64), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_rnlen.data(), d_rnlen.p, (size_t)n_runs * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_rmax.data(), d_rmax.p, (size_t)n_runs * sizeof(int), hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipMemcpyAsync(h_names.data(), d_names.p, (size_t)n_runs * 256, hipMemcpyDeviceToHost, stream));
                        FRAGDEV_HIP(hipStreamSynchronize(stream));
                        for (size_t r = 0; r < (size_t)n_runs; ++r) {
                            const u64 a = h_rfirst[r], b = r + 1 < (size_t)n_runs ? h_rfirst[r + 1] : n_data;
                            if (a >= b || b > n_data || h_rnlen[r] == 0 || h_rnlen[r] > 255) return give_up("run table out of range");
                            pos.resize((size_t)(b - a));
                            tlen.resize((size_t)(b - a));
                            for (u64 i = a; i < b; ++i) {
                                pos[(size_t)(i - a)] = (int64_t)h_start[(size_t)i] - 4;
                                tlen[(size_t)(i - a)] = (int64_t)h_end[(size_t)i] - (int64_t)h_start[(size_t)i] + 8;
                            }
                            natac_fragio::append_run(bd, std::string((const char *)h_names.data() + r * 256, h_rnlen[r]), pos.data(), tlen.data(), (size_t)(b - a),
                                                     h_rmax[r]);
                        }
                    }
                }
            }
        }
        // ---- carry the bytes behind the last '\n' to the front of the other buffer
        pend = n - cur;
        FRAGDEV_HIP(d_data[cur_buf ^ 1].reserve((size_t)pend + 64));
        if (pend) FRAGDEV_HIP(hipMemcpyAsync(d_data[cur_buf ^ 1].p, data + cur, (size_t)pend, hipMemcpyDeviceToDevice, stream));
        FRAGDEV_HIP(hipStreamSynchronize(stream));
        cur_buf ^= 1;
        lap(t_out);
        if (eof) break;
    }
    if (timing)
        std::fprintf(stderr, "[natac_frag_dev] read + upload %.3f s, waiting for the member chain %.3f, inflate %.3f, line index %.3f, parse %.3f, compaction + append + carry %.3f\n",
                     t_read, t_scan, t_inflate, t_lines, t_parse, t_out);
#undef FRAGDEV_HIP
    if (pend != 0) return give_up("bytes left behind the last window");
    if (cells) { const std::string stop = cells->finish(stream); if (!stop.empty()) return give_up(stop); }
    if (split) {
        std::vector<u64> h_bcc(split->table->group.size());
        split->bc_count.resize(h_bcc.size());
        const hipError_t e_ = hipMemcpy(h_bcc.data(), d_bcc.p, h_bcc.size() * sizeof(u64), hipMemcpyDeviceToHost);
        if (e_ != hipSuccess) { (void)hipGetLastError(); return give_up(std::string("hipMemcpy of the barcode counts: ") + hipGetErrorString(e_)); }
        for (size_t k = 0; k < h_bcc.size(); ++k) split->bc_count[k] = (int64_t)h_bcc[k];
    }
    cleanup();
    return bam;
}

}  // namespace natac_fragdev
