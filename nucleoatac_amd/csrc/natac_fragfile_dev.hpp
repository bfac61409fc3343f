// natac_fragfile_dev.hpp -- BGZF fragment file -> fragment arrays on the GPU.
//
// The members are found, staged, inflated and CRC-checked exactly as for a BAM: both decoders read the file through
// natac_bgzf_dev.hpp's DevWindows.  What follows the inflate differs: a window's inflated bytes are TEXT, and a line may start
// anywhere and straddle any number of members, so nothing here works per member.  decode_device<Job> is the driver: per window it
// builds the line index (a), hands the lines to the job and carries the bytes behind the window's last '\n' to the front of the next.
// A job is start / window / finish, each returning "" or the reason the device path stops, and owns its device buffers and host
// vectors.  Every device read is bounded by the window's length n, whatever the text holds.
//   (a) frag_count_nl / frag_scan / frag_line_starts: every lane loads 16 bytes and builds a newline mask; the per-tile counts are
//       scanned and become the offsets at which the lanes write the line starts.
// PlainJob (natac_frag_open_device; decode_plain):
//   (b) frag_parse: one lane per line runs natac_fragio::parse_line (the host decoder's own classifier) and compares the line's
//       chromosome field byte-wise with the previous data line's: a difference starts a RUN.
//   (c) frag_compact: a scan over (is data, starts a run) gives every data line its output slot and its run; start / end are
//       written in file order, and per run its first slot, the offset and length of its name and its largest end.
//   The host reads the few run names back (RunTable: frag_gather_names), maps them to chromosome ids with the host decoder's dictionary
//   (this is where a chromosome that comes back gets its old id) and appends.
// SplitJob (natac_frag_split_device), splitting by cell barcode:
//   (b') frag_split_parse: frag_parse with natac_fragio::split_line, so every data line also gets its group (or -1) from the barcode
//        table, and the exact per-barcode counts grow by one integer atomic per set of lanes of a wave that share a barcode.
//   (c') frag_split_compact: the run tables over ALL data lines as in (c), and every line's run instead of the compacted start / end.
//   (d') frag_split_hist / frag_scan / frag_split_scatter: a stable partition of the window's assigned lines by group.  One wave owns a
//        tile of PART_LINES consecutive lines; the per-tile counts, stored group-major, scan into every (group, tile)'s first output
//        slot; the wave then walks its tile in file order, 64 lines a round, and gives the lanes of a group consecutive slots in lane
//        order.  The counts of every (group, run) segment come from the same histogram.  Integers only: nothing depends on order.
//   The host gets start / end of the assigned lines only, in group-major order, and the segment counts, and appends segment by segment.
// CellsJob (natac_frag_cells_device), discovering the cells, needs no runs: cells_parse, rounds of cells_claim / cells_verify,
// cells_number / cells_adopt and cells_count build the barcode table from the file itself (see CellsJob below).
// The host decoder answers instead (the caller runs it) for: a malformed line or a damaged file (so both paths give the same message
// by construction), a window without any line end, more than MAX_RUNS runs in a window, a HIP failure;
// when splitting also for a line without a barcode field (malformed), a table of more than SPLIT_DEV_MAX_BARCODES barcodes and more than
// SPLIT_MAX_SEGMENTS groups x runs in a window; when discovering cells for a line without a barcode field, a full table (more than half
// the slots taken: more than SPLIT_DEV_MAX_BARCODES cells with the default size) and more than 268,435,455 lines in a window.
#pragma once
#include <memory>
#include "natac_bgzf_dev.hpp"
#include "natac_fragfile.hpp"

namespace natac_fragdev {

using natac_bgzfdev::DevWindows;
using natac_bgzfdev::DevBuf;
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

// ---- the jobs ----
// what the driver's clock needs of a job: parsed() marks where the "parse" phase of NATAC_FRAG_DEV_TIMING ends inside window()
struct FragJob {
    natac_bgzfdev::Laps *laps = nullptr;
    double t_parse = 0;
    void parsed() { if (laps) laps->lap(t_parse); }
};

// Discovery: the table on the device and the per-window work behind the line index.
struct CellsJob : FragJob {
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

    // "" or what stops the device path
    std::string start(hipStream_t stream) {
        configure();
        NATAC_DEV_TRY(slot.reserve((size_t)n_slots * sizeof(u64)));
        NATAC_DEV_TRY(state.reserve(CELLS_S_WORDS * sizeof(u64)));
        NATAC_DEV_TRY(off.reserve(4096 * sizeof(u64)));
        NATAC_DEV_TRY(arena.reserve(65536));
        NATAC_DEV_TRY(cnt.reserve(3 * 4096 * sizeof(u64)));
        NATAC_DEV_TRY(hipMemsetAsync(slot.p, 0xff, (size_t)n_slots * sizeof(u64), stream));          // CELLS_EMPTY
        NATAC_DEV_TRY(hipMemsetAsync(state.p, 0, CELLS_S_WORDS * sizeof(u64), stream));
        NATAC_DEV_TRY(hipMemsetAsync(off.p, 0, sizeof(u64), stream));                                 // off[0]
        return std::string();
    }

    // the lines of one window (ls[n_lines + 1] into data[0, n))
    std::string window(const unsigned char *data, u64 n, const u64 *ls, u64 n_lines, int open_tail, hipStream_t stream) {
        NATAC_DEV_TRY(hipStreamSynchronize(stream));            // the line index is complete
        if (n_lines >= CELLS_MAX_LINES) return "more than 268,435,455 lines in a window";
        const u64 blocks = (n_lines + TILE_T - 1) / TILE_T;
        NATAC_DEV_TRY(bc_at.reserve((size_t)n_lines * sizeof(u64)));
        NATAC_DEV_TRY(meta.reserve((size_t)n_lines * sizeof(unsigned int)));
        NATAC_DEV_TRY(probe.reserve((size_t)n_lines * sizeof(unsigned int)));
        NATAC_DEV_TRY(bsum.reserve((size_t)blocks * sizeof(u64)));
        u64 *st = (u64 *)state.p;
        NATAC_DEV_TRY(hipMemsetAsync(st + CELLS_S_UNRESOLVED, 0, 2 * sizeof(u64), stream));          // (the flags stay: any of them ends the device path)
        hipLaunchKernelGGL(cells_parse, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, data, ls, n_lines, open_tail, nfr_upper, mono_upper,
                           hash_mask & (n_slots - 1u), (u64 *)bc_at.p, (unsigned int *)meta.p, (unsigned int *)probe.p, st);
        u64 h[3] = {0, 0, 0};                            // unresolved, new, flags
        for (unsigned int round = 0;; ++round) {
            if (round) NATAC_DEV_TRY(hipMemsetAsync(st + CELLS_S_UNRESOLVED, 0, sizeof(u64), stream));
            hipLaunchKernelGGL(cells_claim, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const unsigned int *)probe.p, n_lines, (u64 *)slot.p, n_slots,
                               slot_bits, round);
            hipLaunchKernelGGL(cells_verify, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, data, n, (const u64 *)bc_at.p, (const unsigned int *)meta.p,
                               (unsigned int *)probe.p, n_lines, (const u64 *)slot.p, n_slots, (const unsigned char *)arena.p, (const u64 *)off.p, n_cells,
                               fill, round, st);
            NATAC_DEV_TRY(hipMemcpyAsync(h, st + CELLS_S_UNRESOLVED, sizeof h, hipMemcpyDeviceToHost, stream));
            NATAC_DEV_TRY(hipStreamSynchronize(stream));
            if (h[2] & CELLS_F_MALFORMED) return "a malformed line";
            if (h[2] & CELLS_F_BROKEN) return "the cell table is out of range";
            if (h[2] & CELLS_F_FULL) return "the cell table is full";
            if (h[0] == 0) break;
            if (h[0] > n_lines || round + 1u >= CELLS_MAX_ROUNDS) return "the cell table is full";
        }
        hipLaunchKernelGGL(cells_number, dim3((unsigned)blocks), dim3(TILE_T), 0, stream, (const unsigned int *)probe.p, (const unsigned int *)meta.p,
                           (const u64 *)slot.p, n_slots, n_lines, (u64 *)bsum.p);
        hipLaunchKernelGGL(frag_scan, dim3(1), dim3(1024), 0, stream, (u64 *)bsum.p, blocks, st + CELLS_S_NEW);
        NATAC_DEV_TRY(hipMemcpyAsync(h, st + CELLS_S_NEW, sizeof(u64), hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipStreamSynchronize(stream));
        const u64 n_new = h[0] >> 36, new_bytes = h[0] & ((1ull << 36) - 1ull);
        if (n_new > n_lines || new_bytes > 255 * n_new) return "counts out of range";
        if (n_cells + n_new > n_slots / 2) return "the cell table is full";
        if (n_new) {
            NATAC_DEV_TRY(arena.reserve((size_t)(fill + new_bytes), (size_t)fill, stream));
            NATAC_DEV_TRY(off.reserve((size_t)(n_cells + n_new + 1) * sizeof(u64), (size_t)(n_cells + 1) * sizeof(u64), stream));
            NATAC_DEV_TRY(cnt.reserve((size_t)(n_cells + n_new) * 3 * sizeof(u64), (size_t)n_cells * 3 * sizeof(u64), stream));
            NATAC_DEV_TRY(hipMemsetAsync((u64 *)cnt.p + 3 * n_cells, 0, (size_t)n_new * 3 * sizeof(u64), stream));
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
        NATAC_DEV_TRY(hipGetLastError());
        parsed();
        return std::string();
    }

    // the table comes to the host once, behind the last window
    std::string finish(hipStream_t stream) {
        u64 h[CELLS_S_WORDS];
        std::vector<u64> h_off((size_t)n_cells + 1), h_cnt((size_t)n_cells * 3);
        out->bytes.resize((size_t)fill);
        NATAC_DEV_TRY(hipMemcpyAsync(h, state.p, sizeof h, hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(h_off.data(), off.p, h_off.size() * sizeof(u64), hipMemcpyDeviceToHost, stream));
        if (n_cells) NATAC_DEV_TRY(hipMemcpyAsync(h_cnt.data(), cnt.p, h_cnt.size() * sizeof(u64), hipMemcpyDeviceToHost, stream));
        if (fill) NATAC_DEV_TRY(hipMemcpyAsync(out->bytes.data(), arena.p, (size_t)fill, hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipStreamSynchronize(stream));
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
};

// ---- what PlainJob and SplitJob share: RunTable and LineParse ----
// The runs of a window's data lines (a run: consecutive data lines of one chromosome), as frag_compact / frag_split_compact write them:
// zero() in front of that kernel, gather() behind it, download() in front of the job's synchronise, span() / name() behind it.
struct RunTable {
    DevBuf d_first, d_name, d_nlen, d_max, d_names;
    std::vector<u64> first;
    std::vector<unsigned int> nlen;
    std::vector<int> rmax;
    std::vector<unsigned char> names;
    std::string zero(u64 n_runs, hipStream_t stream) {
        NATAC_DEV_TRY(d_first.reserve((size_t)n_runs * sizeof(u64)));
        NATAC_DEV_TRY(d_name.reserve((size_t)n_runs * sizeof(u64)));
        NATAC_DEV_TRY(d_nlen.reserve((size_t)n_runs * sizeof(unsigned int)));
        NATAC_DEV_TRY(d_max.reserve((size_t)n_runs * sizeof(int)));
        NATAC_DEV_TRY(d_names.reserve((size_t)n_runs * 256));
        NATAC_DEV_TRY(hipMemsetAsync(d_max.p, 0, (size_t)n_runs * sizeof(int), stream));
        NATAC_DEV_TRY(hipMemsetAsync(d_first.p, 0, (size_t)n_runs * sizeof(u64), stream));
        NATAC_DEV_TRY(hipMemsetAsync(d_nlen.p, 0, (size_t)n_runs * sizeof(unsigned int), stream));
        NATAC_DEV_TRY(hipMemsetAsync(d_name.p, 0, (size_t)n_runs * sizeof(u64), stream));
        return std::string();
    }
    void gather(const unsigned char *data, u64 n, u64 n_runs, hipStream_t stream) {
        hipLaunchKernelGGL(frag_gather_names, dim3((unsigned)((n_runs + 63) / 64)), dim3(64), 0, stream, data, n, (const u64 *)d_name.p,
                           (const unsigned int *)d_nlen.p, (unsigned int)n_runs, (unsigned char *)d_names.p);
    }
    std::string download(u64 n_runs, hipStream_t stream) {
        first.resize(n_runs); nlen.resize(n_runs); rmax.resize(n_runs); names.resize((size_t)n_runs * 256);
        NATAC_DEV_TRY(hipMemcpyAsync(first.data(), d_first.p, (size_t)n_runs * sizeof(u64), hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(nlen.data(), d_nlen.p, (size_t)n_runs * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(rmax.data(), d_max.p, (size_t)n_runs * sizeof(int), hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(names.data(), d_names.p, (size_t)n_runs * 256, hipMemcpyDeviceToHost, stream));
        return std::string();
    }
    // run r = the data lines [*a, *b) of the window's n_data; false: the table is out of range
    bool span(size_t r, u64 n_data, u64 *a, u64 *b) const {
        *a = first[r];
        *b = r + 1 < first.size() ? first[r + 1] : n_data;
        return !(*a >= *b || *b > n_data || nlen[r] == 0 || nlen[r] > 255);
    }
    std::string name(size_t r) const { return std::string((const char *)names.data() + r * 256, nlen[r]); }
};

// The per-line arrays frag_parse / frag_split_parse fill, and the counts behind them.  `flag` is the parse kernels' status word: zeroed
// once, so a malformed line ends the device path in the window where it occurs (the counts are read behind every parse).
struct LineParse {
    DevBuf code, start, end, nlen, bsum, total;            // total: the scan's sum, and behind it the flag
    u64 blocks = 0, n_data = 0, n_runs = 0;
    u64 packed = 0;                         // host words of the asynchronous downloads
    int malformed = 0;
    int *flag() const { return (int *)((u64 *)total.p + 1); }
    std::string begin(hipStream_t stream) {
        NATAC_DEV_TRY(total.reserve(2 * sizeof(u64)));
        NATAC_DEV_TRY(hipMemsetAsync(flag(), 0, sizeof(int), stream));
        return std::string();
    }
    std::string reserve(u64 n_lines) {
        blocks = (n_lines + TILE_T - 1) / TILE_T;
        NATAC_DEV_TRY(code.reserve((size_t)n_lines * sizeof(u64)));
        NATAC_DEV_TRY(start.reserve((size_t)n_lines * sizeof(int)));
        NATAC_DEV_TRY(end.reserve((size_t)n_lines * sizeof(int)));
        NATAC_DEV_TRY(nlen.reserve((size_t)n_lines * sizeof(unsigned int)));
        NATAC_DEV_TRY(bsum.reserve((size_t)blocks * sizeof(u64)));
        return std::string();
    }
    // behind the parse kernel: bsum scanned in place (the compaction's block offsets), n_data and n_runs on the host; G: groups (0: no split)
    std::string counts(u64 n_lines, int G, hipStream_t stream) {
        hipLaunchKernelGGL(frag_scan, dim3(1), dim3(1024), 0, stream, (u64 *)bsum.p, blocks, (u64 *)total.p);
        NATAC_DEV_TRY(hipMemcpyAsync(&packed, total.p, sizeof packed, hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(&malformed, flag(), sizeof malformed, hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipStreamSynchronize(stream));
        if (malformed != 0) return "a malformed line";
        n_data = packed >> 32;
        n_runs = packed & 0xffffffffull;
        if (n_data > n_lines || n_runs > n_data) return "counts out of range";
        if (n_runs > MAX_RUNS) return "more than 65,536 chromosome runs in a window";
        if (n_runs * (u64)G > SPLIT_MAX_SEGMENTS) return "more than 1,048,576 groups x chromosome runs in a window";
        return std::string();
    }
};

// ---- the plain decode: (b) frag_parse, (c) frag_compact, the run names, and the append on the host ----
struct PlainJob : FragJob {
    natac_fragio::Builder bd;
    LineParse lp;
    RunTable runs;
    DevBuf d_ostart, d_oend;
    std::vector<int> h_start, h_end;
    std::vector<int64_t> pos, tlen;
    explicit PlainJob(natac_bamio::Bam *bam) : bd(bam) {}
    std::string start(hipStream_t stream) { return lp.begin(stream); }
    std::string window(const unsigned char *data, u64 n, const u64 *ls, u64 n_lines, int open_tail, hipStream_t stream) {
        NATAC_DEV_TRY(lp.reserve(n_lines));
        hipLaunchKernelGGL(frag_parse, dim3((unsigned)lp.blocks), dim3(TILE_T), 0, stream, data, ls, n_lines, open_tail, (u64 *)lp.code.p, (int *)lp.start.p,
                           (int *)lp.end.p, (unsigned int *)lp.nlen.p, (u64 *)lp.bsum.p, lp.flag());
        NATAC_DEV_TRY(lp.counts(n_lines, 0, stream));
        parsed();
        const u64 n_data = lp.n_data, n_runs = lp.n_runs;
        if (!n_data) return std::string();
        NATAC_DEV_TRY(d_ostart.reserve((size_t)n_data * sizeof(int)));
        NATAC_DEV_TRY(d_oend.reserve((size_t)n_data * sizeof(int)));
        NATAC_DEV_TRY(runs.zero(n_runs, stream));
        hipLaunchKernelGGL(frag_compact, dim3((unsigned)lp.blocks), dim3(TILE_T), 0, stream, ls, n_lines, (const u64 *)lp.code.p, (const int *)lp.start.p,
                           (const int *)lp.end.p, (const unsigned int *)lp.nlen.p, (const u64 *)lp.bsum.p, n_data, (unsigned int)n_runs, (int *)d_ostart.p,
                           (int *)d_oend.p, (u64 *)runs.d_first.p, (u64 *)runs.d_name.p, (unsigned int *)runs.d_nlen.p, (int *)runs.d_max.p);
        runs.gather(data, n, n_runs, stream);
        h_start.resize(n_data); h_end.resize(n_data);
        NATAC_DEV_TRY(hipMemcpyAsync(h_start.data(), d_ostart.p, (size_t)n_data * sizeof(int), hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(h_end.data(), d_oend.p, (size_t)n_data * sizeof(int), hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(runs.download(n_runs, stream));
        NATAC_DEV_TRY(hipStreamSynchronize(stream));
        for (size_t r = 0; r < (size_t)n_runs; ++r) {
            u64 a, b;
            if (!runs.span(r, n_data, &a, &b)) return "run table out of range";
            pos.resize((size_t)(b - a));
            tlen.resize((size_t)(b - a));
            for (u64 i = a; i < b; ++i) {
                pos[(size_t)(i - a)] = (int64_t)h_start[(size_t)i] - 4;
                tlen[(size_t)(i - a)] = (int64_t)h_end[(size_t)i] - (int64_t)h_start[(size_t)i] + 8;
            }
            natac_fragio::append_run(bd, runs.name(r), pos.data(), tlen.data(), (size_t)(b - a), runs.rmax[r]);
        }
        return std::string();
    }
    std::string finish(hipStream_t) { return std::string(); }
};

// ---- the split: the table goes up once, (b') to (d') per window, the segments into the builder both paths share, the per-barcode counts
// (table->group.size() of them) at the end ----
struct SplitJob : FragJob {
    const natac_fragio::SplitTableHost *table = nullptr;
    natac_fragio::SplitBuilder *sb = nullptr;
    std::vector<int64_t> bc_count;
    LineParse lp;
    RunTable runs;
    DevBuf d_tb_bytes, d_tb_off, d_tb_group, d_tb_slot, d_bcc, d_grp, d_lrun, d_thist, d_seg, d_assigned, d_ostart, d_oend;
    natac_fragio::SplitTable dev_tb{};
    int bc_bits = 1, G = 0;
    u64 n_assigned = 0;
    std::vector<unsigned int> h_seg;
    std::vector<int> run_chrom, h_start, h_end;
    std::string start(hipStream_t stream) {
        const natac_fragio::SplitTableHost &t = *table;
        G = t.n_groups;
        while (bc_bits < 32 && ((size_t)1 << bc_bits) < t.group.size()) ++bc_bits;
        NATAC_DEV_TRY(d_assigned.reserve(sizeof(u64)));
        NATAC_DEV_TRY(d_tb_bytes.reserve(t.bytes.size()));
        NATAC_DEV_TRY(d_tb_off.reserve(t.off.size() * sizeof(uint32_t)));
        NATAC_DEV_TRY(d_tb_group.reserve(t.group.size() * sizeof(int32_t)));
        NATAC_DEV_TRY(d_tb_slot.reserve(t.slot.size() * sizeof(uint32_t)));
        NATAC_DEV_TRY(d_bcc.reserve(t.group.size() * sizeof(u64)));
        NATAC_DEV_TRY(hipMemcpyAsync(d_tb_bytes.p, t.bytes.data(), t.bytes.size(), hipMemcpyHostToDevice, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(d_tb_off.p, t.off.data(), t.off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(d_tb_group.p, t.group.data(), t.group.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        NATAC_DEV_TRY(hipMemcpyAsync(d_tb_slot.p, t.slot.data(), t.slot.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        NATAC_DEV_TRY(hipMemsetAsync(d_bcc.p, 0, t.group.size() * sizeof(u64), stream));
        NATAC_DEV_TRY(hipStreamSynchronize(stream));
        dev_tb = natac_fragio::SplitTable{(const unsigned char *)d_tb_bytes.p, (const uint32_t *)d_tb_off.p, (const int32_t *)d_tb_group.p,
                                          (const uint32_t *)d_tb_slot.p, (uint32_t)t.group.size(), (uint32_t)t.slot.size(), t.hash_mask};
        return lp.begin(stream);
    }
    std::string window(const unsigned char *data, u64 n, const u64 *ls, u64 n_lines, int open_tail, hipStream_t stream) {
        NATAC_DEV_TRY(lp.reserve(n_lines));
        NATAC_DEV_TRY(d_grp.reserve((size_t)n_lines * sizeof(int)));
        hipLaunchKernelGGL(frag_split_parse, dim3((unsigned)lp.blocks), dim3(TILE_T), 0, stream, data, ls, n_lines, open_tail, dev_tb, bc_bits, (u64 *)lp.code.p,
                           (int *)lp.start.p, (int *)lp.end.p, (unsigned int *)lp.nlen.p, (int *)d_grp.p, (u64 *)d_bcc.p, (u64 *)lp.bsum.p, lp.flag());
        NATAC_DEV_TRY(lp.counts(n_lines, G, stream));
        parsed();
        const u64 n_data = lp.n_data, n_runs = lp.n_runs;
        if (!n_data) return std::string();
        NATAC_DEV_TRY(d_lrun.reserve((size_t)n_lines * sizeof(int)));
        const u64 n_tiles = (n_lines + PART_LINES - 1) / PART_LINES, n_seg = n_runs * (u64)G;
        NATAC_DEV_TRY(d_thist.reserve((size_t)(n_tiles * (u64)G) * sizeof(u64)));
        NATAC_DEV_TRY(d_seg.reserve((size_t)n_seg * sizeof(unsigned int)));
        NATAC_DEV_TRY(runs.zero(n_runs, stream));
        NATAC_DEV_TRY(hipMemsetAsync(d_seg.p, 0, (size_t)n_seg * sizeof(unsigned int), stream));
        hipLaunchKernelGGL(frag_split_compact, dim3((unsigned)lp.blocks), dim3(TILE_T), 0, stream, ls, n_lines, (const u64 *)lp.code.p, (const int *)lp.end.p,
                           (const unsigned int *)lp.nlen.p, (const u64 *)lp.bsum.p, n_data, (unsigned int)n_runs, (u64 *)runs.d_first.p, (u64 *)runs.d_name.p,
                           (unsigned int *)runs.d_nlen.p, (int *)runs.d_max.p, (int *)d_lrun.p);
        runs.gather(data, n, n_runs, stream);
        hipLaunchKernelGGL(frag_split_hist, dim3((unsigned)n_tiles), dim3(PART_T), 0, stream, (const int *)d_grp.p, (const int *)d_lrun.p, n_lines, G,
                           (unsigned int)n_runs, n_tiles, (u64 *)d_thist.p, (unsigned int *)d_seg.p);
        hipLaunchKernelGGL(frag_scan, dim3(1), dim3(1024), 0, stream, (u64 *)d_thist.p, n_tiles * (u64)G, (u64 *)d_assigned.p);
        NATAC_DEV_TRY(hipMemcpyAsync(&n_assigned, d_assigned.p, sizeof n_assigned, hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(runs.download(n_runs, stream));
        h_seg.resize((size_t)n_seg);
        NATAC_DEV_TRY(hipMemcpyAsync(h_seg.data(), d_seg.p, (size_t)n_seg * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipStreamSynchronize(stream));
        if (n_assigned > n_data) return "counts out of range";
        if (n_assigned) {                    // unassigned lines stay on the device
            NATAC_DEV_TRY(d_ostart.reserve((size_t)n_assigned * sizeof(int)));
            NATAC_DEV_TRY(d_oend.reserve((size_t)n_assigned * sizeof(int)));
            hipLaunchKernelGGL(frag_split_scatter, dim3((unsigned)n_tiles), dim3(PART_T), 0, stream, (const int *)d_grp.p, (const int *)d_lrun.p,
                               (const int *)lp.start.p, (const int *)lp.end.p, n_lines, G, (unsigned int)n_runs, n_tiles, (const u64 *)d_thist.p, n_assigned,
                               (int *)d_ostart.p, (int *)d_oend.p);
            h_start.resize(n_assigned); h_end.resize(n_assigned);
            NATAC_DEV_TRY(hipMemcpyAsync(h_start.data(), d_ostart.p, (size_t)n_assigned * sizeof(int), hipMemcpyDeviceToHost, stream));
            NATAC_DEV_TRY(hipMemcpyAsync(h_end.data(), d_oend.p, (size_t)n_assigned * sizeof(int), hipMemcpyDeviceToHost, stream));
            NATAC_DEV_TRY(hipStreamSynchronize(stream));
        }
        run_chrom.resize(n_runs);
        for (size_t r = 0; r < (size_t)n_runs; ++r) {
            u64 a, b;
            if (!runs.span(r, n_data, &a, &b)) return "run table out of range";
            run_chrom[r] = sb->chrom(runs.name(r), runs.rmax[r], (int64_t)(b - a));
        }
        u64 at = 0;                          // the segments, group-major as the partition wrote them
        for (int g = 0; g < G; ++g)
            for (size_t r = 0; r < (size_t)n_runs; ++r) {
                const u64 cnt = h_seg[(size_t)g * (size_t)n_runs + r];
                if (cnt > n_assigned - at) return "segment table out of range";
                for (u64 k = at; k < at + cnt; ++k) sb->append(g, run_chrom[r], h_start[(size_t)k], h_end[(size_t)k]);
                at += cnt;
            }
        if (at != n_assigned) return "segment table out of range";
        return std::string();
    }
    std::string finish(hipStream_t) {
        std::vector<u64> h_bcc(table->group.size());
        bc_count.resize(h_bcc.size());
        NATAC_DEV_TRY(hipMemcpy(h_bcc.data(), d_bcc.p, h_bcc.size() * sizeof(u64), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < h_bcc.size(); ++k) bc_count[k] = (int64_t)h_bcc[k];
        return std::string();
    }
};

// ---- the driver: per window (a), then the job, then the carry of the bytes behind the last '\n' ----
// "" or why the host path answers instead (natac_files.hpp runs it).  A job's window() synchronises the stream before it returns.
template <class Job>
inline std::string decode_device(const char *path, hipStream_t stream, size_t window_bytes, Job &job) {
    DevBuf d_tile, d_ls, d_total;
    DevWindows win;                        // (declared last: it waits for the device before any buffer above is freed)
    NATAC_DEV_TRY(win.open(path, stream, window_bytes, (size_t)256 << 20));
    NATAC_DEV_TRY(d_total.reserve(sizeof(u64)));
    NATAC_DEV_TRY(job.start(stream));
    job.laps = &win.laps;
    double t_lines = 0, t_out = 0;
    const DevWindows::Window &w = win.w;
    for (;;) {
        NATAC_DEV_TRY(win.next());
        if (w.M == 0) break;                // the whole chain is done
        const unsigned char *data = w.data;
        const u64 n = w.n;
        u64 cur = 0;                        // the carry into the next window starts here
        if (n > 0) {
            const u64 tiles = (n + TILE_B - 1) / TILE_B;
            NATAC_DEV_TRY(d_tile.reserve((size_t)tiles * sizeof(u64)));
            hipLaunchKernelGGL(frag_count_nl, dim3((unsigned)tiles), dim3(TILE_T), 0, stream, data, n, (u64 *)d_tile.p);
            hipLaunchKernelGGL(frag_scan, dim3(1), dim3(1024), 0, stream, (u64 *)d_tile.p, tiles, (u64 *)d_total.p);
            u64 n_nl = 0;
            unsigned char last_byte = 0;
            NATAC_DEV_TRY(hipMemcpyAsync(&n_nl, d_total.p, sizeof n_nl, hipMemcpyDeviceToHost, stream));
            NATAC_DEV_TRY(hipMemcpyAsync(&last_byte, data + n - 1, 1, hipMemcpyDeviceToHost, stream));
            NATAC_DEV_TRY(hipStreamSynchronize(stream));
            if (n_nl > n) return "line count out of range";
            const int open_tail = w.eof && last_byte != '\n' ? 1 : 0;      // a last line without '\n' is a line
            const u64 n_lines = n_nl + (u64)open_tail;
            if (n_lines == 0) return "a window without a line end (a line longer than a window)";
            NATAC_DEV_TRY(d_ls.reserve((size_t)(n_lines + 2) * sizeof(u64)));
            u64 *ls = (u64 *)d_ls.p;
            const u64 zero = 0, behind = n + 1;
            NATAC_DEV_TRY(hipMemcpyAsync(ls, &zero, sizeof zero, hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(frag_line_starts, dim3((unsigned)tiles), dim3(TILE_T), 0, stream, data, n, (const u64 *)d_tile.p, n_nl, ls);
            if (open_tail) NATAC_DEV_TRY(hipMemcpyAsync(ls + n_lines, &behind, sizeof behind, hipMemcpyHostToDevice, stream));
            NATAC_DEV_TRY(hipMemcpyAsync(&cur, ls + n_nl, sizeof cur, hipMemcpyDeviceToHost, stream));      // (arrives with the job's first synchronise)
            win.laps.lap(t_lines);
            NATAC_DEV_TRY(job.window(data, n, (const u64 *)ls, n_lines, open_tail, stream));
            if (cur > n) return "counts out of range";
            if (open_tail) cur = n;
        }
        NATAC_DEV_TRY(win.carry(cur));
        win.laps.lap(t_out);
        if (w.eof) break;
    }
    if (getenv("NATAC_FRAG_DEV_TIMING"))
        std::fprintf(stderr, "[natac_frag_dev] read + upload %.3f s, waiting for the member chain %.3f, inflate %.3f, line index %.3f, parse %.3f, compaction + append + carry %.3f\n",
                     win.t_read, win.t_chain, win.t_inflate, t_lines, job.t_parse, t_out);
    if (win.pend != 0) return "bytes left behind the last window";
    return job.finish(stream);
}

// Returns the same object as natac_fragio::decode, or nullptr: the host decoder answers (`why` says what stopped the device path).
inline natac_bamio::Bam *decode_plain(const char *path, hipStream_t stream, std::string &why, size_t window_bytes) {
    std::unique_ptr<natac_bamio::Bam> bam(new natac_bamio::Bam());
    PlainJob job(bam.get());
    why = decode_device(path, stream, window_bytes, job);
    return why.empty() ? bam.release() : nullptr;
}

}  // namespace natac_fragdev
