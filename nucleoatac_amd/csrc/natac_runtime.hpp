// natac_runtime.hpp -- what every entry point of the library stands on, host side: the error state (fail, HIPCHK), the caching device
// pool and the owner of its blocks (PoolBuf), the context and the batch (natac_ctx, natac_batch), the event profile, the scope of one
// per-call device operation (DeviceCall) and the device scans its callers share.  The library is one translation unit (natac_api.hip);
// every header that holds entry points includes this one.
#pragma once
#include "../../include/natac.h"
#include "natac_textz.hpp"      // natac_text::P10, natac_deflate::CrcTables (natac_textfmt.hpp, natac_deflate.hpp) and the scan kernels

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(e_ == hipErrorOutOfMemory ? NATAC_E_NOMEM : NATAC_E_HIP, "%s: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                   \
    } while (0)

static hipError_t pool_alloc(void **p, size_t bytes);     // the caching pool, defined below
static void dev_free(void *p);

// The owner of one pool block of n elements of T (move-only): the block goes back to the pool when the owner is reset or destroyed,
// so whoever holds it must know the block's queued work has finished by then -- the context and the batch free theirs after draining
// their stream, a call's temporaries live in a DeviceCall.  Converts to T * for launches and copies.
template <class T>
class PoolBuf {
  public:
    PoolBuf() = default;
    PoolBuf(PoolBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    PoolBuf &operator=(PoolBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~PoolBuf() { reset(); }
    void reset() { dev_free(p_); p_ = nullptr; n_ = 0; }
    // the old block goes first; n == 0 takes one element.  On failure the owner stays empty.
    hipError_t alloc(size_t n) {
        reset();
        if (n == 0) n = 1;
        void *p = nullptr;
        const hipError_t e = pool_alloc(&p, n * sizeof(T));
        if (e == hipSuccess) { p_ = (T *)p; n_ = n; }
        return e;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t size() const { return n_; }

  private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

template <class T>
static int dev_alloc(PoolBuf<T> &buf, size_t n) {
    HIPCHK(buf.alloc(n));
    return NATAC_OK;
}

struct natac_ctx {
    int device = 0;
    hipStream_t stream = nullptr;    // every stage, uploads, drop-ins: one stream
    hipStream_t copy_stream = nullptr;   // natac_batch_format_fetch_begin: a finished result leaves the device while the next track is formatted
    hipDeviceProp_t prop;
    // constants
    PoolBuf<double> d_vmat, d_vmat_pad, d_srow, d_sizes;   // d_vmat_pad: VMatDev::matp
    PoolBuf<double> d_lrt;           // VMatDev::lrt (natac_lr_table), formed for model generation lrt_gen
    long long lrt_gen = -1;
    PoolBuf<double> d_ctab;          // VMatDev::ctab (natac_cand_table), formed for model generation ctab_gen
    long long ctab_gen = -1;
    int vlower = 0, vupper = 0, vw = 0, R = 0, W = 0, sizes_upper = 0;
    bool have_vmat = false, have_sizes = false, srow_dirty = true;
    bool vmat_zero = false, srow_zero = false;
    long long model_gen = 0;         // bumped by natac_set_vmat / natac_set_sizes
    // FFT background path: twiddles (once) and template spectra (per V-plot)
    PoolBuf<double> d_fft_tw, d_fft_k;
    PoolBuf<double> d_fft_mtab, d_fft_swt;   // natac_fft_edge_table_mfma (the edge pass of extended tiles)
    bool smooth_fused = true;        // NATAC_SMOOTH_FUSED=0: natac_run_nuc smooths itself, the peak search reads both tracks (A-B timing / validation)
    bool bg_ext = true;              // NATAC_BG_EXT=0: no extended FFT tiles (A-B timing / validation of the edge pass)
    bool fft_dirty = true, bg_direct = false, occ_ordered = true, occ_zero_nfr = false;
    std::vector<double> h_sizes;
    PoolBuf<double> d_nucp, d_nfrp, d_alphas;
    int occ_upper = 0, n_alpha = 0, step = 0, halfstep = 0, flank = 0;
    double cutoff = 0;
    bool have_occ = false;
    int occ_zero_flags = 0;          // zero pattern of nuc_probs / nfr_probs (bits as in the MLE kernel)
    // fast occupancy path (natac_occ_fast.hpp): model tables + eligibility
    PoolBuf<double> d_occ_q4, d_occ_rho;
    int occ_nm = 0;
    bool occ_fast_ok = false, occ_force_general = false, occ_rn16 = false;
    double occ_b_floor = 0;          // see OccModelDev::b_floor
    // gaussian windows (cached by (M, sd))
    PoolBuf<double> d_win_nuc, d_win_occ;
    PoolBuf<double> d_wb_occ;        // block weights of natac_occ_smooth_blk for (win_occ_M, wb_step)
    int wb_M = 0, wb_step = 0;
    int win_nuc_M = 0, win_occ_M = 0;
    double win_nuc_sd = -1, win_occ_sd = -1;
    double win_nuc_sum = 0, win_occ_sum = 0;   // sequential sums of the window values (the all-valid denominator)
    // profiling
    bool profiling = false;
    struct Ev { int k; hipEvent_t a, b; hipStream_t st; };
    std::vector<Ev> pending;
    double prof_ms[NATAC_K_COUNT] = {0};
    int64_t prof_n[NATAC_K_COUNT] = {0};
    hipEvent_t t0 = nullptr, t1 = nullptr;
    // shader-clock trace (natac_clock_trace_*): a one-wave sampler kernel on its own stream + where the profiled launches fall on its time axis
    hipStream_t ck_stream = nullptr;
    hipEvent_t ck_start = nullptr;
    long long *d_ck = nullptr;       // [0] = samples written, [1] = stop flag, then (wall ticks, shader cycles) pairs
    int ck_cap = 0;
    bool ck_active = false;
    struct Iv { int k; float t0, t1; };
    std::vector<Iv> ck_iv;
    // device-side track writer (natac_textz.hpp): power-of-ten table of the '%.12g' formatter, CRC-32 tables
    PoolBuf<natac_text::P10> d_p10;
    PoolBuf<natac_deflate::CrcTables> d_crc;
};

// What each output of a batch holds and who wrote it: the stages and natac_batch_set_track write it, every reader asks need_track().
// PENDING: formed on the first request from what the stage left (BACKGROUND from d_bnum / d_bcov, OCC_PREFILL from the grids, SMOOTH
// from NORM with the window natac_run_nuc was asked for -- by the peak search itself if that is the first reader).
enum TrackState : unsigned char { TS_EMPTY = 0, TS_PENDING, TS_RUN /* a natac_run_* stage */, TS_HOST /* natac_batch_set_track */ };
struct BatchOutputs {
    TrackState track[NATAC_T_COUNT] = {};
    bool grids = false;               // d_grid written by natac_run_occ
    long long bg_gen = -1;            // model generation d_bnum / d_bcov were formed with (natac_run_nuc); -1: none
    int nuc_w = -1, nuc_lower = -1, nuc_upper = -1;   // V-plot geometry natac_run_nuc ran with (its tracks depend on it); -1: no run
    bool occ_cov_by_nuc = false;      // OCC_COV holds natac_run_nuc's nuc_cov + nfr_cov for that geometry
    int smooth_M = 0;                 // window (length, sd) natac_run_nuc was asked for: what a pending SMOOTH is formed with
    double smooth_sd = 0;
    // occupancy geometry natac_run_occ ran with (the grids and the OCC tracks depend on it); -1: no run
    int occ_step = -1, occ_half = -1, occ_flank = -1, occ_upper = -1;
};

struct natac_batch {
    natac_ctx *ctx = nullptr;
    int nc = 0, max_len = 0;          // chunks, and the longest one's bases
    long long nf = 0, nb = 0, total_bp = 0, total_grid = 0;
    int bias_left = 0, bias_right = 0;
    std::vector<int> h_len;
    std::vector<long long> h_out_off, h_grid_off;
    PoolBuf<int> d_len, d_lpos, d_ilen, d_centre, d_status;
    PoolBuf<long long> d_frag_off, d_bias_off, d_out_off, d_grid_off;
    PoolBuf<double> d_bias, d_ebias;
    PoolBuf<unsigned long long> d_occ_minkey;   // natac_occ_smooth_blk: per-chunk minimum finite smoothed occupancy (double_key)
    PoolBuf<int> d_occ_nan;
    int n_tiles_os = 0, os_width = 0;
    PoolBuf<int2> d_tiles_os, d_tiles1k;
    int n_tiles1k = 0;
    PoolBuf<int2> d_tiles256, d_tiles_bg, d_tiles_occ, d_ranges_occ, d_ranges256;
    PoolBuf<long long> d_tile256_first;   // [nc + 1] first 256-base tile of every chunk (the candidates' way into d_ranges256)
    PoolBuf<int> d_order_occ;        // natac_tile_heavy: {count, claims, list[HEAVY_CAP], flag bytes[n_tiles_occ]} of the occupancy tiles
    int ranges256_w = -1;
    int ranges_occ_key[3] = {-1, -1, -1};   // (step, halfstep, flank) the occupancy tiles' fragment ranges were formed for
    int n_tiles256 = 0, n_tiles_bg = 0, n_tiles_occ = 0, bgG = 0;   // bgG: lanes' output count of the direct kernel, -1 = FFT tiles
    int grid_step = 0, grid_half = 0;
    // fast occupancy path: per-block sums of g_n / g_f, their tile table and the list of tiles left to natac_occ_mle
    PoolBuf<long long> d_blk_off;
    long long total_blocks = 0;
    PoolBuf<double> d_gsum;
    PoolBuf<int2> d_tiles_gs;
    int n_tiles_gs = 0, gs_Q = -1;
    PoolBuf<int> d_defer;            // [0] = count, [1 ..] = tile indices
    // occupancy peaks (natac_run_occ_peaks): OccPeak values + keep flags of the last search (opk_cap apart), per-chunk nuc_dist
    PoolBuf<double> d_opk_vals, d_nuc_dist;
    PoolBuf<int> d_opk_keep;
    long long opk_cap = 0, opk_n = -1;
    int nd_upper = 0;
    PoolBuf<double> d_track[NATAC_T_COUNT];
    PoolBuf<double> d_grid[3];
    BatchOutputs out;
    bool ebias_fresh = false;
    // device-side candidate search
    // (d_pk_chunk, d_pk_pos and the three columns of d_pk_out hold pk_cap candidates each)
    PoolBuf<double> d_jitter, d_pk_out;
    PoolBuf<long long> d_cap_off, d_pk_offs;
    PoolBuf<int> d_slot, d_pk_count, d_pk_chunk, d_pk_pos;
    PoolBuf<double> d_pk_big;         // natac_peaks_chunk: global (sig, pos, state) lists of chunks with more maxima than fit in LDS
    long long n_jitter = 0, pk_cap = 0, pk_n = -1, slot_total = 0;
    int pk_order = -1;
    bool pk_has_stats = false;
    PoolBuf<double> d_bnum, d_bcov;                // per-base sum B V / sum B of the background kernel (candidate statistics)
    PoolBuf<unsigned char> d_fmt_out;              // result of the last natac_batch_format_track (text or BGZF members)
    std::vector<std::pair<PoolBuf<unsigned char>, hipEvent_t>> fmt_pending;   // results on their way to the host (natac_batch_format_fetch_begin)
    long long fmt_bytes = -1;
    // tabix records of that result (compress mode): runs of lines per leaf bin, member offsets, chromosome names
    std::vector<natac_textz::GroupRec> fmt_groups;
    std::vector<unsigned long long> fmt_member_pos;
    std::vector<std::string> fmt_names;
    long long fmt_text_bytes = 0;
};

static hipError_t sync_all(natac_ctx *c) { return hipStreamSynchronize(c->stream); }

static void prof_begin(natac_ctx *c, int k, natac_ctx::Ev &ev, hipStream_t st = nullptr) {
    ev.k = k;
    ev.a = ev.b = nullptr;
    ev.st = nullptr;
    if (!c->profiling) return;
    (void)hipEventCreate(&ev.a);
    (void)hipEventCreate(&ev.b);
    ev.st = st ? st : c->stream;
    (void)hipEventRecord(ev.a, ev.st);
}
static void prof_end(natac_ctx *c, natac_ctx::Ev &ev) {
    if (!c->profiling) return;
    (void)hipEventRecord(ev.b, ev.st);
    c->pending.push_back(ev);
}
static void prof_collect(natac_ctx *c) {
    for (auto &e : c->pending) {
        float ms = 0;
        if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            c->prof_ms[e.k] += ms;
            c->prof_n[e.k] += 1;
            float t0 = 0, t1 = 0;
            if (c->ck_active && hipEventElapsedTime(&t0, c->ck_start, e.a) == hipSuccess &&
                hipEventElapsedTime(&t1, c->ck_start, e.b) == hipSuccess)
                c->ck_iv.push_back({e.k, t0, t1});
        }
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    c->pending.clear();
}

// Device memory goes through a small caching pool (per device, shared by the contexts of a process, thread-safe): a freed block
// is kept and handed to the next request of (nearly) the same size.  Batches of similar shape follow each other in every
// driver (run_occ / run_nuc / bench), and hipMalloc / hipFree synchronise the whole device -- which would also stall the
// streams of OTHER contexts that overlap their copies with this one's kernels.  Every use of a block is ordered on its
// context's stream and a batch is only freed after that stream has drained (natac_batch_free), so reuse is safe.
// NATAC_POOL=0 disables the cache; natac_pool_trim() returns the cached blocks to the driver.
struct DevPool {
    std::mutex mu;
    std::multimap<size_t, void *> free_blocks[16];          // per device
    std::unordered_map<void *, std::pair<int, size_t>> live;  // ptr -> (device, bytes)
    bool enabled = true;
    DevPool() { const char *e = getenv("NATAC_POOL"); enabled = !(e && e[0] == '0'); }
    void trim_locked(int dev) {
        for (auto &kv : free_blocks[dev]) (void)hipFree(kv.second);
        free_blocks[dev].clear();
    }
};
static DevPool g_pool;

static hipError_t pool_alloc(void **p, size_t bytes) {
    *p = nullptr;
    bytes = (bytes + 255) & ~(size_t)255;
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev &= 15;
    std::lock_guard<std::mutex> lk(g_pool.mu);
    if (g_pool.enabled) {
        auto it = g_pool.free_blocks[dev].lower_bound(bytes);
        if (it != g_pool.free_blocks[dev].end() && it->first <= bytes + bytes / 8 + 4096) {
            *p = it->second;
            g_pool.live[*p] = {dev, it->first};
            g_pool.free_blocks[dev].erase(it);
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipErrorOutOfMemory && !g_pool.free_blocks[dev].empty()) {      // give the cached blocks back and retry
        (void)hipGetLastError();
        g_pool.trim_locked(dev);
        e = hipMalloc(p, bytes);
    }
    if (e == hipSuccess) g_pool.live[*p] = {dev, bytes};
    else (void)hipGetLastError();      // reported through the return value; a later hipGetLastError() on this thread must not see it again
    return e;
}

// bytes the device could still hand out: what the driver reports as free + the blocks this process caches for reuse
static hipError_t pool_mem_info(int dev, size_t *avail, size_t *total) {
    size_t fr = 0, tot = 0;
    hipError_t e = hipMemGetInfo(&fr, &tot);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(g_pool.mu);
    for (auto &kv : g_pool.free_blocks[dev & 15]) fr += kv.first;
    *avail = fr;
    *total = tot;
    return hipSuccess;
}

static void dev_free(void *p) {
    if (!p) return;
    std::lock_guard<std::mutex> lk(g_pool.mu);
    auto it = g_pool.live.find(p);
    if (it == g_pool.live.end()) { (void)hipFree(p); return; }
    const int dev = it->second.first;
    const size_t bytes = it->second.second;
    g_pool.live.erase(it);
    if (g_pool.enabled) g_pool.free_blocks[dev].insert({bytes, p});
    else (void)hipFree(p);
}

template <class T>
static int dev_upload(natac_ctx *c, PoolBuf<T> &buf, const T *src, size_t n) {
    int rc = dev_alloc(buf, n);
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpyAsync(buf, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return NATAC_OK;
}

// One per-call device operation on the context's stream, from selecting the device to reporting the result: the call's device
// temporaries, its copies in and out, optional event timing of its kernels, and one finishing step.  The first HIP error is latched:
// after it uploads, memsets and fetches do nothing, the caller asks ok() before it launches, and finish() reports "<name>: <error>"
// (NATAC_E_NOMEM for a failed allocation, NATAC_E_HIP otherwise).
// The temporaries go back to the pool when the scope ends.  The pool may hand a freed block to another context at once, so a block
// may go back only once the stream has finished with it: finish() has seen to that; a scope left without it may have kernels or
// copies queued, and then drains the stream before it frees.
namespace {
class DeviceCall {
  public:
    DeviceCall(natac_ctx *c, const char *name) : c_(c), name_(name) { note(hipSetDevice(c->device)); }
    DeviceCall(const DeviceCall &) = delete;
    DeviceCall &operator=(const DeviceCall &) = delete;
    ~DeviceCall() {
        if (!bufs_.empty() && hipStreamQuery(c_->stream) != hipSuccess) (void)hipStreamSynchronize(c_->stream);
        if (t0_) (void)hipEventDestroy(t0_);
        if (t1_) (void)hipEventDestroy(t1_);
    }
    bool ok() const { return e_ == hipSuccess; }
    void launched() { note(hipGetLastError()); }      // right after every launch
    // device temporaries of n elements (n == 0 takes one element); nullptr once a step has failed
    template <class T>
    T *alloc(size_t n) {
        if (!ok()) return nullptr;
        bufs_.emplace_back();
        note(bufs_.back().alloc(std::max<size_t>(n, 1) * sizeof(T)));
        return (T *)bufs_.back().get();
    }
    template <class T>
    T *zeroed(size_t n) {
        T *p = alloc<T>(n);
        zero(p, n);
        return p;
    }
    template <class T>
    T *upload(const T *src, size_t n) {
        T *p = alloc<T>(n);
        send(p, src, n);
        return p;
    }
    // the stream's memset and copies, in elements of T
    template <class T>
    void zero(T *dst, size_t n) {
        if (ok() && n) note(hipMemsetAsync(dst, 0, n * sizeof(T), c_->stream));
    }
    template <class T>
    void send(T *dst, const T *src, size_t n) {
        if (ok() && n) note(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, c_->stream));
    }
    template <class T>
    void fetch(void *dst, const T *src, size_t n) {
        if (ok() && n) note(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, c_->stream));
    }
    // device events around the kernels of the call: *ms (may be NULL: no timing) is written by finish()
    void time_begin(double *ms) {
        if (!ms || !ok()) return;
        note(hipEventCreate(&t0_));
        if (ok()) note(hipEventCreate(&t1_));
        if (ok()) note(hipEventRecord(t0_, c_->stream));
        ms_ = ms;
    }
    void time_end() {
        if (ms_ && ok()) note(hipEventRecord(t1_, c_->stream));
    }
    // a profile event around the launches between the two (collected by finish())
    void prof_begin(int k) { ::prof_begin(c_, k, ev_, c_->stream); profiled_ = true; }
    void prof_end() { ::prof_end(c_, ev_); }
    // waits for what has been queued -- also after a failure, so that nothing of the call is still running -- and reports the latch.
    // For a call of several phases that needs a value on the host before it goes on; the last wait of a call is finish().
    int sync() {
        note(hipStreamSynchronize(c_->stream));
        return report();
    }
    // the one finishing step of a call: wait, read the timer, collect the profile events, report
    int finish() {
        note(hipStreamSynchronize(c_->stream));
        if (ms_ && ok()) {
            float f = 0;
            note(hipEventElapsedTime(&f, t0_, t1_));
            *ms_ = f;
        }
        if (profiled_) prof_collect(c_);
        return report();
    }

  private:
    void note(hipError_t e) { if (e_ == hipSuccess) e_ = e; }
    int report() const {
        if (ok()) return NATAC_OK;
        return fail(e_ == hipErrorOutOfMemory ? NATAC_E_NOMEM : NATAC_E_HIP, "%s: %s", name_, hipGetErrorString(e_));
    }
    natac_ctx *c_;
    const char *name_;
    hipError_t e_ = hipSuccess;
    std::vector<PoolBuf<unsigned char>> bufs_;
    hipEvent_t t0_ = nullptr, t1_ = nullptr;
    double *ms_ = nullptr;
    natac_ctx::Ev ev_;
    bool profiled_ = false;
};
}  // namespace

// exclusive scan of in[0..n) into out[0..n], out[n] = total (device arrays; n > 0).  The block sums are a temporary of the CALLER's scope
// (`dc`, freed after the caller's last synchronisation): freeing them here needed a stream synchronisation per scan -- six per formatted
// track -- because the pool may hand a freed block to another context at once.  A failure stays in the scope's latch.
template <class T>
static void dev_scan(natac_ctx *c, const T *in, long long n, unsigned long long *out, DeviceCall &dc) {
    using namespace natac_textz;
    const long long nblk = (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK;
    unsigned long long *sums = dc.alloc<unsigned long long>((size_t)nblk + 1);
    if (!dc.ok()) return;
    hipLaunchKernelGGL((tz_scan_block_sums<T>), dim3((unsigned)nblk), dim3(256), 0, c->stream, in, n, sums);
    hipLaunchKernelGGL(tz_scan_sums, dim3(1), dim3(1024), 0, c->stream, sums, nblk);
    hipLaunchKernelGGL((tz_scan_final<T>), dim3((unsigned)nblk), dim3(256), 0, c->stream, in, n, sums, out);
    dc.launched();
}

// the two scans over a track's runs (byte offsets and indices of its lines) in one pass over the length array (tz_scan2_*)
static void dev_scan2(natac_ctx *c, const unsigned char *in, long long n, unsigned long long *out_sum, unsigned long long *out_cnt, DeviceCall &dc) {
    using namespace natac_textz;
    const long long nblk = (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK;
    unsigned long long *sums = dc.alloc<unsigned long long>(2 * ((size_t)nblk + 1));
    if (!dc.ok()) return;
    hipLaunchKernelGGL(tz_scan2_block_sums, dim3((unsigned)nblk), dim3(256), 0, c->stream, in, n, nblk, sums);
    hipLaunchKernelGGL(tz_scan_sums, dim3(1), dim3(1024), 0, c->stream, sums, nblk);
    hipLaunchKernelGGL(tz_scan_sums, dim3(1), dim3(1024), 0, c->stream, sums + nblk + 1, nblk);
    hipLaunchKernelGGL(tz_scan2_final, dim3((unsigned)nblk), dim3(256), 0, c->stream, in, n, nblk, sums, out_sum, out_cnt);
    dc.launched();
}

// What the headers' entry points take from the batch pipeline, which natac_api.hip defines after them ...
static int need_track(natac_batch *b, int t);          // every read of an output track: NATAC_E_STATE if it holds nothing, formed if pending
static natac::OccModelDev make_occ(natac_ctx *c);      // the context's occupancy model as the kernels take it
// ... and what the pipeline takes from the track writer (natac_trackio.hpp)
static int fmt_pending_wait(natac_batch *b);
