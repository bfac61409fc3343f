// natac_api.hip -- the library's one translation unit: the C-ABI of include/natac.h.  This file holds the context and its model
// setters and the batch pipeline (batches of packed chunks resident in HBM, tile tables, the natac_run_* stages, peaks, downloads); every
// other family of entry points sits in the header of its kernels, over the runtime of natac_runtime.hpp (DESIGN.md section 3 has the map).
#include "../../include/natac.h"
#ifndef NATAC_GNBL
#define NATAC_GNBL 2
#endif
#include "natac_kernels.hpp"
#include "natac_fft_bg.hpp"
#include "natac_occ_fast.hpp"
#include "natac_cand.hpp"
#include "natac_covsweep.hpp"
#include "natac_textz.hpp"
#include "natac_cores.hpp"
#include "natac_writer.hpp"
#include "natac_tabix.hpp"
#include "natac_pack.hpp"
#include "natac_bam.hpp"
#include "natac_bam_dev.hpp"
#include "natac_fragfile.hpp"
#include "natac_fragfile_dev.hpp"
#include "natac_fasta.hpp"
#include "natac_fuzzfit.hpp"
#include "natac_bedtab.hpp"
#include "natac_runtime.hpp"
#include "natac_pwmfit.hpp"
#include "natac_sites.hpp"
#include "natac_cellcounts.hpp"
#include "natac_cellqc.hpp"
#include "natac_lsi.hpp"
#include "natac_peakcall.hpp"
#include "natac_motifs.hpp"
#include "natac_deviations.hpp"
#include "natac_markers.hpp"
#include "natac_coaccess.hpp"
#include "natac_genescores.hpp"
#include "natac_knn.hpp"
#include "natac_peaks.hpp"
#include "natac_tracks.hpp"
#include "natac_dropins.hpp"
#include "natac_trackio.hpp"
#include "natac_files.hpp"
#include "natac_store.hpp"
#include "natac_profile.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace natac;

// Contract B of natac.h: a call that combines what an earlier stage left on the batch with the context's model goes on only while
// the context holds the geometry that stage ran with; NATAC_E_STATE otherwise, before any HIP call.  Values may differ (the readers
// below take none of them from the earlier run's model).  Outputs no stage wrote (natac_batch_set_track alone) carry no geometry.
static int need_nuc_geometry(const natac_batch *b, const char *who) {
    const natac_ctx *c = b->ctx;
    const BatchOutputs &o = b->out;
    if (o.nuc_w < 0 || (o.nuc_w == c->vw && o.nuc_lower == c->vlower && o.nuc_upper == c->vupper)) return NATAC_OK;
    return fail(NATAC_E_STATE, "%s: natac_run_nuc ran with the V-plot geometry lower=%d upper=%d w=%d, the context now holds lower=%d "
                "upper=%d w=%d: run natac_run_nuc again", who, o.nuc_lower, o.nuc_upper, o.nuc_w, c->vlower, c->vupper, c->vw);
}
static int need_occ_geometry(const natac_batch *b, const char *who) {
    const natac_ctx *c = b->ctx;
    const BatchOutputs &o = b->out;
    if (o.occ_step < 0 || (o.occ_step == c->step && o.occ_half == c->halfstep && o.occ_flank == c->flank && o.occ_upper == c->occ_upper))
        return NATAC_OK;
    return fail(NATAC_E_STATE, "%s: natac_run_occ ran with step=%d flank=%d upper=%d, the context now holds step=%d flank=%d upper=%d: "
                "run natac_run_occ again", who, o.occ_step, o.occ_flank, o.occ_upper, c->step, c->flank, c->occ_upper);
}

// pick the per-lane output count G of the background kernel: minimise idle lanes (sum of tile widths) with a small
// penalty for the halo work of narrow tiles.
static int choose_bg_G(const natac_batch *b, int W) {
    const int cand[4] = {7, 9, 13, 17};
    double best = 1e300;
    int bestG = 9;
    // histogram-free: sample up to 65536 chunks evenly
    const int stride = std::max(1, b->nc / 65536);
    for (int ci = 0; ci < 4; ++ci) {
        const int G = cand[ci], TW = 64 * G;
        double cost = 0;
        for (int i = 0; i < b->nc; i += stride) {
            const int nt = (b->h_len[i] + TW - 1) / TW;
            cost += (double)nt * (TW + (W - 1) * 0.15 * 8);
        }
        if (cost < best) { best = cost; bestG = G; }
    }
    return bestG;
}

static void launch_candidates(natac_ctx *c, const ChunkTable &ct, const VMatDev &vm, const int *d_cc, const int *d_cp, long long n,
                              const double *nuc_cov, const double *norm, const double *bnum, const double *bcov, double *lr,
                              double *var, double *z, const long long *tile_first = nullptr, const int2 *ranges256 = nullptr) {
    const int EW = c->W + ((c->vupper - 2) >> 1) + ((c->vupper - 1) >> 1);
    const int ZN = (((c->vupper - 2) >> 1) + ((c->vupper - 1) >> 1) + 5 + 32) & ~1, ON = (c->W + 1) & ~1;
    const size_t lds4 = ((size_t)4 * CAND_PER_WAVE * ((EW + 1) & ~1) + ZN + ON) * sizeof(double);
    // The paired-row and four-per-wave kernels give each lane the template columns `lane` and `lane + 64`, nothing more: templates
    // wider than 128 columns take natac_candidates (a column loop), whatever NATAC_CAND_OLD / NATAC_CAND_FULL ask for.
    const bool per_wave = c->W <= 2 * WAVE;
    // paired-row kernel (natac_cand.hpp): needs the background kernel's window sums, no single-cell row, whole row pairs, a template
    // 64 to 128 columns wide (every lane's first column exists) and
    // a model without exact zeros (those take the per-cell zero test of natac_candidates4).  NATAC_CAND_OLD=1: validation.
    const size_t ldsp = (size_t)4 * CAND_PER_WAVE * CANDP_STRIDE * sizeof(double);
    bool paired = per_wave && bnum && bcov && c->vlower >= 2 && (c->R & 1) == 0 && c->W >= 64 && !vm.has_zero && EW <= CANDP_STRIDE &&
                  !getenv("NATAC_CAND_FULL") && !getenv("NATAC_CAND_OLD");
    if (paired && (c->lrt_gen != c->model_gen || !c->d_lrt)) {      // log(V / s) of the current model, on the launch stream (natac_lr_table)
        if (c->d_lrt.size() < (size_t)c->R * c->W && dev_alloc(c->d_lrt, (size_t)c->R * c->W) != NATAC_OK)
            paired = false;                                          // out of memory: the per-cell kernel below needs no table
        if (paired) {
            hipLaunchKernelGGL(natac_lr_table, dim3((unsigned)((c->R * c->W + 255) / 256)), dim3(256), 0, c->stream, c->d_vmat, c->d_srow, c->R, c->W,
                               c->d_lrt);
            c->lrt_gen = c->model_gen;
        }
    }
    if (paired && (c->ctab_gen != c->model_gen || !c->d_ctab)) {    // the sweep's template stream, likewise (natac_cand_table)
        const size_t nd = cand_table_doubles(c->R);
        if (c->d_ctab.size() < nd && dev_alloc(c->d_ctab, nd) != NATAC_OK) paired = false;
        if (paired) {
            hipLaunchKernelGGL(natac_cand_table, dim3((unsigned)((nd / 2 + 255) / 256)), dim3(256), 0, c->stream, c->d_vmat, c->R, c->W, c->d_ctab);
            c->ctab_gen = c->model_gen;
        }
    }
    if (paired) {
        VMatDev vml = vm;
        vml.lrt = c->d_lrt;
        vml.ctab = c->d_ctab;
        const long long per_block = 4 * CAND_PER_WAVE;
        const dim3 grid((unsigned)((n + per_block - 1) / per_block));
        if (c->vlower & 1)
            hipLaunchKernelGGL((natac_candidates_paired<true>), grid, dim3(256), ldsp, c->stream, ct, vml, d_cc, d_cp, (int)n, nuc_cov, norm,
                               bnum, bcov, tile_first, ranges256, lr, var, z);
        else
            hipLaunchKernelGGL((natac_candidates_paired<false>), grid, dim3(256), ldsp, c->stream, ct, vml, d_cc, d_cp, (int)n, nuc_cov, norm,
                               bnum, bcov, tile_first, ranges256, lr, var, z);
        return;
    }
    if (per_wave && lds4 <= 64 * 1024) {
        const long long per_block = 4 * CAND_PER_WAVE;
        if (bnum && bcov && !getenv("NATAC_CAND_FULL"))   // NATAC_CAND_FULL=1: all four window sums in the kernel (validation)
            hipLaunchKernelGGL((natac_candidates4<true>), dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), lds4, c->stream,
                               ct, vm, d_cc, d_cp, (int)n, nuc_cov, norm, bnum, bcov, lr, var, z);
        else
            hipLaunchKernelGGL((natac_candidates4<false>), dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), lds4, c->stream,
                               ct, vm, d_cc, d_cp, (int)n, nuc_cov, norm, bnum, bcov, lr, var, z);
    } else {   // templates wider than 128 columns or windows too wide for four per wave in LDS: one workgroup per candidate
        hipLaunchKernelGGL(natac_candidates, dim3((unsigned)n), dim3(256), (size_t)(EW + 2) * sizeof(double), c->stream, ct, vm, d_cc,
                           d_cp, nuc_cov, norm, lr, var, z);
    }
}

template <int G>
static void launch_bg(natac_batch *b, const ChunkTable &ct, const VMatDev &vm) {
    natac_ctx *c = b->ctx;
    constexpr int W = 121;
    const int PW = 64 * G + W - 1;
    const int EW = PW + ((vm.upper - 2) >> 1) + ((vm.upper - 1) >> 1);
    const size_t lds = ((size_t)((EW + 1) & ~1) + PW) * sizeof(double);
    hipLaunchKernelGGL((natac_background<G, W>), dim3(b->n_tiles_bg), dim3(64), lds, c->stream, ct, b->d_tiles_bg, vm,
                       b->d_track[NATAC_T_NUC_COV], b->d_track[NATAC_T_RAW], b->d_track[NATAC_T_BACKGROUND],
                       b->d_track[NATAC_T_NORM], b->d_bnum, b->d_bcov);
}

// natac_occ_gsum<STEP, REM> + natac_occ_decide<STEP, RN> for the model's step and window remainder
struct OccFastLaunch { natac_batch *b; const ChunkTable &ct; const OccFastDev &of; size_t lds_gs, lds_od; int rem; bool rn16; };
template <int STEP, int REM = 0>
static void occ_gsum_launch(const OccFastLaunch &f) {
    if constexpr (REM < STEP) {
        if (f.rem == REM)
            hipLaunchKernelGGL((natac_occ_gsum<STEP, REM>), dim3(f.b->n_tiles_gs), dim3(256), f.lds_gs, f.b->ctx->stream, f.ct, f.b->d_tiles_gs, f.of,
                               f.b->d_blk_off, f.b->total_blocks, f.b->d_gsum);
        else
            occ_gsum_launch<STEP, REM + 1>(f);
    }
}
template <int STEP>
static void occ_fast_launch(const OccFastLaunch &f) {
    natac_batch *b = f.b;
    occ_gsum_launch<STEP>(f);
    auto kd = (f.of.flags & 2) ? (f.rn16 ? natac_occ_decide<STEP, 16, true> : natac_occ_decide<STEP, 4, true>)
                               : (f.rn16 ? natac_occ_decide<STEP, 16, false> : natac_occ_decide<STEP, 4, false>);
    const bool heavy_first = b->ctx->occ_ordered;
    hipLaunchKernelGGL(kd, dim3((b->n_tiles_occ + (heavy_first ? HEAVY_CAP : 0) + 3) / 4), dim3(256), f.lds_od, b->ctx->stream, f.ct, b->d_tiles_occ,
                       b->n_tiles_occ, b->d_ranges_occ, heavy_first ? b->d_order_occ : nullptr, f.of, b->d_blk_off, b->total_blocks, b->d_gsum, b->d_grid[0], b->d_grid[1], b->d_grid[2], b->d_defer,
                       b->d_defer + 1);
}

extern "C" {

int natac_abi_version(void) { return NATAC_ABI_VERSION; }
const char *natac_last_error(void) { return g_err.c_str(); }

int natac_device_count(int *count) {
    if (!count) return fail(NATAC_E_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(NATAC_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return NATAC_OK;
}

int natac_ctx_create(int device_id, natac_ctx **out) {
    if (!out) return fail(NATAC_E_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n) return fail(NATAC_E_ARG, "device %d out of range (%d devices)", device_id, n);
    HIPCHK(hipSetDevice(device_id));
    natac_ctx *c = new natac_ctx();
    c->device = device_id;
    HIPCHK(hipGetDeviceProperties(&c->prop, device_id));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    // one stream for both stages.  Measured on MI355X: a second stream for the occ stage does not overlap with the nuc stage on its
    // own (the background kernel's workgroups keep every CU's LDS full); co-scheduling them on purpose (a persistent half-occupancy
    // background launch next to the occupancy kernels, round 4) overlapped exactly as designed and was not faster -- the fp64
    // kernels are clock-limited.  The experiment lives in DESIGN.md section 3.3c and profiles/r4/, not in the library.
    HIPCHK(hipEventCreate(&c->t0));
    HIPCHK(hipEventCreate(&c->t1));
    {   // NATAC_BG_DIRECT=1 selects the direct-summation background kernel (validation / A-B timing of the FFT path)
        const char *e = getenv("NATAC_BG_DIRECT");
        c->bg_direct = e && e[0] == '1';
        e = getenv("NATAC_BG_EXT");
        c->bg_ext = !(e && e[0] == '0');
        e = getenv("NATAC_OCC_GENERAL");   // NATAC_OCC_GENERAL=1: every tile through natac_occ_mle (validation / A-B timing)
        c->occ_force_general = e && e[0] == '1';
        e = getenv("NATAC_OCC_ORDER");     // NATAC_OCC_ORDER=0: natac_occ_decide visits its tiles in chunk order (A-B timing of the ordering)
        c->occ_ordered = !(e && e[0] == '0');
        e = getenv("NATAC_SMOOTH_FUSED");  // NATAC_SMOOTH_FUSED=0: T_SMOOTH is written by natac_run_nuc, never by the peak search (validation / A-B timing)
        c->smooth_fused = !(e && e[0] == '0');
    }
    *out = c;
    return NATAC_OK;
}

void natac_ctx_destroy(natac_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)sync_all(c);
    prof_collect(c);
    if (c->t0) (void)hipEventDestroy(c->t0);
    if (c->t1) (void)hipEventDestroy(c->t1);
    if (c->ck_stream) (void)hipStreamDestroy(c->ck_stream);
    if (c->ck_start) (void)hipEventDestroy(c->ck_start);
    if (c->d_ck) (void)hipFree(c->d_ck);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;      // the pool blocks go back with the members
}

int natac_ctx_sync(natac_ctx *c) {
    if (!c) return fail(NATAC_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    prof_collect(c);
    return NATAC_OK;
}

int natac_ctx_device_info(natac_ctx *c, char *name, size_t name_len, int *n_cu, size_t *mem_bytes) {
    if (!c) return fail(NATAC_E_ARG, "ctx is NULL");
    if (name && name_len) {
        snprintf(name, name_len, "%s (%s)", c->prop.name, c->prop.gcnArchName);
    }
    if (n_cu) *n_cu = c->prop.multiProcessorCount;
    if (mem_bytes) *mem_bytes = c->prop.totalGlobalMem;
    return NATAC_OK;
}

int natac_ctx_device_ids(natac_ctx *c, int *hip_device, char *pci_bus_id, size_t pci_len) {
    if (!c) return fail(NATAC_E_ARG, "ctx is NULL");
    if (hip_device) *hip_device = c->device;
    if (pci_bus_id && pci_len) {
        pci_bus_id[0] = 0;
        HIPCHK(hipDeviceGetPCIBusId(pci_bus_id, (int)pci_len, c->device));
    }
    return NATAC_OK;
}

int natac_set_vmat(natac_ctx *c, const double *mat, int lower, int upper, int w) {
    if (!c || !mat) return fail(NATAC_E_ARG, "null argument");
    if (lower < 0 || upper <= lower || w < 0) return fail(NATAC_E_ARG, "bad vmat geometry lower=%d upper=%d w=%d", lower, upper, w);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    c->vlower = lower; c->vupper = upper; c->vw = w; c->R = upper - lower; c->W = 2 * w + 1;
    int rc = dev_upload(c, c->d_vmat, mat, (size_t)c->R * c->W);
    if (rc) return rc;
    {   // the same rows between VPAD zero columns (natac_frag_gather)
        const int WP = c->W + 2 * VPAD;
        std::vector<double> padded((size_t)c->R * WP, 0.0);
        for (int r = 0; r < c->R; ++r) std::copy(mat + (size_t)r * c->W, mat + (size_t)(r + 1) * c->W, padded.begin() + (size_t)r * WP + VPAD);
        if ((rc = dev_upload(c, c->d_vmat_pad, padded.data(), padded.size()))) return rc;
        HIPCHK(sync_all(c));   // `padded` is a local
    }
    c->vmat_zero = false;
    for (size_t i = 0; i < (size_t)c->R * c->W; ++i) if (mat[i] == 0.0) { c->vmat_zero = true; break; }
    HIPCHK(sync_all(c));
    c->have_vmat = true;
    c->srow_dirty = true;
    c->fft_dirty = true;
    ++c->model_gen;
    return NATAC_OK;
}

int natac_set_sizes(natac_ctx *c, const double *sizes, int upper) {
    if (!c || !sizes || upper <= 0) return fail(NATAC_E_ARG, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    int rc = dev_upload(c, c->d_sizes, sizes, (size_t)upper);
    if (rc) return rc;
    c->h_sizes.assign(sizes, sizes + upper);
    HIPCHK(sync_all(c));
    c->sizes_upper = upper;
    c->have_sizes = true;
    c->srow_dirty = true;
    c->fft_dirty = true;             // the template spectra carry the size weights
    ++c->model_gen;
    return NATAC_OK;
}

int natac_set_occ_model(natac_ctx *c, const double *nuc_probs, const double *nfr_probs, int upper, const double *alphas,
                        int n_alpha, double cutoff, int step, int flank) {
    if (!c || !nuc_probs || !nfr_probs || !alphas) return fail(NATAC_E_ARG, "null argument");
    if (upper < 2 || n_alpha < 1 || n_alpha > 128) return fail(NATAC_E_ARG, "need upper >= 2 and 1 <= n_alpha <= 128");
    if (upper > 256) return fail(NATAC_E_ARG, "occupancy kernel supports upper <= 256 (got %d)", upper);
    if (step < 1 || flank < 0) return fail(NATAC_E_ARG, "bad step/flank");
    if (step % 2 == 0) step -= 1; /* Occupancy.py:190-191 */
    double apos = 1.0;               // smallest positive alpha
    for (int a = 0; a < n_alpha; ++a)
        if (alphas[a] > 0.0 && alphas[a] < apos) apos = alphas[a];
    // a fragment whose size has nfr_prob 0 contributes the factor alpha * probability: natac_occ_mle (which renormalises after every such
    // factor) is exact while that product is >= 2^-1021, so with such a model alphas below 2^-500 are refused (probabilities >= 2^-500 remain)
    if (apos < std::ldexp(1.0, -500))
        for (int j = 0; j < upper; ++j)
            if (nfr_probs[j] == 0.0)
                return fail(NATAC_E_ARG, "occupancy model with a zero nfr probability: the smallest positive alpha must be >= 2^-500 (got %g)", apos);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    c->d_nucp.reset(); c->d_nfrp.reset(); c->d_alphas.reset();
    int rc;
    if ((rc = dev_upload(c, c->d_nucp, nuc_probs, (size_t)upper))) return rc;
    if ((rc = dev_upload(c, c->d_nfrp, nfr_probs, (size_t)upper))) return rc;
    if ((rc = dev_upload(c, c->d_alphas, alphas, (size_t)n_alpha))) return rc;
    HIPCHK(sync_all(c));
    {
        int zf = 0;
        double pmin = 1.0;
        bool odd = false;   // negative / non-finite probabilities: always take the exact per-element path
        for (int j = 0; j < upper; ++j) {
            const double a = nuc_probs[j], f = nfr_probs[j];
            if (a == 0.0) zf |= 1;
            if (f == 0.0) zf |= 2;
            if (a == 0.0 && f == 0.0) zf |= 4;
            if (!(a >= 0.0) || !(f >= 0.0) || std::isinf(a) || std::isinf(f)) odd = true;
            if (a > 0.0 && a < pmin) pmin = a;
            if (f > 0.0 && f < pmin) pmin = f;
        }
        c->occ_zero_flags = zf;
        // p * b >= DBL_MIN needs b >= DBL_MIN / pmin; 2^-1000 leaves room for any positive double pmin >= 2^-22
        c->occ_b_floor = odd ? std::numeric_limits<double>::infinity() : std::ldexp(1.0, -1000) / pmin;
    }
    c->occ_upper = upper; c->n_alpha = n_alpha; c->cutoff = cutoff; c->step = step;
    c->halfstep = (step - 1) / 2; c->flank = flank;
    {   // fast path (natac_occ_fast.hpp): up to 101 increasing alphas in [0, 1], no insert size with probability 0 under both models, an odd
        // step up to 9 (kernel instantiations; the CLI's --step), a window of at least one step (any --flank: a whole number of
        // step-blocks + the first (2 flank + 1) % step bases of the next one), and a probability range that keeps four likelihood
        // factors inside the fp64 range
        c->d_occ_q4.reset(); c->d_occ_rho.reset();
        bool ok = n_alpha <= OD_NA && step <= 9 && 2 * flank + 1 >= step;
        for (int a = 0; ok && a < n_alpha; ++a) ok = alphas[a] >= 0.0 && alphas[a] <= 1.0 && (a == 0 || alphas[a] > alphas[a - 1]);
        double rmin = std::numeric_limits<double>::infinity(), rmax = 0.0, pmin = 1.0;
        bool anynuc = false;
        std::vector<double> rho((size_t)upper, 0.0);
        bool zero_nfr = false;
        for (int j = 0; ok && j < upper; ++j) {
            const double a = nuc_probs[j], f = nfr_probs[j];
            ok = f >= 0.0 && std::isfinite(f) && a >= 0.0 && std::isfinite(a) && (f > 0.0 || a > 0.0);   // 0 under both: natac_occ_mle
            if (!ok) break;
            if (f == 0.0) {       // a fragment of this size can only be nucleosomal: factor alpha (occ_eval, ZF)
                rho[j] = std::numeric_limits<double>::infinity();
                zero_nfr = true;
                anynuc = true;
                pmin = std::min(pmin, a);
                continue;
            }
            rho[j] = a / f;
            ok = std::isfinite(rho[j]);
            if (a > 0.0) { anynuc = true; rmin = std::min(rmin, rho[j]); rmax = std::max(rmax, rho[j]); pmin = std::min(pmin, a); }
            pmin = std::min(pmin, f);
        }
        if (rmax == 0.0) { rmin = 1.0; rmax = 1.0; }      // every nucleosomal size has nfr_prob 0: no finite ratio to bound
        ok = ok && anynuc && rmax <= rmin * std::ldexp(1.0, 200) && pmin >= std::ldexp(1.0, -200);
        // a zero probability excludes alpha = 1 (nuc) or alpha = 0 (nfr) for every window (Occupancy.py:112-114); with an alpha strictly
        // between them the likelihood is positive somewhere, so the all-(-inf) case (the reference raises) cannot reach these kernels
        if ((zero_nfr || (c->occ_zero_flags & 1)) && n_alpha < 3) ok = false;
        // the factor alpha of a zero-nfr size: four of them between two renormalisations (occ_eval, RN = 4) stay normal numbers only for
        // alpha >= 2^-255.  A grid with a smaller positive alpha goes to natac_occ_mle, which renormalises after every factor of such a fragment
        if ((c->occ_zero_flags & 2) && apos < std::ldexp(1.0, -250)) ok = false;
        c->occ_zero_nfr = ok && zero_nfr;
        c->occ_fast_ok = ok;
        // a likelihood factor 1 + alpha (rho kappa - 1) lies in [1 - alpha, 1 + rmax / rmin] with 1 - alpha >= the grid's
        // smallest positive value (or exactly 0 at alpha = 1): 16 of them between two renormalisations stay far inside the
        // fp64 range when rmax / rmin < 2^50 and that smallest step is > 2^-50
        {
            double amin = 1.0;
            for (int a = 0; ok && a < n_alpha; ++a) {
                if (1 - alphas[a] > 0) amin = std::min(amin, 1 - alphas[a]);
                if (zero_nfr && alphas[a] > 0) amin = std::min(amin, alphas[a]);       // the factor alpha of a zero-nfr size
            }
            c->occ_rn16 = ok && rmax <= rmin * std::ldexp(1.0, 50) && amin >= std::ldexp(1.0, -50);
        }
        if (ok) {
            c->occ_nm = (upper + 1) / 2;
            std::vector<double> q4((size_t)4 * c->occ_nm, 0.0);
            for (int j = 0; j < upper; ++j) {
                q4[(size_t)4 * (j >> 1) + (j & 1)] = nuc_probs[j];
                q4[(size_t)4 * (j >> 1) + 2 + (j & 1)] = nfr_probs[j];
            }
            if ((rc = dev_upload(c, c->d_occ_q4, q4.data(), q4.size()))) return rc;
            if ((rc = dev_upload(c, c->d_occ_rho, rho.data(), rho.size()))) return rc;
            HIPCHK(sync_all(c));
        }
    }
    c->have_occ = true;
    return NATAC_OK;
}

int natac_ctx_occ_route(natac_ctx *c, int32_t *fast, int32_t *rn, int32_t *zero_flags) {
    if (!c || !fast || !rn || !zero_flags) return fail(NATAC_E_ARG, "null argument");
    if (!c->have_occ) return fail(NATAC_E_STATE, "natac_set_occ_model has not been called");
    const bool f = c->occ_fast_ok && !c->occ_force_general;
    *fast = f ? 1 : 0;
    *rn = f ? (c->occ_rn16 ? 16 : 4) : 0;
    *zero_flags = (c->occ_zero_flags & 1) | (c->occ_zero_nfr ? 2 : 0);     // OccFastDev::flags of occ_launch
    return NATAC_OK;
}

static int ensure_srow(natac_ctx *c) {
    if (!c->have_vmat) return fail(NATAC_E_STATE, "natac_set_vmat has not been called");
    if (!c->have_sizes) return fail(NATAC_E_STATE, "natac_set_sizes has not been called");
    if (c->sizes_upper < c->vupper) return fail(NATAC_E_ARG, "sizes cover [0,%d) but vmat.upper is %d", c->sizes_upper, c->vupper);
    if (!c->srow_dirty) return NATAC_OK;
    int rc = dev_alloc(c->d_srow, (size_t)c->R);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->d_srow, c->d_sizes + c->vlower, (size_t)c->R * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    c->srow_zero = false;
    for (int r = 0; r < c->R; ++r) if (c->h_sizes[(size_t)c->vlower + r] == 0.0) c->srow_zero = true;
    c->srow_dirty = false;
    return NATAC_OK;
}

// FFT background path applies when the valid part of a 512-point tile is still most of it and the product row has no
// single-cell special case (i == 1, handled by the generic kernel)
static bool fft_bg_applicable(const natac_ctx *c) {
    if (c->bg_direct || c->W > 192 || c->vlower < 2) return false;
    return natac::bg_fft_lds_bytes(c->vupper) <= 64 * 1024;
}

// Extended tiles (natac_fft_bg.hpp): FFT_EXT more outputs on each side of a tile, finished by an edge pass at the end of the tile's wave.  An extended
// tile costs ~10 % more than a plain one (edge pass 6-7 %, its own longer epilogue 3 %: profiles/r5; the rule prices it at 11), so a chunk gets the cheapest
// mix of n tiles of which the first k are extended, 100 n + 11 k smallest with 392 n + 32 k >= L: 2,120 bases take 5 extended tiles
// instead of 6 plain ones, 2,000 bases 5 tiles of which 2 are extended, 10,120 bases stay at 26 plain tiles (25 would need 10 extended
// ones).  The choice depends on the chunk's length alone -- results do not depend on the batch a chunk is in.
static bool bg_ext_possible(const natac_ctx *c) {
    // the edge pass's scratch (partial outputs, reduction scratch, the rows' weights) lives in the transposes' LDS region
    return c->bg_ext && c->W >= 2 * natac::FFT_EXT &&
           4 * natac::FFT_EXT + natac::EDGE_SCRATCH + 4 * ((c->R + 3) / 4) <= 2 * natac::FFT_LA;
}
static void bg_chunk_tiling(int L, int TV, bool ext_ok, int *n_tiles, int *n_extended) {
    const int E2 = 2 * natac::FFT_EXT;
    const int n_std = (L + TV - 1) / TV;
    int best_n = n_std, best_k = 0;
    long long best = 100LL * n_std;
    for (int n = n_std - 1; ext_ok && n >= 1 && (long long)n * (TV + E2) >= L; --n) {
        const int k = (int)((L - (long long)n * TV + E2 - 1) / E2);
        const long long cost = 100LL * n + 11LL * k;
        if (cost < best) { best = cost; best_n = n; best_k = k; }
    }
    *n_tiles = best_n;
    *n_extended = best_k;
}
int natac_bg_tiling(natac_ctx *c, int32_t chunk_len, int32_t *n_tiles, int32_t *extended) {
    if (!c || chunk_len <= 0) return fail(NATAC_E_ARG, "natac_bg_tiling: context and a positive chunk length");
    if (!c->d_vmat) return fail(NATAC_E_STATE, "natac_bg_tiling: set the V-plot first");
    int nt = 0, ex = 0;
    if (fft_bg_applicable(c)) bg_chunk_tiling(chunk_len, natac::FFT_N - c->W + 1, bg_ext_possible(c), &nt, &ex);
    if (n_tiles) *n_tiles = nt;
    if (extended) *extended = ex;
    return NATAC_OK;
}

static int build_tiles_bg(natac_batch *b, int TV, bool ext_ok) {
    std::vector<int2> tiles;
    tiles.reserve((size_t)(b->total_bp / TV) + b->nc);
    const int TVX = TV + 2 * natac::FFT_EXT;
    for (int i = 0; i < b->nc; ++i) {
        int nt, k;
        bg_chunk_tiling(b->h_len[i], TV, ext_ok, &nt, &k);
        int x = 0;
        for (int t = 0; t < nt; ++t) {
            if (t < k) {       // outputs [x, x + TVX): the transform's exact ones start at x + FFT_EXT
                tiles.push_back(make_int2(i, (x + natac::FFT_EXT) | natac::FFT_EXT_BIT));
                x += TVX;
            } else {
                tiles.push_back(make_int2(i, x));
                x += TV;
            }
        }
    }
    b->n_tiles_bg = (int)tiles.size();
    int rc = dev_upload(b->ctx, b->d_tiles_bg, tiles.data(), tiles.size());
    if (rc) return rc;
    HIPCHK(sync_all(b->ctx));  // `tiles` is a local
    return NATAC_OK;
}

static int ensure_fft(natac_ctx *c) {
    int rc;
    if (!c->d_fft_tw) {
        std::vector<double> tw(2 * (size_t)natac::FFT_N);
        for (int k = 0; k < natac::FFT_N; ++k) {
            const double a = 2.0 * M_PI * k / natac::FFT_N;
            tw[2 * k] = std::cos(a);
            tw[2 * k + 1] = -std::sin(a);
        }
        // fault injection for the test suite's own sensitivity check (tests/test_gpu_tight_tier.py): NATAC_FAULT_TWIDDLE="k:delta" adds delta
        // to cos(2 pi k / 512).  The parity tests must FAIL with k = 37, delta = 1e-9 -- a tolerance that lets this through is not a test.
        if (const char *e = getenv("NATAC_FAULT_TWIDDLE")) {
            int k = 0; double dlt = 0.0;
            if (sscanf(e, "%d:%lf", &k, &dlt) == 2 && k >= 0 && k < natac::FFT_N) tw[2 * (size_t)k] += dlt;
        }
        if ((rc = dev_upload(c, c->d_fft_tw, tw.data(), tw.size()))) return rc;
        HIPCHK(sync_all(c));
    }
    if (!c->fft_dirty) return NATAC_OK;
    HIPCHK(sync_all(c));
    const int npair = (c->R + 1) / 2;
    if ((rc = dev_alloc(c->d_fft_k, (size_t)npair * 2 * natac::FFT_N))) return rc;
    hipLaunchKernelGGL(natac_fft_template, dim3(npair), dim3(64), 0, c->stream, c->d_vmat, c->d_srow, c->R, c->W, c->d_fft_tw, c->d_fft_k);
    if (c->W >= natac::FFT_EXT) {
        c->d_fft_mtab.reset(); c->d_fft_swt.reset();
        const int NJ = (c->R + 3) / 4;
        if ((rc = dev_alloc(c->d_fft_mtab, (size_t)2 * NJ * 64)) || (rc = dev_alloc(c->d_fft_swt, (size_t)4 * NJ))) return rc;
        hipLaunchKernelGGL(natac_fft_edge_table_mfma, dim3((2 * NJ * 64 + 255) / 256), dim3(256), 0, c->stream, c->d_vmat, c->d_srow, c->R, c->W, NJ,
                           c->d_fft_mtab, c->d_fft_swt);
    }
    HIPCHK(hipGetLastError());
    c->fft_dirty = false;
    return NATAC_OK;
}

static int ensure_window(natac_ctx *c, PoolBuf<double> &slot, int *slotM, double *slotsd, int M, double sd, double *slotsum = nullptr) {
    if (slot && *slotM == M && *slotsd == sd) return NATAC_OK;
    HIPCHK(sync_all(c));
    // scipy.signal.gaussian(M, sd): exp(-0.5 (n/sd)^2), n = arange(M) - (M-1)/2   (pyatac/utils.py:40)
    std::vector<double> w((size_t)3 * M);
    for (int i = 0; i < M; ++i) {
        double n = (double)i - (M - 1) / 2.0;
        double q = n / sd;
        w[i] = std::exp(-0.5 * (q * q));
    }
    // behind the window, the denominators of a base next to a chunk end, in the kernels' order (acc = fma(w, 1, acc) from 0):
    // w[M + m] = w[0] + .. + w[m] (the taps left when the window hangs over the chunk's start), w[2 M + k] = w[k] + .. + w[M - 1] (its end)
    for (int m = 0; m < M; ++m) w[M + m] = (m ? w[M + m - 1] : 0.0) + w[m];
    for (int k = 0; k < M; ++k) {
        double acc = 0.0;
        for (int i = k; i < M; ++i) acc = acc + w[i];
        w[2 * M + k] = acc;
    }
    int rc = dev_upload(c, slot, w.data(), (size_t)3 * M);
    if (rc) return rc;
    HIPCHK(sync_all(c));
    if (slotsum) {
        double acc = 0.0;
        for (int i = 0; i < M; ++i) acc = acc + w[i];     // same order as the kernel's fma(w, 1, den) chain
        *slotsum = acc;
    }
    *slotM = M;
    *slotsd = sd;
    return NATAC_OK;
}

// E = exp(bias) of the batch on `st`: part of the work of the stage that needs it.  natac_run_nuc always computes it;
// natac_run_occ reuses the array natac_run_nuc left since the last natac_run_occ (once per nuc + occ pass), else computes it.
static int run_exp_bias(natac_batch *b, hipStream_t st, bool from_occ) {
    if (!b->d_bias) return NATAC_OK;
    if (from_occ && b->ebias_fresh) { b->ebias_fresh = false; return NATAC_OK; }
    b->ebias_fresh = !from_occ;
    int rc;
    if (!b->d_ebias && (rc = dev_alloc(b->d_ebias, (size_t)b->nb))) return rc;
    const int blocks = (int)std::min<long long>((b->nb + 255) / 256, 16384);
    hipLaunchKernelGGL(natac_exp_bias, dim3(blocks), dim3(256), 0, st, b->d_bias, b->d_ebias, b->nb);
    return NATAC_OK;
}

static ChunkTable make_table(natac_batch *b) {
    ChunkTable t;
    t.nc = b->nc; t.chunk_len = b->d_len; t.frag_off = b->d_frag_off; t.lpos = b->d_lpos; t.ilen = b->d_ilen;
    t.centre = b->d_centre; t.bias_off = b->d_bias_off; t.bias = b->d_bias; t.ebias = b->d_ebias; t.bias_left = b->bias_left;
    t.bias_right = b->bias_right; t.out_off = b->d_out_off; t.grid_off = b->d_grid_off;
    return t;
}
static VMatDev make_vmat(natac_ctx *c) {
    VMatDev v;
    v.mat = c->d_vmat; v.matp = c->d_vmat_pad; v.srow = c->d_srow; v.lower = c->vlower; v.upper = c->vupper; v.w = c->vw; v.R = c->R; v.W = c->W;
    v.has_zero = (c->vmat_zero || c->srow_zero) ? 1 : 0;
    v.lrt = nullptr;
    v.ctab = nullptr;
    return v;
}
static OccModelDev make_occ(natac_ctx *c) {
    OccModelDev o;
    o.nuc_probs = c->d_nucp; o.nfr_probs = c->d_nfrp; o.alphas = c->d_alphas; o.upper = c->occ_upper;
    o.n_alpha = c->n_alpha; o.step = c->step; o.halfstep = c->halfstep; o.flank = c->flank; o.cutoff = c->cutoff;
    o.ci_factor = std::exp(-0.5 * c->cutoff);
    o.zero_flags = c->occ_zero_flags;
    o.b_floor = c->occ_b_floor;
    return o;
}

static int build_tiles(natac_batch *b, int width, PoolBuf<int2> &d_out, int *n_out, bool grid_units = false, int step = 1, int half = 0) {
    std::vector<int2> tiles;
    tiles.reserve((size_t)(b->total_bp / std::max(1, width)) + b->nc);
    for (int i = 0; i < b->nc; ++i) {
        int n = b->h_len[i];
        if (grid_units) n = (b->h_len[i] > half) ? (b->h_len[i] - half + step - 1) / step : 0;
        for (int x = 0; x < n; x += width) tiles.push_back(make_int2(i, x));
    }
    *n_out = (int)tiles.size();
    int rc = dev_upload(b->ctx, d_out, tiles.data(), tiles.size());
    if (rc) return rc;
    HIPCHK(sync_all(b->ctx));  // `tiles` is a local
    return NATAC_OK;
}

int natac_batch_create(natac_ctx *c, int32_t nc, const int32_t *chunk_len, const int64_t *frag_off, const int32_t *frag_lpos,
                       const int32_t *frag_ilen, const int64_t *bias_off, const double *bias_log, int32_t bias_left,
                       int32_t bias_right, natac_batch **out) {
    if (!c || !out || !chunk_len || !frag_off) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    if (nc <= 0) return fail(NATAC_E_ARG, "n_chunks must be positive");
    if (bias_log && !bias_off) return fail(NATAC_E_ARG, "bias_log without bias_off");
    if (frag_off[0] != 0) return fail(NATAC_E_ARG, "frag_off[0] must be 0");
    const long long nf = frag_off[nc];
    if (nf > 0 && (!frag_lpos || !frag_ilen)) return fail(NATAC_E_ARG, "fragment arrays are NULL");
    HIPCHK(hipSetDevice(c->device));
    natac_batch *b = new natac_batch();
    b->ctx = c; b->nc = nc; b->nf = nf; b->bias_left = bias_left; b->bias_right = bias_right;
    b->h_len.assign(chunk_len, chunk_len + nc);
    b->h_out_off.resize((size_t)nc + 1);
    b->h_out_off[0] = 0;
    for (int i = 0; i < nc; ++i) {
        if (chunk_len[i] <= 0) { delete b; return fail(NATAC_E_ARG, "chunk %d has length %d", i, chunk_len[i]); }
        if (frag_off[i + 1] < frag_off[i] || frag_off[i + 1] - frag_off[i] > 0x7fffffffLL) {
            delete b; return fail(NATAC_E_ARG, "frag_off not monotone (chunk %d)", i);
        }
        if (bias_off && bias_off[i + 1] - bias_off[i] != (long long)chunk_len[i] + bias_left + bias_right) {
            delete b; return fail(NATAC_E_ARG, "bias slice of chunk %d must cover [start-%d, end+%d)", i, bias_left, bias_right);
        }
        b->h_out_off[i + 1] = b->h_out_off[i] + chunk_len[i];
        b->max_len = std::max(b->max_len, chunk_len[i]);
    }
    b->total_bp = b->h_out_off[nc];
    b->nb = bias_off ? bias_off[nc] : 0;
    // what fails after an upload was queued leaves the cleanup to natac_batch_free: it drains the stream before the blocks go back
    auto upload = [&]() -> int {
        int rc;
        if ((rc = dev_upload(c, b->d_len, chunk_len, (size_t)nc)) ||
            (rc = dev_upload(c, b->d_frag_off, (const long long *)frag_off, (size_t)nc + 1)) ||
            (rc = dev_upload(c, b->d_lpos, frag_lpos, (size_t)nf)) || (rc = dev_upload(c, b->d_ilen, frag_ilen, (size_t)nf)) ||
            (rc = dev_alloc(b->d_centre, (size_t)nf)) || (rc = dev_upload(c, b->d_out_off, b->h_out_off.data(), (size_t)nc + 1)))
            return rc;
        if (bias_off) {
            if ((rc = dev_upload(c, b->d_bias_off, (const long long *)bias_off, (size_t)nc + 1))) return rc;
            if (bias_log) rc = dev_upload(c, b->d_bias, bias_log, (size_t)b->nb);
            else rc = dev_alloc(b->d_bias, (size_t)b->nb);           // filled on the device (natac_batch_create_from_seq)
            if (rc) return rc;
        }
        if ((rc = dev_alloc(b->d_status, (size_t)nc))) return rc;
        hipError_t e = hipMemsetAsync(b->d_status, 0, (size_t)nc * sizeof(int), c->stream);
        if (e != hipSuccess) return fail(NATAC_E_HIP, "memset: %s", hipGetErrorString(e));
        if (nf > 0) {
            int blocks = (int)std::min<long long>((nf + 255) / 256, 4096);
            hipLaunchKernelGGL(natac_frag_centres, dim3(blocks), dim3(256), 0, c->stream, b->d_lpos, b->d_ilen, b->d_centre, nf);
        }
        if ((rc = build_tiles(b, 256, b->d_tiles256, &b->n_tiles256))) return rc;
        {
            std::vector<long long> first((size_t)nc + 1, 0);
            for (int i = 0; i < nc; ++i) first[(size_t)i + 1] = first[i] + (chunk_len[i] + 255) / 256;
            if ((rc = dev_upload(c, b->d_tile256_first, first.data(), first.size()))) return rc;
        }
        e = hipStreamSynchronize(c->stream);  // host buffers may be released by the caller after return
        if (e != hipSuccess) return fail(NATAC_E_HIP, "upload: %s", hipGetErrorString(e));
        return NATAC_OK;
    };
    if (int rc = upload()) {
        natac_batch_free(b);
        return rc;
    }
    *out = b;
    return NATAC_OK;
}

int natac_batch_create_from_seq(natac_ctx *c, int32_t nc, const int32_t *chunk_len, const int64_t *frag_off, const int32_t *frag_lpos,
                                const int32_t *frag_ilen, const int64_t *seq_off, const uint8_t *seq, const double *log_pwm,
                                const uint8_t *nucleotides, int nrow, int K, int32_t bias_left, int32_t bias_right, natac_batch **out) {
    if (!c || !out || !chunk_len || !seq_off || !seq || !log_pwm || !nucleotides) return fail(NATAC_E_ARG, "null argument");
    if (nc <= 0 || nrow < 1 || K < 1) return fail(NATAC_E_ARG, "bad argument");
    std::vector<int64_t> boff((size_t)nc + 1, 0);
    for (int i = 0; i < nc; ++i) {
        const int64_t nb = (int64_t)chunk_len[i] + bias_left + bias_right;
        if (seq_off[i + 1] - seq_off[i] != nb + K - 1)
            return fail(NATAC_E_ARG, "sequence window of chunk %d must hold %lld bases ([start-%d-up, end+%d+down))", i, (long long)(nb + K - 1),
                        bias_left, bias_right);
        boff[(size_t)i + 1] = boff[(size_t)i] + nb;
    }
    int rc = natac_batch_create(c, nc, chunk_len, frag_off, frag_lpos, frag_ilen, boff.data(), nullptr, bias_left, bias_right, out);
    if (rc) return rc;
    natac_batch *b = *out;
    DeviceCall dc(c, "pwm score");
    const unsigned char *d_s = dc.upload((const unsigned char *)seq, (size_t)seq_off[nc]);
    const long long *d_so = dc.upload((const long long *)seq_off, (size_t)nc + 1);
    const unsigned char *d_n = dc.upload((const unsigned char *)nucleotides, (size_t)nrow);
    const double *d_p = dc.upload(log_pwm, (size_t)nrow * K);
    if (dc.ok()) {
        const int maxlen = b->max_len + bias_left + bias_right;
        const unsigned gx = (unsigned)std::min(16, (maxlen + 1023) / 1024);
        hipLaunchKernelGGL(natac_pwm_score_chunks, dim3(gx, (unsigned)nc), dim3(256), 0, c->stream, d_s, d_so, b->d_bias_off, d_p, d_n, nrow, K,
                           b->d_bias);
        dc.launched();
    }
    if ((rc = dc.finish())) { natac_batch_free(b); *out = nullptr; }
    return rc;
}

void natac_batch_free(natac_batch *b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    (void)sync_all(b->ctx);
    prof_collect(b->ctx);
    (void)fmt_pending_wait(b);
    delete b;      // the pool blocks go back with the members
}

int natac_batch_release_outputs(natac_batch *b) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    prof_collect(c);
    for (auto &t : b->d_track) t.reset();
    for (auto &g : b->d_grid) g.reset();
    b->d_bnum.reset(); b->d_bcov.reset(); b->d_gsum.reset(); b->d_pk_out.reset();
    b->d_pk_chunk.reset(); b->d_pk_pos.reset(); b->d_opk_vals.reset(); b->d_opk_keep.reset(); b->d_nuc_dist.reset();
    b->d_fmt_out.reset(); b->fmt_bytes = -1;
    (void)fmt_pending_wait(b);
    b->pk_cap = 0; b->pk_n = -1; b->opk_cap = 0; b->opk_n = -1;
    b->out = BatchOutputs();
    // the per-chunk status words describe the outputs that were just dropped
    HIPCHK(hipMemsetAsync(b->d_status, 0, (size_t)b->nc * sizeof(int), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return NATAC_OK;     // offset / tile tables stay: the next natac_run_* only re-allocates the arrays
}

int natac_batch_info(natac_batch *b, int64_t *total_bp, int64_t *total_grid, int64_t *n_frags) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    if (total_bp) *total_bp = b->total_bp;
    if (total_grid) *total_grid = b->total_grid;
    if (n_frags) *n_frags = b->nf;
    return NATAC_OK;
}

static int ensure_track(natac_batch *b, int t) {
    if (b->d_track[t]) return NATAC_OK;
    return dev_alloc(b->d_track[t], (size_t)b->total_bp);  // INS uses the first half of a double slot (int32)
}

// SMOOTH = the clamped NaN-aware Gaussian of NORM, window c->d_win_nuc (M values); the caller has built d_tiles1k for M = 61
static void launch_nuc_smooth(natac_batch *b, const ChunkTable &ct, int M) {
    natac_ctx *c = b->ctx;
    const int h = (M - 1) / 2;
    if (h == 30) {      // the cli's smooth_sd = 10: four bases per lane
        hipLaunchKernelGGL((natac_smooth_same4<true, 30>), dim3(b->n_tiles1k), dim3(256), (size_t)8 * SM4_S(30) * sizeof(double),
                           c->stream, ct, b->d_tiles1k, c->d_win_nuc, c->win_nuc_sum, b->d_track[NATAC_T_NORM],
                           b->d_track[NATAC_T_SMOOTH]);
    } else {
        const size_t lds = ((size_t)2 * (256 + 2 * h)) * sizeof(double);
        hipLaunchKernelGGL((natac_smooth_same<true>), dim3(b->n_tiles256), dim3(256), lds, c->stream, ct, b->d_tiles256,
                           c->d_win_nuc, M, c->win_nuc_sum, b->d_track[NATAC_T_NORM], b->d_track[NATAC_T_SMOOTH]);
    }
}

// the peak search can form SMOOTH itself for some `order`: order 1 keeps the longest lists, so if any order's arm can, its arm can
static bool peaks_can_smooth(const natac_batch *b, int M) {
    return b->ctx->smooth_fused && (M - 1) / 2 == PK_SM_H && peaks_plan(b->max_len, 1).forms_smooth;
}

int natac_run_nuc(natac_batch *b, double smooth_sd) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_srow(c);
    if (rc) return rc;
    if (!(smooth_sd > 0)) return fail(NATAC_E_ARG, "smooth_sd must be positive");
    const int M = 6 * (int)smooth_sd + 1;  /* NucleosomeCalling.py:276 (integer sd from the cli) */
    const int need_l = c->vw + ((c->vupper - 2) >> 1), need_r = c->vw + ((c->vupper - 1) >> 1) + 1;
    if (b->d_bias && (b->bias_left < need_l || b->bias_right < need_r))
        return fail(NATAC_E_ARG, "bias track must extend >= %d left / %d right of the chunk (has %d / %d)", need_l, need_r,
                    b->bias_left, b->bias_right);
    for (int i = 0; i < b->nc; ++i)
        if (b->h_len[i] < M) return fail(NATAC_E_ARG, "chunk %d shorter (%d) than the smoothing window (%d)", i, b->h_len[i], M);
    if ((rc = ensure_window(c, c->d_win_nuc, &c->win_nuc_M, &c->win_nuc_sd, M, smooth_sd, &c->win_nuc_sum))) return rc;
    const bool use_fft = fft_bg_applicable(c);
    // The background track itself is an output only with --write_all (run_nuc.py:22-39: _nucHelper returns it, run_nuc writes it only
    // then); the FFT kernel leaves its two factors per base (bnum, bcov: the candidates read them) and T_BACKGROUND is formed from them
    // on the first request (materialise_bg) -- the same expression, the same bits, 8 bytes per base less written per step.
    for (int t : {NATAC_T_NUC_COV, NATAC_T_NFR_COV, NATAC_T_RAW, NATAC_T_NORM, NATAC_T_SMOOTH})
        if ((rc = ensure_track(b, t))) return rc;
    if (!use_fft && (rc = ensure_track(b, NATAC_T_BACKGROUND))) return rc;
    if (!b->d_bnum && (rc = dev_alloc(b->d_bnum, (size_t)b->total_bp))) return rc;
    if (!b->d_bcov && (rc = dev_alloc(b->d_bcov, (size_t)b->total_bp))) return rc;
    const bool fast = !use_fft && (c->W == 121 && c->vlower >= 2);
    if (use_fft) {
        if ((rc = ensure_fft(c))) return rc;
        const int TV = FFT_N - c->W + 1;
        const bool ext_ok = bg_ext_possible(c);
        const int key = -(TV + (ext_ok ? 4096 : 0));   // the tiling this batch's table was built for
        if (b->bgG != key) {
            if ((rc = build_tiles_bg(b, TV, ext_ok))) return rc;
            b->bgG = key;
        }
    } else if (fast) {
        const int G = choose_bg_G(b, c->W);
        if (G != b->bgG) {
            if ((rc = build_tiles(b, 64 * G, b->d_tiles_bg, &b->n_tiles_bg))) return rc;
            b->bgG = G;
        }
    }
    if (!b->d_ebias && b->d_bias && (rc = dev_alloc(b->d_ebias, (size_t)b->nb))) return rc;
    const ChunkTable ct = make_table(b);
    const VMatDev vm = make_vmat(c);
    natac_ctx::Ev ev;
    if (!b->d_ranges256 && (rc = dev_alloc(b->d_ranges256, (size_t)b->n_tiles256))) return rc;
    // the default pass reads SMOOTH in the peak search first, and that can form it from the chunk it holds: left pending then
    const bool smooth_later = peaks_can_smooth(b, M);
    if (!smooth_later && (M - 1) / 2 == 30 && !b->d_tiles1k && (rc = build_tiles(b, 1024, b->d_tiles1k, &b->n_tiles1k))) return rc;
    prof_begin(c, NATAC_K_FRAG_GATHER, ev);
    if (b->ranges256_w != c->vw) {
        hipLaunchKernelGGL(natac_tile_ranges256, dim3((b->n_tiles256 + 255) / 256), dim3(256), 0, c->stream, ct, b->d_tiles256,
                           b->n_tiles256, c->vw, b->d_ranges256);
        b->ranges256_w = c->vw;
    }
    // OccChunk.getCov = nuc_cov + nfr_cov when the occupancy model's window / size range are the V-plot's: written here too
    // -- unless OCC_COV holds what another writer left (natac_run_occ under another window, natac_batch_set_track) or what this stage
    // wrote for another window or size range: that stays readable as it is, and the next natac_run_occ forms the sum itself
    const bool cov_mine = b->out.occ_cov_by_nuc && b->out.nuc_w == c->vw && b->out.nuc_upper == c->vupper;
    const bool cov_too = c->have_occ && c->flank == c->vw && c->occ_upper == c->vupper &&
                         (b->out.track[NATAC_T_OCC_COV] == TS_EMPTY || cov_mine);
    if (cov_too && (rc = ensure_track(b, NATAC_T_OCC_COV))) return rc;
    constexpr int GNBL = NATAC_GNBL;      // adjacent bases per lane: 2.  Round 5, lanes outside a window reading one shared zero line:
                                          // 0.63 ms per 20 k chunks against 0.79 with 4 and 0.85 with 1 (round 2: 3.5 / 4.5 / 3.8 ms per step)
    hipLaunchKernelGGL((natac_frag_gather<GNBL>), dim3(b->n_tiles256), dim3(256 / GNBL), 0, c->stream, ct, b->d_tiles256, b->d_ranges256, vm,
                       b->d_track[NATAC_T_NUC_COV], b->d_track[NATAC_T_NFR_COV], b->d_track[NATAC_T_RAW],
                       cov_too ? b->d_track[NATAC_T_OCC_COV] : nullptr);
    prof_end(c, ev);
    prof_begin(c, NATAC_K_BACKGROUND, ev);
    if ((rc = run_exp_bias(b, c->stream, false))) return rc;
    if (use_fft) {
        const size_t lds = bg_fft_lds_bytes(vm.upper);
        hipLaunchKernelGGL(natac_background_fft, dim3(b->n_tiles_bg), dim3(64), lds, c->stream, ct, b->d_tiles_bg, vm, c->d_fft_tw,
                           c->d_fft_k, b->d_track[NATAC_T_NUC_COV], b->d_track[NATAC_T_RAW], (double *)nullptr,
                           b->d_track[NATAC_T_NORM], b->d_bnum, b->d_bcov, (unsigned)b->n_tiles_bg, c->d_fft_mtab,
                           c->d_fft_swt, (c->R + 3) / 4);
    } else if (fast) {
        switch (b->bgG) {
            case 7: launch_bg<7>(b, ct, vm); break;
            case 9: launch_bg<9>(b, ct, vm); break;
            case 13: launch_bg<13>(b, ct, vm); break;
            default: launch_bg<17>(b, ct, vm); break;
        }
    } else {
        hipLaunchKernelGGL(natac_background_generic, dim3(b->n_tiles256), dim3(256), 0, c->stream, ct, b->d_tiles256, vm,
                           b->d_track[NATAC_T_NUC_COV], b->d_track[NATAC_T_RAW], b->d_track[NATAC_T_BACKGROUND],
                           b->d_track[NATAC_T_NORM], b->d_bnum, b->d_bcov);
    }
    prof_end(c, ev);
    if (!smooth_later) {
        prof_begin(c, NATAC_K_SMOOTH_NUC, ev);
        launch_nuc_smooth(b, ct, M);
        prof_end(c, ev);
    }
    HIPCHK(hipGetLastError());
    for (int t : {NATAC_T_NUC_COV, NATAC_T_NFR_COV, NATAC_T_RAW, NATAC_T_NORM, NATAC_T_SMOOTH}) b->out.track[t] = TS_RUN;
    if (smooth_later) b->out.track[NATAC_T_SMOOTH] = TS_PENDING;
    b->out.smooth_M = M;
    b->out.smooth_sd = smooth_sd;
    b->out.track[NATAC_T_BACKGROUND] = use_fft ? TS_PENDING : TS_RUN;
    b->out.bg_gen = c->model_gen;
    b->out.nuc_w = c->vw;
    b->out.nuc_lower = c->vlower;
    b->out.nuc_upper = c->vupper;
    b->out.occ_cov_by_nuc = cov_too;     // OCC_COV itself becomes readable through natac_run_occ only
    return NATAC_OK;
}

// natac_occ_smooth (one base per lane, any step / window): smoothed occupancy -> dst_occ (un-filled), bounds -> dst_lo / dst_hi (or null)
static void launch_occ_smooth_generic(natac_batch *b, const ChunkTable &ct, const OccModelDev &om, int M, double *dst_occ, double *dst_lo,
                                      double *dst_hi) {
    natac_ctx *c = b->ctx;
    const int h = (M - 1) / 2;
    const int NB = 2 * ((h + c->step - 1) / c->step) + 2, NG = (255 + 2 * h) / c->step + 3;
    const size_t lds = ((size_t)((M + 1) & ~1) + (size_t)c->step * NB + 3 * (size_t)NG) * sizeof(double);
    hipLaunchKernelGGL(natac_occ_smooth, dim3(b->n_tiles256), dim3(256), lds, c->stream, ct, b->d_tiles256, om, c->d_win_occ, M,
                       b->d_grid[0], b->d_grid[1], b->d_grid[2], dst_occ, dst_lo, dst_hi);
}

// blocks the STEP bases of a step-block see in natac_occ_smooth_blk: ceil(h / step) to the left + their own + (h + step - 1) / step to
// the right; for h a multiple of the step that is 2 h / step + 1, launched with the spare (zero-weight) block round 2 measured with
static int occ_smooth_blocks(int h, int step) {
    if (h % step == 0) return 2 * (h / step) + 2;
    return (h + step - 1) / step + (h + step - 1) / step + 1;
}

// block weights of natac_occ_smooth_blk: wb[bi][j] = sum of the window taps that fall on block bmin + bi for a base at offset j
// of its block -- the table natac_occ_smooth forms per workgroup, same summation order
static int ensure_block_weights(natac_ctx *c, int M, double sd, int NB) {
    if (c->d_wb_occ && c->wb_M == M && c->wb_step == c->step) return NATAC_OK;
    HIPCHK(sync_all(c));
    const int h = (M - 1) / 2, step = c->step;
    std::vector<double> w((size_t)M), wb((size_t)step * NB + step);     // + the full denominators wb[NB][j] of the clean sweep
    for (int i = 0; i < M; ++i) {           // as ensure_window
        const double n = (double)i - (M - 1) / 2.0, q = n / sd;
        w[i] = std::exp(-0.5 * (q * q));
    }
    for (int j = 0; j < step; ++j)
        for (int bi = 0; bi < NB; ++bi) {
            const int bmin = -((h + step - 1) / step);    // leftmost block any base of a block reaches
            double sacc = 0.0;
            for (int d = 0; d < step; ++d) {
                const int n = j + h - (bmin + bi) * step - d;
                if (n >= 0 && n < M) sacc += w[n];
            }
            wb[(size_t)bi * step + j] = sacc;
        }
    for (int j = 0; j < step; ++j) {        // den[j] of a base with every block present: the kernel's own sequence fma(w, 1, den)
        double den = 0.0;
        for (int bi = 0; bi < NB; ++bi) den = std::fma(wb[(size_t)bi * step + j], 1.0, den);
        wb[(size_t)NB * step + j] = den;
    }
    int rc = dev_upload(c, c->d_wb_occ, wb.data(), wb.size());
    if (rc) return rc;
    HIPCHK(sync_all(c));
    c->wb_M = M;
    c->wb_step = step;
    return NATAC_OK;
}

// BACKGROUND after the FFT kernel: (bnum * nuc_cov) / bcov per base, the expression of the kernel's own epilogue (natac_fft_bg.hpp)
static int materialise_bg(natac_batch *b) {
    natac_ctx *c = b->ctx;
    int rc = ensure_track(b, NATAC_T_BACKGROUND);
    if (rc) return rc;
    const int blocks = (int)std::min<long long>((b->total_bp + 255) / 256, 1 << 20);
    hipLaunchKernelGGL(natac_bg_from_factors, dim3(blocks), dim3(256), 0, c->stream, b->d_bnum, b->d_track[NATAC_T_NUC_COV], b->d_bcov,
                       b->d_track[NATAC_T_BACKGROUND], b->total_bp);
    HIPCHK(hipGetLastError());
    b->out.track[NATAC_T_BACKGROUND] = TS_RUN;
    return NATAC_OK;
}

// OCC_PREFILL (smoothed_vals before call_peaks' NaN fill) is not part of the default pass: written on the first request
static int materialise_prefill(natac_batch *b) {
    natac_ctx *c = b->ctx;
    int rc = ensure_track(b, NATAC_T_OCC_PREFILL);
    if (rc) return rc;
    // the context's step, halfstep and flank are the run's (need_track); its window may be another batch's by now
    if ((rc = ensure_window(c, c->d_win_occ, &c->win_occ_M, &c->win_occ_sd, 2 * c->flank + 1, c->flank / 3.0))) return rc;
    const ChunkTable ct = make_table(b);
    const OccModelDev om = make_occ(c);
    launch_occ_smooth_generic(b, ct, om, 2 * c->flank + 1, b->d_track[NATAC_T_OCC_PREFILL], nullptr, nullptr);
    HIPCHK(hipGetLastError());
    b->out.track[NATAC_T_OCC_PREFILL] = TS_RUN;
    return NATAC_OK;
}

// SMOOTH that natac_run_nuc left to the peak search and another reader asks for first (a download, a writer, a peak search
// the fused kernel does not cover, natac_batch_set_track about to replace NORM): the smoothing kernels natac_run_nuc would have run
static int materialise_smooth(natac_batch *b) {
    natac_ctx *c = b->ctx;
    int rc;
    // the window natac_run_nuc was asked for; the context's may be another batch's by now
    if ((rc = ensure_window(c, c->d_win_nuc, &c->win_nuc_M, &c->win_nuc_sd, b->out.smooth_M, b->out.smooth_sd, &c->win_nuc_sum))) return rc;
    if ((b->out.smooth_M - 1) / 2 == 30 && !b->d_tiles1k && (rc = build_tiles(b, 1024, b->d_tiles1k, &b->n_tiles1k))) return rc;
    const ChunkTable ct = make_table(b);
    natac_ctx::Ev ev;
    prof_begin(c, NATAC_K_SMOOTH_NUC, ev);
    launch_nuc_smooth(b, ct, b->out.smooth_M);
    prof_end(c, ev);
    HIPCHK(hipGetLastError());
    b->out.track[NATAC_T_SMOOTH] = TS_RUN;
    return NATAC_OK;
}

// Every read of an output track goes through here: NATAC_E_STATE (before any HIP call) if it holds nothing, formed if pending.
static int need_track(natac_batch *b, int t) {
    static const char *const names[NATAC_T_COUNT] = {"NUC_COV", "NFR_COV", "RAW", "BACKGROUND", "NORM", "SMOOTH", "OCC", "OCC_LOWER",
                                                     "OCC_UPPER", "OCC_COV", "INS", "OCC_PREFILL", "INS_SMOOTH", "CENTER_COV", "BIAS"};
    if (t < 0 || t >= NATAC_T_COUNT) return fail(NATAC_E_ARG, "bad track id %d", t);
    if (b->out.track[t] == TS_EMPTY)
        return fail(NATAC_E_STATE, "track NATAC_T_%s holds nothing: no stage has written it and natac_batch_set_track has not", names[t]);
    if (b->out.track[t] != TS_PENDING) return NATAC_OK;
    if (t == NATAC_T_OCC_PREFILL) {      // formed from the grids with the context's step and window: they must be the run's
        const int rc = need_occ_geometry(b, "NATAC_T_OCC_PREFILL");
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(b->ctx->device));
    if (t == NATAC_T_SMOOTH) return materialise_smooth(b);
    return t == NATAC_T_BACKGROUND ? materialise_bg(b) : materialise_prefill(b);
}

// natac_run_occ, part 1: every allocation, table upload and host synchronisation of the stage (nothing is launched that
// depends on another stream), so that part 2 can be enqueued behind a running kernel without stalling the host
static int occ_prepare(natac_batch *b) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!c->have_occ) return fail(NATAC_E_STATE, "natac_set_occ_model has not been called");
    const int M = 2 * c->flank + 1;              /* OccupancyParameters.window, Occupancy.py:184 */
    const double sd = c->flank / 3.0;            /* Occupancy.py:220 */
    const int need_l = c->flank + ((c->occ_upper - 2) >> 1), need_r = c->flank + ((c->occ_upper - 1) >> 1) + 1;
    if (b->d_bias && (b->bias_left < need_l || b->bias_right < need_r))
        return fail(NATAC_E_ARG, "bias track must extend >= %d left / %d right of the chunk (has %d / %d)", need_l, need_r,
                    b->bias_left, b->bias_right);
    for (int i = 0; i < b->nc; ++i)
        if (b->h_len[i] < M) return fail(NATAC_E_ARG, "chunk %d shorter (%d) than the occupancy window (%d)", i, b->h_len[i], M);
    int rc;
    if ((rc = ensure_window(c, c->d_win_occ, &c->win_occ_M, &c->win_occ_sd, M, sd))) return rc;
    if (!b->d_grid_off || b->grid_step != c->step) {
        b->h_grid_off.assign((size_t)b->nc + 1, 0);
        for (int i = 0; i < b->nc; ++i) {
            const int nk = (b->h_len[i] > c->halfstep) ? (b->h_len[i] - c->halfstep + c->step - 1) / c->step : 0;
            b->h_grid_off[i + 1] = b->h_grid_off[i] + nk;
        }
        b->total_grid = b->h_grid_off[b->nc];
        HIPCHK(sync_all(c));
        // the grids of the earlier run go with their layout, whatever becomes of this call
        b->out.grids = false;
        if (b->out.track[NATAC_T_OCC_PREFILL] == TS_PENDING) b->out.track[NATAC_T_OCC_PREFILL] = TS_EMPTY;
        if ((rc = dev_upload(c, b->d_grid_off, b->h_grid_off.data(), (size_t)b->nc + 1))) return rc;
        for (auto &g : b->d_grid)
            if ((rc = dev_alloc(g, (size_t)b->total_grid))) return rc;
        if ((rc = build_tiles(b, OCC_T * OCC_NP, b->d_tiles_occ, &b->n_tiles_occ, true, c->step, c->halfstep))) return rc;
        b->d_ranges_occ.reset(); b->d_order_occ.reset();
        if ((rc = dev_alloc(b->d_ranges_occ, (size_t)b->n_tiles_occ))) return rc;
        if ((rc = dev_alloc(b->d_order_occ, (size_t)2 + HEAVY_CAP + ((size_t)b->n_tiles_occ + 3) / 4))) return rc;
        b->ranges_occ_key[0] = -1;       // new tile table: ranges not formed yet
        b->gs_Q = -1;                    // ... and the block tables of natac_occ_gsum follow the grid
        b->grid_step = c->step;
        b->grid_half = c->halfstep;
    }
    for (int i = 0; i < 3; ++i)      // released by natac_batch_release_outputs
        if (!b->d_grid[i] && (rc = dev_alloc(b->d_grid[i], (size_t)b->total_grid))) return rc;
    for (int t : {NATAC_T_OCC, NATAC_T_OCC_LOWER, NATAC_T_OCC_UPPER, NATAC_T_OCC_COV})
        if ((rc = ensure_track(b, t))) return rc;
    if (!b->d_ebias && b->d_bias && (rc = dev_alloc(b->d_ebias, (size_t)b->nb))) return rc;
    const bool fast = c->occ_fast_ok && !c->occ_force_general;
    if (fast) {   // per-block sum buffers + tile table of natac_occ_gsum (geometry: step / flank of the model)
        const int Q = (2 * c->flank + 1) / c->step;      // whole step-blocks of a window; the rest is a prefix of the next block
        if (b->gs_Q != Q) {
            HIPCHK(sync_all(c));
            std::vector<long long> bo((size_t)b->nc + 1);
            std::vector<int2> tiles;
            for (int i = 0; i <= b->nc; ++i) bo[i] = b->h_grid_off[i] + (long long)Q * i;
            for (int i = 0; i < b->nc; ++i) {
                const int nblk = (int)(b->h_grid_off[i + 1] - b->h_grid_off[i]) + Q;
                for (int x = 0; x < nblk; x += GS_BLOCKS) tiles.push_back(make_int2(i, x));
            }
            b->total_blocks = bo[b->nc];
            b->d_blk_off.reset(); b->d_gsum.reset(); b->d_tiles_gs.reset(); b->d_defer.reset();
            if ((rc = dev_upload(c, b->d_blk_off, bo.data(), bo.size()))) return rc;
            if ((rc = dev_upload(c, b->d_tiles_gs, tiles.data(), tiles.size()))) return rc;
            HIPCHK(sync_all(c));
            b->n_tiles_gs = (int)tiles.size();
            if ((rc = dev_alloc(b->d_defer, (size_t)b->n_tiles_occ + 1))) return rc;
            b->gs_Q = Q;
        }
        if (!b->d_gsum && (rc = dev_alloc(b->d_gsum, (size_t)4 * b->total_blocks))) return rc;
    }
    // geometry checks + tables of the smoothing pass
    {
        const int U = c->occ_upper, UP = (U + 1) & ~1;
        const int span = (OCC_T * OCC_NP - 1) * c->step + M + c->step;
        const int EW = span + ((U - 2) >> 1) + ((U - 1) >> 1) + 2;
        const int n_ones = ((OCC_T - 1) * c->step + M + c->step + 3) & ~1;
        const size_t lds = ((size_t)((EW + 1) & ~1) + (size_t)OCC_T * UP + 2 * (size_t)UP + OCC_ACL + n_ones) * sizeof(double) +
                           (size_t)2 * OCC_FMAX * sizeof(int);
        if (lds > 64 * 1024)
            return fail(NATAC_E_ARG, "occupancy window / step too large for the device tile (step=%d flank=%d upper=%d)", c->step, c->flank, U);
        if (fast) {
            const int R = c->occ_nm - 1, Q = b->gs_Q;
            const size_t lds_gs = ((size_t)((GS_BLOCKS * c->step + 2 * R + 2 * GS_MG + 1) & ~1) + 16 * 64) * sizeof(double);
            const int NGP = (64 + Q + 1) & ~1;
            const size_t lds_od = (size_t)4 * ((OD_FM + 4) + 4 * NGP + OD_FM / 2) * sizeof(double);
            if (lds_gs > 64 * 1024 || lds_od > 64 * 1024)
                return fail(NATAC_E_ARG, "occupancy window too large for the device tile (flank=%d upper=%d)", c->flank, U);
        }
    }
    const bool blk = c->step <= 9;     // natac_occ_smooth_blk<1, 3, 5, 7, 9> (the step is odd)
    if (blk) {
        const int NB = occ_smooth_blocks((M - 1) / 2, c->step);
        if ((rc = ensure_block_weights(c, M, sd, NB))) return rc;
        if (b->os_width != 256 * c->step) {
            if ((rc = build_tiles(b, 256 * c->step, b->d_tiles_os, &b->n_tiles_os))) return rc;
            b->os_width = 256 * c->step;
        }
        if (!b->d_occ_minkey && (rc = dev_alloc(b->d_occ_minkey, (size_t)b->nc))) return rc;
        if (!b->d_occ_nan && (rc = dev_alloc(b->d_occ_nan, (size_t)b->nc))) return rc;
    } else {
        if ((rc = ensure_track(b, NATAC_T_OCC_PREFILL))) return rc;
    }
    return NATAC_OK;
}

// natac_run_occ, part 2: the launches
static int occ_launch(natac_batch *b) {
    natac_ctx *c = b->ctx;
    const int M = 2 * c->flank + 1;
    int rc;
    const ChunkTable ct = make_table(b);
    const OccModelDev om = make_occ(c);
    natac_ctx::Ev ev;
    const bool fast = c->occ_fast_ok && !c->occ_force_general;
    prof_begin(c, NATAC_K_OCC_MLE, ev, c->stream);
    // bit 0 of the status words is this stage's: what an earlier run under another model raised does not outlive it
    hipLaunchKernelGGL(natac_status_clear, dim3((b->nc + 255) / 256), dim3(256), 0, c->stream, b->d_status, b->nc, 1);
    {
        const int U = c->occ_upper, UP = (U + 1) & ~1;
        const int span = (OCC_T * OCC_NP - 1) * c->step + M + c->step;
        const int EW = span + ((U - 2) >> 1) + ((U - 1) >> 1) + 2;
        const int n_ones = ((OCC_T - 1) * c->step + M + c->step + 3) & ~1;
        const size_t lds = ((size_t)((EW + 1) & ~1) + (size_t)OCC_T * UP + 2 * (size_t)UP + OCC_ACL + n_ones) * sizeof(double) +
                           (size_t)2 * OCC_FMAX * sizeof(int);
        if (b->ranges_occ_key[0] != c->step || b->ranges_occ_key[1] != c->halfstep || b->ranges_occ_key[2] != c->flank) {
            // an index over the (immutable) fragment list, like the 256-base tiles' ranges: formed once per batch and geometry
            hipLaunchKernelGGL(natac_occ_tile_ranges, dim3((b->n_tiles_occ + 255) / 256), dim3(256), 0, c->stream, ct, b->d_tiles_occ,
                               b->n_tiles_occ, c->step, c->halfstep, c->flank, b->d_ranges_occ);
            // ... and the heavy tiles natac_occ_decide visits first: more than four times the batch's mean fragment count (and > 256)
            const double span = (double)(OCC_T * OCC_NP - 1) * c->step + 2.0 * c->flank + 1.0;
            const int thr = (int)std::max(256.0, 4.0 * (double)b->nf * span / (double)std::max<long long>(1, b->total_bp));
            HIPCHK(hipMemsetAsync(b->d_order_occ, 0, 2 * sizeof(int), c->stream));
            hipLaunchKernelGGL(natac_tile_heavy, dim3((b->n_tiles_occ + 255) / 256), dim3(256), 0, c->stream, b->d_ranges_occ, b->n_tiles_occ, thr,
                               b->d_order_occ, b->d_order_occ + 2, (unsigned char *)(b->d_order_occ + 2 + HEAVY_CAP));
            b->ranges_occ_key[0] = c->step; b->ranges_occ_key[1] = c->halfstep; b->ranges_occ_key[2] = c->flank;
        }
        const int *d_list = nullptr, *d_count = nullptr;
        unsigned grid_general = (unsigned)b->n_tiles_occ;
        if (fast) {
            OccFastDev of;
            of.q4 = c->d_occ_q4; of.rho = c->d_occ_rho; of.alphas = c->d_alphas; of.na = c->n_alpha; of.nm = c->occ_nm; of.upper = U; of.step = c->step;
            of.halfstep = c->halfstep; of.flank = c->flank; of.Q = b->gs_Q; of.flags = (c->occ_zero_flags & 1) | (c->occ_zero_nfr ? 2 : 0);
            of.ci_factor = om.ci_factor; of.e_lo = std::ldexp(1.0, -190); of.e_hi = std::ldexp(1.0, 190);
            const int R = of.nm - 1;
            const size_t lds_gs = ((size_t)((GS_BLOCKS * c->step + 2 * R + 2 * GS_MG + 1) & ~1) + 16 * 64) * sizeof(double);
            const int NGP = (64 + of.Q + 1) & ~1;
            const size_t lds_od = (size_t)4 * ((OD_FM + 4) + 4 * NGP + OD_FM / 2) * sizeof(double);
            HIPCHK(hipMemsetAsync(b->d_defer, 0, sizeof(int), c->stream));
            if ((rc = run_exp_bias(b, c->stream, true))) return rc;
            const OccFastLaunch fl{b, ct, of, lds_gs, lds_od, (2 * c->flank + 1) % c->step, c->occ_rn16};
            switch (c->step) {
                case 1: occ_fast_launch<1>(fl); break;
                case 3: occ_fast_launch<3>(fl); break;
                case 5: occ_fast_launch<5>(fl); break;
                case 7: occ_fast_launch<7>(fl); break;
                default: occ_fast_launch<9>(fl); break;
            }
            d_count = b->d_defer;
            d_list = b->d_defer + 1;
            grid_general = (unsigned)std::min(b->n_tiles_occ, 2048);   // walks the deferred list (normally empty)
        }
        if (c->step == 5 && c->flank == 60 && c->n_alpha <= 16 * OCC_RA)
            hipLaunchKernelGGL((natac_occ_mle<5, 60, 0, 1>), dim3(grid_general), dim3(256), lds, c->stream, ct, b->d_tiles_occ,
                               b->d_ranges_occ, om, b->d_grid[0], b->d_grid[1], b->d_grid[2], b->d_status, d_list, d_count);
        else if (c->step == 5 && c->flank == 60)
            hipLaunchKernelGGL((natac_occ_mle<5, 60, 0>), dim3(grid_general), dim3(256), lds, c->stream, ct, b->d_tiles_occ,
                               b->d_ranges_occ, om, b->d_grid[0], b->d_grid[1], b->d_grid[2], b->d_status, d_list, d_count);
        else
            hipLaunchKernelGGL((natac_occ_mle<0, 0, 0>), dim3(grid_general), dim3(256), lds, c->stream, ct, b->d_tiles_occ,
                               b->d_ranges_occ, om, b->d_grid[0], b->d_grid[1], b->d_grid[2], b->d_status, d_list, d_count);
    }
    prof_end(c, ev);
    prof_begin(c, NATAC_K_OCC_SMOOTH, ev, c->stream);
    const bool blk = c->step <= 9;     // natac_occ_smooth_blk<1, 3, 5, 7, 9> (the step is odd)
    if (blk) {
        const int NB = occ_smooth_blocks((M - 1) / 2, c->step);
        HIPCHK(hipMemsetAsync(b->d_occ_minkey, 0xff, (size_t)b->nc * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(b->d_occ_nan, 0, (size_t)b->nc * sizeof(int), c->stream));
        const size_t lds_os = ((size_t)3 * (256 + NB) + 256 * c->step) * sizeof(double);
        auto ks = c->step == 1 ? natac_occ_smooth_blk<1> : c->step == 3 ? natac_occ_smooth_blk<3> : c->step == 5 ? natac_occ_smooth_blk<5>
                : c->step == 7 ? natac_occ_smooth_blk<7> : natac_occ_smooth_blk<9>;
        hipLaunchKernelGGL(ks, dim3(b->n_tiles_os), dim3(256), lds_os, c->stream, ct,
                           b->d_tiles_os, om, c->d_win_occ, M, c->d_wb_occ, NB, b->d_grid[0], b->d_grid[1], b->d_grid[2],
                           b->d_track[NATAC_T_OCC], b->d_track[NATAC_T_OCC_LOWER], b->d_track[NATAC_T_OCC_UPPER], b->d_occ_minkey,
                           b->d_occ_nan);
    } else {
        launch_occ_smooth_generic(b, ct, om, M, b->d_track[NATAC_T_OCC_PREFILL], b->d_track[NATAC_T_OCC_LOWER],
                                  b->d_track[NATAC_T_OCC_UPPER]);
    }
    {   // OCC_COV: natac_run_nuc's coverage when natac_run_nuc wrote it for this window and size range, else from the fragments
        const bool same = c->flank == b->out.nuc_w && c->occ_upper == b->out.nuc_upper;
        if (same && b->out.occ_cov_by_nuc) {
            // natac_frag_gather of natac_run_nuc already wrote OCC_COV = nuc_cov + nfr_cov for this geometry
        } else if (same && b->out.track[NATAC_T_NUC_COV] == TS_RUN && b->out.track[NATAC_T_NFR_COV] == TS_RUN) {
            hipLaunchKernelGGL(natac_add_tracks, dim3(4096), dim3(256), 0, c->stream, b->d_track[NATAC_T_NUC_COV],
                               b->d_track[NATAC_T_NFR_COV], b->d_track[NATAC_T_OCC_COV], b->total_bp);
        } else {
            hipLaunchKernelGGL(natac_occ_cov, dim3(b->n_tiles256), dim3(256), 0, c->stream, ct, b->d_tiles256, c->occ_upper, c->flank,
                               b->d_track[NATAC_T_OCC_COV]);
            b->out.occ_cov_by_nuc = false;
        }
    }
    prof_end(c, ev);
    prof_begin(c, NATAC_K_OCC_FILL, ev, c->stream);
    if (blk)     // in place, and only the chunks that hold a NaN
        hipLaunchKernelGGL(natac_fill_nan_chunks, dim3(b->nc), dim3(256), 0, c->stream, ct, b->d_occ_minkey, b->d_occ_nan,
                           b->d_track[NATAC_T_OCC]);
    else
        hipLaunchKernelGGL(natac_fill_nan_min, dim3(b->nc), dim3(256), 0, c->stream, ct, b->d_track[NATAC_T_OCC_PREFILL],
                           b->d_track[NATAC_T_OCC]);
    prof_end(c, ev);
    HIPCHK(hipGetLastError());
    for (int t : {NATAC_T_OCC, NATAC_T_OCC_LOWER, NATAC_T_OCC_UPPER, NATAC_T_OCC_COV}) b->out.track[t] = TS_RUN;
    b->out.track[NATAC_T_OCC_PREFILL] = blk ? TS_PENDING : TS_RUN;
    b->out.grids = true;
    b->out.occ_step = c->step; b->out.occ_half = c->halfstep; b->out.occ_flank = c->flank; b->out.occ_upper = c->occ_upper;
    return NATAC_OK;
}

int natac_run_occ(natac_batch *b) {
    int rc = occ_prepare(b);
    if (rc) return rc;
    return occ_launch(b);
}

static int ins_launch(natac_batch *b, int lower, int upper);

int natac_run_ins(natac_batch *b, int lower, int upper) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_track(b, NATAC_T_INS);
    if (rc) return rc;
    return ins_launch(b, lower, upper);
}

static int ins_launch(natac_batch *b, int lower, int upper) {
    natac_ctx *c = b->ctx;
    const ChunkTable ct = make_table(b);
    natac_ctx::Ev ev;
    prof_begin(c, NATAC_K_INS, ev, c->stream);
    const int maxL = b->max_len;
    if ((size_t)maxL * sizeof(int) <= 60 * 1024) {
        hipLaunchKernelGGL(natac_insertions_lds, dim3(b->nc), dim3(256), (size_t)maxL * sizeof(int), c->stream, ct, lower, upper,
                           (int *)b->d_track[NATAC_T_INS].get());
    } else {
        HIPCHK(hipMemsetAsync(b->d_track[NATAC_T_INS], 0, (size_t)b->total_bp * sizeof(int), c->stream));
        hipLaunchKernelGGL(natac_insertions, dim3(b->nc), dim3(256), 0, c->stream, ct, lower, upper, (int *)b->d_track[NATAC_T_INS].get());
    }
    prof_end(c, ev);
    HIPCHK(hipGetLastError());
    b->out.track[NATAC_T_INS] = TS_RUN;
    return NATAC_OK;
}

// the 1-kb tile table of the per-base track kernels (natac_tracks.hpp); the same table natac_smooth_same4 uses
static int ensure_tiles1k(natac_batch *b) {
    static_assert(natac_tracks::TR_TILE == 1024, "the track kernels share the 1-kb tile table");
    if (b->d_tiles1k) return NATAC_OK;
    return build_tiles(b, 1024, b->d_tiles1k, &b->n_tiles1k);
}

int natac_run_ins_smooth(natac_batch *b, int lower, int upper, const double *w, int M, double wsum) {
    using namespace natac_tracks;
    if (!b || !w) return fail(NATAC_E_ARG, "null argument");
    if (M < 1 || M > TR_MAX_M || !(M & 1)) return fail(NATAC_E_ARG, "window needs an odd number of taps in [1, %d] (got %d)", TR_MAX_M, M);
    for (int j = 0; j < M; ++j)
        if (!std::isfinite(w[j])) return fail(NATAC_E_ARG, "window tap %d is not finite", j);
    if (!(wsum > 0) || !std::isfinite(wsum)) return fail(NATAC_E_ARG, "window sum must be positive and finite (got %g)", wsum);
    natac_ctx *c = b->ctx;
    DeviceCall dc(c, "ins_smooth");
    int rc;
    if (!dc.ok()) return dc.finish();
    if ((rc = ensure_track(b, NATAC_T_INS_SMOOTH)) || (rc = ensure_tiles1k(b))) return rc;
    const double *d_w = dc.upload(w, (size_t)M);     // the window: on the device for this call only
    if (dc.ok()) {
        dc.prof_begin(NATAC_K_INS_SMOOTH);
        hipLaunchKernelGGL(natac_ins_smooth, dim3(b->n_tiles1k), dim3(TR_BLOCK), ins_smooth_lds(M), c->stream, b->d_tiles1k.get(), b->d_len.get(),
                           b->d_frag_off.get(), b->d_lpos.get(), b->d_ilen.get(), b->d_centre.get(), b->d_out_off.get(), lower, upper, d_w, M, wsum,
                           b->d_track[NATAC_T_INS_SMOOTH].get());
        dc.prof_end();
        dc.launched();
    }
    if ((rc = dc.finish())) return rc;          // the window must outlive the kernel
    b->out.track[NATAC_T_INS_SMOOTH] = TS_RUN;
    return NATAC_OK;
}

int natac_run_center_cov(natac_batch *b, int lower, int upper, int W, double mult) {
    using namespace natac_tracks;
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    if (W < 1 || W > TR_MAX_W) return fail(NATAC_E_ARG, "window must be in [1, %d] (got %d)", TR_MAX_W, W);
    if (!std::isfinite(mult)) return fail(NATAC_E_ARG, "multiplier must be finite");
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_track(b, NATAC_T_CENTER_COV)) || (rc = ensure_tiles1k(b))) return rc;
    const int h = W / 2;
    natac_ctx::Ev ev;
    prof_begin(c, NATAC_K_CENTER_COV, ev, c->stream);
    hipLaunchKernelGGL(natac_center_cov, dim3(b->n_tiles1k), dim3(TR_BLOCK), center_cov_lds(h), c->stream, b->d_tiles1k.get(), b->d_len.get(),
                       b->d_frag_off.get(), b->d_ilen.get(), b->d_centre.get(), b->d_out_off.get(), lower, upper, h, mult,
                       b->d_track[NATAC_T_CENTER_COV].get());
    prof_end(c, ev);
    HIPCHK(hipGetLastError());
    b->out.track[NATAC_T_CENTER_COV] = TS_RUN;
    return NATAC_OK;
}

int natac_run_pwm_track(natac_batch *b, const int64_t *seq_off, const uint8_t *seq, const double *log_pwm, const uint8_t *nucleotides, int nrow,
                        int K) {
    using namespace natac_tracks;
    if (!b || !seq_off || !seq || !log_pwm || !nucleotides) return fail(NATAC_E_ARG, "null argument");
    if (K < 1 || nrow < 1 || nrow > PT_MAX_ROWS || (long long)nrow * K > PT_MAX_CELLS)
        return fail(NATAC_E_ARG, "PWM needs 1 <= rows <= %d, 1 <= width and rows * width <= %d (got %d x %d)", PT_MAX_ROWS, PT_MAX_CELLS, nrow, K);
    for (int j = 0; j < nrow * K; ++j)
        if (!std::isfinite(log_pwm[j])) return fail(NATAC_E_ARG, "log PWM entry (%d, %d) is not finite", j / K, j % K);
    for (int r = 1; r < nrow; ++r)
        for (int q = 0; q < r; ++q)
            if (nucleotides[q] == nucleotides[r]) return fail(NATAC_E_ARG, "PWM rows %d and %d have the same letter", q, r);
    if (seq_off[0] != 0) return fail(NATAC_E_ARG, "seq_off[0] must be 0");
    for (int i = 0; i < b->nc; ++i)
        if (seq_off[i + 1] - seq_off[i] != (int64_t)b->h_len[i] + K - 1)
            return fail(NATAC_E_ARG, "sequence window of chunk %d must hold %lld bases (its length + K - 1)", i, (long long)b->h_len[i] + K - 1);
    natac_ctx *c = b->ctx;
    DeviceCall dc(c, "pwm_track");
    int rc;
    if (!dc.ok()) return dc.finish();
    if ((rc = ensure_track(b, NATAC_T_BIAS)) || (rc = ensure_tiles1k(b))) return rc;
    // sequence, offsets, table and letters: on the device for this call only
    const unsigned char *d_s = dc.upload((const unsigned char *)seq, (size_t)seq_off[b->nc]);
    const long long *d_so = dc.upload((const long long *)seq_off, (size_t)b->nc + 1);
    const unsigned char *d_n = dc.upload((const unsigned char *)nucleotides, (size_t)nrow);
    const double *d_p = dc.upload(log_pwm, (size_t)nrow * K);
    if (dc.ok()) {
        dc.prof_begin(NATAC_K_PWM_TRACK);
        hipLaunchKernelGGL(natac_pwm_track, dim3(b->n_tiles1k), dim3(TR_BLOCK), pwm_track_lds(nrow, K), c->stream, b->d_tiles1k.get(), b->d_len.get(),
                           d_so, d_s, b->d_out_off.get(), d_p, d_n, nrow, K, b->d_track[NATAC_T_BIAS].get());
        dc.prof_end();
        dc.launched();
    }
    if ((rc = dc.finish())) return rc;           // the host arrays may be released by the caller after return
    b->out.track[NATAC_T_BIAS] = TS_RUN;
    return NATAC_OK;
}

// what launch_candidates reads of the batch: NUC_COV, NORM and, with a bias track, exp(bias) (formed by natac_run_nuc)
static int need_candidate_inputs(natac_batch *b) {
    int rc;
    if ((rc = need_track(b, NATAC_T_NUC_COV)) || (rc = need_track(b, NATAC_T_NORM))) return rc;
    if (b->d_bias && !b->d_ebias) return fail(NATAC_E_STATE, "natac_run_nuc must run before the candidate statistics (exp(bias))");
    return NATAC_OK;
}

int natac_run_candidates(natac_batch *b, int64_t n_cand, const int32_t *cand_chunk, const int32_t *cand_pos, double *lr,
                         double *var, double *z) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    natac_ctx *c = b->ctx;
    int rc = need_candidate_inputs(b);
    if (rc || (rc = need_nuc_geometry(b, "natac_run_candidates"))) return rc;
    if (n_cand < 0 || (n_cand > 0 && (!cand_chunk || !cand_pos || !lr || !var || !z))) return fail(NATAC_E_ARG, "null argument");
    if (n_cand == 0) return NATAC_OK;
    if (n_cand > 0x7fffffffLL) return fail(NATAC_E_ARG, "too many candidates");
    DeviceCall dc(c, "candidates");
    if (!dc.ok()) return dc.finish();
    for (int64_t k = 0; k < n_cand; ++k) {
        const int ci = cand_chunk[k];
        if (ci < 0 || ci >= b->nc || cand_pos[k] < 0 || cand_pos[k] >= b->h_len[ci])
            return fail(NATAC_E_ARG, "candidate %lld out of range (chunk %d pos %d)", (long long)k, ci, cand_pos[k]);
    }
    if ((rc = ensure_srow(c))) return rc;      // the size weights of the model that is set now, whichever call set it
    const int *d_cc = dc.upload(cand_chunk, (size_t)n_cand), *d_cp = dc.upload(cand_pos, (size_t)n_cand);
    double *d_out = dc.alloc<double>((size_t)3 * n_cand);
    if (dc.ok()) {
        const ChunkTable ct = make_table(b);
        const VMatDev vm = make_vmat(c);
        dc.prof_begin(NATAC_K_CAND);
        launch_candidates(c, ct, vm, d_cc, d_cp, n_cand, b->d_track[NATAC_T_NUC_COV], b->d_track[NATAC_T_NORM],
                          b->out.bg_gen == c->model_gen ? b->d_bnum : nullptr, b->out.bg_gen == c->model_gen ? b->d_bcov : nullptr, d_out,
                          d_out + n_cand,
                          d_out + 2 * n_cand, b->ranges256_w == c->vw ? b->d_tile256_first : nullptr, b->ranges256_w == c->vw ? b->d_ranges256 : nullptr);
        dc.prof_end();
        dc.launched();
    }
    dc.fetch(lr, d_out, (size_t)n_cand);
    dc.fetch(var, d_out + n_cand, (size_t)n_cand);
    dc.fetch(z, d_out + 2 * n_cand, (size_t)n_cand);
    return dc.finish();
}

int natac_run_candidates_cov(natac_batch *b, int64_t n_cand, const int32_t *cand_chunk, const int32_t *cand_pos, int mode,
                             double *var) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    natac_ctx *c = b->ctx;
    int rc = need_track(b, NATAC_T_NUC_COV);
    if (rc || (rc = need_nuc_geometry(b, "natac_run_candidates_cov"))) return rc;
    if (mode < 0 || mode > 2) return fail(NATAC_E_ARG, "mode must be 0 (closed form), 1 (literal) or 2 (closed form in fp32)");
    if (n_cand < 0 || (n_cand > 0 && (!cand_chunk || !cand_pos || !var))) return fail(NATAC_E_ARG, "null argument");
    if (n_cand == 0) return NATAC_OK;
    DeviceCall dc(c, "candidates_cov");
    if (!dc.ok()) return dc.finish();
    for (int64_t k = 0; k < n_cand; ++k) {
        const int ci = cand_chunk[k];
        if (ci < 0 || ci >= b->nc || cand_pos[k] < 0 || cand_pos[k] >= b->h_len[ci])
            return fail(NATAC_E_ARG, "candidate %lld out of range (chunk %d pos %d)", (long long)k, ci, cand_pos[k]);
    }
    if ((rc = ensure_srow(c))) return rc;
    const int N = c->R * c->W;
    const int NBLK = 64;                       // row groups of the literal pair sum per candidate
    const int64_t SLAB = 2048;                 // candidates per pass: 2048 x N doubles = 289 MB for the default V-plot
    const ChunkTable ct = make_table(b);
    const VMatDev vm = make_vmat(c);
    const int EW = c->W + ((c->vupper - 2) >> 1) + ((c->vupper - 1) >> 1);
    const int64_t slab = std::min<int64_t>(SLAB, n_cand);
    std::vector<double> part((size_t)slab * NBLK);
    int *d_cc = dc.alloc<int>((size_t)slab), *d_cp = dc.alloc<int>((size_t)slab);
    double *d_p = dc.alloc<double>((size_t)slab * N), *d_out = dc.alloc<double>((size_t)slab * NBLK);
    for (int64_t k0 = 0; k0 < n_cand; k0 += slab) {
        const int64_t m = std::min<int64_t>(slab, n_cand - k0);
        const int per = mode == 1 ? NBLK : 1;
        dc.send(d_cc, cand_chunk + k0, (size_t)m);
        dc.send(d_cp, cand_pos + k0, (size_t)m);
        if (dc.ok()) {
            hipLaunchKernelGGL(natac_cand_window_probs, dim3((unsigned)m), dim3(256), (size_t)(EW + 2) * sizeof(double), c->stream, ct, vm,
                               d_cc, d_cp, d_p);
            dc.launched();
        }
        if (dc.ok()) {
            if (mode == 1)
                hipLaunchKernelGGL(natac_cov_literal_many, dim3(NBLK, (unsigned)m), dim3(256), 0, c->stream, d_p, c->d_vmat, N, d_out);
            else if (mode == 0)
                hipLaunchKernelGGL((natac_cov_closed_many<double>), dim3((unsigned)m), dim3(256), 0, c->stream, d_p, c->d_vmat, N, d_out);
            else
                hipLaunchKernelGGL((natac_cov_closed_many<float>), dim3((unsigned)m), dim3(256), 0, c->stream, d_p, c->d_vmat, N, d_out);
            dc.launched();
        }
        dc.fetch(part.data(), d_out, (size_t)m * per);
        if ((rc = dc.sync())) return rc;
        for (int64_t k = 0; k < m; ++k) {
            double s = 0;
            for (int j = 0; j < per; ++j) s += part[(size_t)k * per + j];
            var[k0 + k] = s;
        }
    }
    // r = int(nuc_cov[pos]) like the .pyx's `int r` (NucleosomeCalling.py:125): one gather of the coverage values
    std::vector<double> reads((size_t)n_cand);
    std::vector<long long> idx((size_t)n_cand);
    for (int64_t k = 0; k < n_cand; ++k) idx[(size_t)k] = b->h_out_off[cand_chunk[k]] + cand_pos[k];
    const long long *d_idx = dc.upload(idx.data(), (size_t)n_cand);
    double *d_r = dc.alloc<double>((size_t)n_cand);
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_gather_f64, dim3((unsigned)((n_cand + 255) / 256)), dim3(256), 0, c->stream,
                           b->d_track[NATAC_T_NUC_COV], d_idx, (long long)n_cand, d_r);
        dc.launched();
    }
    dc.fetch(reads.data(), d_r, (size_t)n_cand);
    if ((rc = dc.finish())) return rc;
    for (int64_t k = 0; k < n_cand; ++k) var[k] = var[k] * cov_reads(reads[(size_t)k]);
    return NATAC_OK;
}

// natac_run_peaks with SMOOTH still pending (so peaks_can_smooth() held): does the search take a kernel arm that forms it?
static bool peaks_smooth_arm(const natac_batch *b, int order) {
    return order >= 1 && order <= 255 && peaks_plan(b->max_len, order).forms_smooth;
}

// form_smooth: sig_b is the batch's pending SMOOTH and peaks_smooth_arm() holds -- the search forms it from sig_a (the batch's NORM)
static int run_peaks_impl(natac_batch *b, const double *sig_a, const double *sig_b, bool with_stats, double min_signal, int sep,
                          int boundary, int order, const double *jitter, int64_t n_jitter, int64_t *n_cand, bool form_smooth = false) {
    if (!b || !jitter || !n_cand) return fail(NATAC_E_ARG, "null argument");
    natac_ctx *c = b->ctx;
    if (order < 1 || order > 255 || sep < 1 || boundary < 0) return fail(NATAC_E_ARG, "bad peak parameters");
    const int maxL = b->max_len;
    if (n_jitter < maxL) return fail(NATAC_E_ARG, "jitter stream (%lld) shorter than the longest chunk (%d)", (long long)n_jitter, maxL);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    int rc;
    if (with_stats && (rc = ensure_srow(c))) return rc;      // as natac_run_candidates
    if (!b->d_jitter || b->n_jitter < maxL) {
        if ((rc = dev_upload(c, b->d_jitter, jitter, (size_t)maxL))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        b->n_jitter = maxL;
    } else {
        HIPCHK(hipMemcpyAsync(b->d_jitter, jitter, (size_t)maxL * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (b->pk_order != order) {   // slot regions: a chunk of L bases holds at most L/(order+1) + 1 maxima
        std::vector<long long> cap((size_t)b->nc + 1, 0);
        for (int i = 0; i < b->nc; ++i) cap[i + 1] = cap[i] + b->h_len[i] / (order + 1) + 2;
        b->slot_total = cap[b->nc];
        b->d_cap_off.reset(); b->d_slot.reset();
        if ((rc = dev_upload(c, b->d_cap_off, cap.data(), (size_t)b->nc + 1))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        if ((rc = dev_alloc(b->d_slot, (size_t)b->slot_total))) return rc;
        b->pk_order = order;
    }
    if (!b->d_pk_count && (rc = dev_alloc(b->d_pk_count, (size_t)b->nc))) return rc;
    if (!b->d_pk_offs && (rc = dev_alloc(b->d_pk_offs, (size_t)b->nc + 1))) return rc;
    // the window natac_run_nuc was asked for; the context's may be another batch's by now
    if (form_smooth &&
        (rc = ensure_window(c, c->d_win_nuc, &c->win_nuc_M, &c->win_nuc_sd, b->out.smooth_M, b->out.smooth_sd, &c->win_nuc_sum))) return rc;
    const PeakPlan plan = peaks_plan(maxL, order);
    PeakSearch s{sig_a, sig_b, b->d_jitter, min_signal, boundary, order, sep, b->d_cap_off, b->d_slot, b->d_pk_count, b->d_status,
                 b->d_pk_offs, c->d_win_nuc, c->win_nuc_sum, form_smooth ? b->d_track[NATAC_T_SMOOTH].get() : nullptr};
    if (plan.global_lists) {      // per slot: sig (8 bytes) + pos (4) + state (1), laid out as three arrays in one block
        if (b->d_pk_big.size() < (size_t)b->slot_total * 2 + 2 && (rc = dev_alloc(b->d_pk_big, (size_t)b->slot_total * 2 + 2))) return rc;
        s.big_sig = b->d_pk_big;
        s.big_pos = (int *)(b->d_pk_big + b->slot_total);
        s.big_state = (unsigned char *)(s.big_pos + b->slot_total);
    }
    natac_ctx::Ev ev;
    prof_begin(c, NATAC_K_CAND, ev);
    const ChunkTable ct = make_table(b);
    if ((rc = peaks_enqueue(plan, ct, b->nc, s, c->stream))) return rc;
    long long total = 0;
    HIPCHK(hipGetLastError());
    if (form_smooth) b->out.track[NATAC_T_SMOOTH] = TS_RUN;
    HIPCHK(hipMemcpyAsync(&total, b->d_pk_offs + b->nc, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (total > b->pk_cap) {      // pk_cap is the stride of all three: set once they all exist, 0 while they do not
        b->d_pk_chunk.reset(); b->d_pk_pos.reset(); b->d_pk_out.reset();
        b->pk_cap = 0;
        const long long cap = total + total / 4 + 16;
        if ((rc = dev_alloc(b->d_pk_chunk, (size_t)cap)) || (rc = dev_alloc(b->d_pk_pos, (size_t)cap)) ||
            (rc = dev_alloc(b->d_pk_out, (size_t)3 * cap))) {
            b->d_pk_chunk.reset(); b->d_pk_pos.reset();
            return rc;
        }
        b->pk_cap = cap;
    }
    if (total > 0) {
        hipLaunchKernelGGL(natac_compact_candidates, dim3((b->nc + 3) / 4), dim3(256), 0, c->stream, b->nc, b->d_pk_count, b->d_pk_offs,
                           b->d_cap_off, b->d_slot, b->d_pk_chunk, b->d_pk_pos);
        if (with_stats) {
            const VMatDev vm = make_vmat(c);
            launch_candidates(c, ct, vm, b->d_pk_chunk, b->d_pk_pos, total, b->d_track[NATAC_T_NUC_COV], b->d_track[NATAC_T_NORM],
                              b->out.bg_gen == c->model_gen ? b->d_bnum : nullptr, b->out.bg_gen == c->model_gen ? b->d_bcov : nullptr,
                              b->d_pk_out, b->d_pk_out + b->pk_cap, b->d_pk_out + 2 * b->pk_cap,
                              b->ranges256_w == c->vw ? b->d_tile256_first : nullptr, b->ranges256_w == c->vw ? b->d_ranges256 : nullptr);
        }
    }
    b->pk_has_stats = with_stats;
    prof_end(c, ev);
    HIPCHK(hipGetLastError());
    b->pk_n = total;
    *n_cand = total;
    return NATAC_OK;
}

int natac_peaks_plan(int32_t max_len, int32_t order, int32_t *kernel, int32_t *bt, int32_t *nj, int32_t *mask, int32_t *global_lists,
                     int32_t *forms_smooth, int32_t *pk_cap, int64_t *lds_bytes) {
    if (!kernel || !bt || !nj || !mask || !global_lists || !forms_smooth || !pk_cap || !lds_bytes) return fail(NATAC_E_ARG, "null argument");
    if (max_len < 1 || order < 1 || order > 255) return fail(NATAC_E_ARG, "natac_peaks_plan: a positive length and an order in 1..255");
    const PeakPlan p = peaks_plan(max_len, order);
    *kernel = p.kernel; *bt = p.bt; *nj = p.nj; *mask = p.mask; *global_lists = p.global_lists; *forms_smooth = p.forms_smooth;
    *pk_cap = p.pk_cap;
    lds_bytes[0] = (int64_t)p.lds; lds_bytes[1] = (int64_t)p.lds_smooth;
    return NATAC_OK;
}

int natac_run_peaks(natac_batch *b, double min_signal, int sep, int boundary, int order, const double *jitter, int64_t n_jitter,
                    int64_t *n_cand) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    int rc;
    // a SMOOTH that natac_run_nuc left pending (NORM is still its own then) is formed by the search where its kernel can, else here
    const bool form_smooth = b->out.track[NATAC_T_SMOOTH] == TS_PENDING && peaks_smooth_arm(b, order);
    if ((!form_smooth && (rc = need_track(b, NATAC_T_SMOOTH))) || (rc = need_candidate_inputs(b)) ||
        (rc = need_nuc_geometry(b, "natac_run_peaks"))) return rc;
    return run_peaks_impl(b, b->d_track[NATAC_T_NORM], b->d_track[NATAC_T_SMOOTH], true, min_signal, sep, boundary, order, jitter,
                          n_jitter, n_cand, form_smooth);
}

int natac_run_track_peaks(natac_batch *b, int track, double min_signal, int sep, int boundary, int order, const double *jitter,
                          int64_t n_jitter, int64_t *n_peaks) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    if (track == NATAC_T_INS) return fail(NATAC_E_ARG, "peak search needs a float64 track");
    int rc = need_track(b, track);
    if (rc) return rc;
    return run_peaks_impl(b, b->d_track[track], nullptr, false, min_signal, sep, boundary, order, jitter, n_jitter, n_peaks);
}

int natac_run_occ_peaks(natac_batch *b, double min_occ, int sep, const double *jitter, int64_t n_jitter, int64_t *n_peaks) {
    if (!b || !n_peaks) return fail(NATAC_E_ARG, "null argument");
    int rc;
    for (int t : {NATAC_T_OCC, NATAC_T_OCC_LOWER, NATAC_T_OCC_UPPER, NATAC_T_OCC_COV}) if ((rc = need_track(b, t))) return rc;
    // natac_occ_peak_dist reads the context's flank and size range next to the run's tracks
    if ((rc = need_occ_geometry(b, "natac_run_occ_peaks"))) return rc;
    natac_ctx *c = b->ctx;
    const int U = c->occ_upper;
    if (U > 1024) return fail(NATAC_E_ARG, "upper > 1024");
    // OccChunk.callPeaks: call_peaks(smoothed_vals, sep, min_signal = min_occ), boundary = sep / 2, order = 1 (Occupancy.py:227)
    rc = run_peaks_impl(b, b->d_track[NATAC_T_OCC], nullptr, false, min_occ, sep, sep / 2, 1, jitter, n_jitter, n_peaks);
    if (rc) return rc;
    const long long n = *n_peaks;
    if (n > b->opk_cap || !b->d_opk_vals) {     // opk_cap is the stride of both: set once both exist, 0 while they do not
        if (n > b->opk_cap) HIPCHK(sync_all(c));
        const long long cap = n > b->opk_cap ? n + n / 4 + 16 : 16;
        b->d_opk_vals.reset(); b->d_opk_keep.reset();
        b->opk_cap = 0;
        if ((rc = dev_alloc(b->d_opk_vals, (size_t)4 * cap)) || (rc = dev_alloc(b->d_opk_keep, (size_t)cap))) {
            b->d_opk_vals.reset();
            return rc;
        }
        b->opk_cap = cap;
    }
    if (!b->d_nuc_dist || b->nd_upper != U) {
        HIPCHK(sync_all(c));
        if ((rc = dev_alloc(b->d_nuc_dist, (size_t)b->nc * U))) return rc;
        b->nd_upper = U;
    }
    const ChunkTable ct = make_table(b);
    natac_ctx::Ev ev;
    prof_begin(c, NATAC_K_CAND, ev);
    hipLaunchKernelGGL(natac_occ_peak_dist, dim3(b->nc), dim3(256), (size_t)U * sizeof(int), c->stream, ct, b->d_pk_offs, b->d_pk_pos,
                       b->d_track[NATAC_T_OCC], b->d_track[NATAC_T_OCC_LOWER], b->d_track[NATAC_T_OCC_UPPER],
                       b->d_track[NATAC_T_OCC_COV], min_occ, c->flank, U, b->opk_cap, b->d_opk_vals, b->d_opk_keep, b->d_nuc_dist);
    prof_end(c, ev);
    HIPCHK(hipGetLastError());
    b->opk_n = n;
    return NATAC_OK;
}

int natac_download_occ_peaks(natac_batch *b, int64_t n, int32_t *chunk, int32_t *pos, double *occ, double *lower, double *upper,
                             double *reads, int32_t *keep) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    if (b->opk_n < 0 || b->opk_n != b->pk_n) return fail(NATAC_E_STATE, "natac_run_occ_peaks has not run (or another peak search ran since)");
    if (n != b->opk_n) return fail(NATAC_E_ARG, "expected %lld peaks, got buffers for %lld", b->opk_n, (long long)n);
    if (n == 0) return NATAC_OK;
    if (!chunk || !pos || !occ || !lower || !upper || !reads || !keep) return fail(NATAC_E_ARG, "null argument");
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    const size_t nb = (size_t)n * sizeof(double);
    HIPCHK(hipMemcpyAsync(chunk, b->d_pk_chunk, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pos, b->d_pk_pos, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(occ, b->d_opk_vals, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(lower, b->d_opk_vals + b->opk_cap, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(upper, b->d_opk_vals + 2 * b->opk_cap, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(reads, b->d_opk_vals + 3 * b->opk_cap, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(keep, b->d_opk_keep, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    return NATAC_OK;
}

int natac_download_nuc_dist(natac_batch *b, double *dst, size_t dst_bytes) {
    if (!b || !dst) return fail(NATAC_E_ARG, "null argument");
    if (b->opk_n < 0 || !b->d_nuc_dist) return fail(NATAC_E_STATE, "natac_run_occ_peaks has not run");
    const size_t need = (size_t)b->nc * b->nd_upper * sizeof(double);
    if (dst_bytes != need) return fail(NATAC_E_ARG, "destination holds %zu bytes, nuc_dist needs %zu", dst_bytes, need);
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipMemcpyAsync(dst, b->d_nuc_dist, need, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    return NATAC_OK;
}

int natac_download_peaks(natac_batch *b, int64_t n, int32_t *cand_chunk, int32_t *cand_pos, double *lr, double *var, double *z) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    if (b->pk_n < 0) return fail(NATAC_E_STATE, "natac_run_peaks has not run");
    if (n != b->pk_n) return fail(NATAC_E_ARG, "expected %lld candidates, got buffers for %lld", b->pk_n, (long long)n);
    if (n == 0) return NATAC_OK;
    if (!cand_chunk || !cand_pos) return fail(NATAC_E_ARG, "null argument");
    if ((lr || var || z) && !b->pk_has_stats) return fail(NATAC_E_STATE, "the last peak search computed no candidate statistics");
    if (b->pk_has_stats && (!lr || !var || !z)) return fail(NATAC_E_ARG, "null argument");
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(cand_chunk, b->d_pk_chunk, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cand_pos, b->d_pk_pos, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (b->pk_has_stats) {
        HIPCHK(hipMemcpyAsync(lr, b->d_pk_out, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(var, b->d_pk_out + b->pk_cap, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(z, b->d_pk_out + 2 * b->pk_cap, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    prof_collect(c);
    return NATAC_OK;
}

int natac_batch_download(natac_batch *b, int track, void *dst, size_t dst_bytes) {
    if (!b || !dst) return fail(NATAC_E_ARG, "null argument");
    int rc = need_track(b, track);
    if (rc) return rc;
    const size_t need = (size_t)b->total_bp * (track == NATAC_T_INS ? sizeof(int) : sizeof(double));
    if (dst_bytes != need) return fail(NATAC_E_ARG, "destination holds %zu bytes, track needs %zu", dst_bytes, need);
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipMemcpyAsync(dst, b->d_track[track], need, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(sync_all(b->ctx));
    prof_collect(b->ctx);
    return NATAC_OK;
}

int natac_batch_download_grid(natac_batch *b, int which, double *dst, size_t dst_bytes) {
    if (!b || !dst) return fail(NATAC_E_ARG, "null argument");
    if (which < 0 || which > 2) return fail(NATAC_E_ARG, "bad grid id");
    if (!b->out.grids) return fail(NATAC_E_STATE, "natac_run_occ has not run");
    const size_t need = (size_t)b->total_grid * sizeof(double);
    if (dst_bytes != need) return fail(NATAC_E_ARG, "destination holds %zu bytes, grid needs %zu", dst_bytes, need);
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipMemcpyAsync(dst, b->d_grid[which], need, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(sync_all(b->ctx));
    return NATAC_OK;
}

int natac_batch_set_track(natac_batch *b, int track, const double *vals, size_t n) {
    if (!b || !vals) return fail(NATAC_E_ARG, "null argument");
    if (track < 0 || track >= NATAC_T_COUNT || track == NATAC_T_INS) return fail(NATAC_E_ARG, "bad track id %d (float64 tracks only)", track);
    if (n != (size_t)b->total_bp) return fail(NATAC_E_ARG, "track needs %lld values, got %zu", b->total_bp, n);
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    int rc;
    // a pending background is formed from NUC_COV: it keeps the values natac_run_nuc gave it
    if (track == NATAC_T_NUC_COV && b->out.track[NATAC_T_BACKGROUND] == TS_PENDING && (rc = materialise_bg(b))) return rc;
    // ... and a pending SMOOTH is formed from NORM
    if (track == NATAC_T_NORM && b->out.track[NATAC_T_SMOOTH] == TS_PENDING && (rc = materialise_smooth(b))) return rc;
    HIPCHK(sync_all(c));
    if ((rc = ensure_track(b, track))) return rc;
    HIPCHK(hipMemcpyAsync(b->d_track[track], vals, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    b->out.track[track] = TS_HOST;      // and no other track changes state
    if (track == NATAC_T_OCC_COV) b->out.occ_cov_by_nuc = false;
    return NATAC_OK;
}

int natac_batch_status(natac_batch *b, int32_t *dst, size_t dst_bytes) {
    if (!b || !dst) return fail(NATAC_E_ARG, "null argument");
    if (dst_bytes != (size_t)b->nc * sizeof(int)) return fail(NATAC_E_ARG, "status buffer must hold n_chunks int32");
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipMemcpyAsync(dst, b->d_status, dst_bytes, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(sync_all(b->ctx));
    return NATAC_OK;
}

int natac_batch_track_ptr(natac_batch *b, int track, void **dptr) {
    if (!b || !dptr) return fail(NATAC_E_ARG, "null argument");
    if (track < 0 || track >= NATAC_T_COUNT) return fail(NATAC_E_ARG, "bad track id");
    *dptr = nullptr;
    if (b->out.track[track] == TS_EMPTY) return NATAC_OK;
    int rc = need_track(b, track);
    if (rc) return rc;
    *dptr = b->d_track[track];
    return NATAC_OK;
}

/* ---------------- pinned host memory + pool control ---------------- */

int natac_host_alloc(size_t bytes, void **out) {
    if (!out) return fail(NATAC_E_ARG, "out is NULL");
    *out = nullptr;
    if (bytes == 0) bytes = 1;
    HIPCHK(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return NATAC_OK;
}

int natac_host_free(void *p) {
    if (!p) return NATAC_OK;
    HIPCHK(hipHostFree(p));
    return NATAC_OK;
}

int natac_pool_trim(void) {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (int d = 0; d < 16; ++d) {
        if (g_pool.free_blocks[d].empty()) continue;
        (void)hipSetDevice(d);
        (void)hipDeviceSynchronize();
        g_pool.trim_locked(d);
    }
    (void)hipSetDevice(cur);
    return NATAC_OK;
}

}  // extern "C"
