/* natac.h -- C-ABI of libnatac_hip.so: NucleoATAC's per-chunk occ + nuc signal path on MI355X (gfx950).
 *
 * The reference (GreenleafLab/NucleoATAC v0.3.4, Python 2.7 + Cython) has no FFI surface; its de-facto
 * operator boundary is
 *   (1) the per-chunk map functions handed to multiprocessing.Pool.map:
 *         _occHelper  nucleoatac/run_occ.py:23-39   -> natac_run_occ  (+ natac_batch_download)
 *         _nucHelper  nucleoatac/run_nuc.py:22-39   -> natac_run_nuc, natac_run_candidates
 *   (2) the two Cython extension modules:
 *         pyatac/fragments.pyx:17   makeFragmentMat               -> natac_make_fragment_mat
 *         pyatac/fragments.pyx:43   getInsertions                 -> natac_get_insertions / natac_run_ins
 *         pyatac/fragments.pyx:71   getStrandedInsertions         -> natac_get_stranded_insertions
 *         pyatac/fragments.pyx:123  getFragmentSizesFromChunkList -> natac_fragment_sizes
 *         nucleoatac/multinomial_cov.pyx:20 calculateCov          -> natac_calculate_cov
 *   (3) `pyatac pwm`'s window counts (pyatac/get_pwm.py:21-40, tracks.py:179-201) -> natac_insertion_seq_counts
 *       and its background base counts (pyatac/seq.py:47-72)                   -> natac_base_counts
 *   (4) `pyatac ins --smooth`'s smoothed insertions (pyatac/get_ins.py:20-32)  -> natac_run_ins_smooth
 *       and `pyatac cov`'s fragment-centre coverage (pyatac/get_cov.py:21-37)   -> natac_run_center_cov
 *   (5) `pyatac bias`'s Tn5 bias track (pyatac/make_bias_track.py, bias.py:85-92) -> natac_run_pwm_track
 *   (6) `pyatac counts`'s per-region fragment counts (pyatac/get_counts.py:30-45) -> natac_region_counts
 *       and `pyatac nucleotide`'s word counts around sites (pyatac/get_nucleotide.py:19-38) -> natac_site_seq_counts
 *   (7) `pyatac signal`'s per-site rows and their aggregate (pyatac/signal_around_sites.py:24-74) -> natac_site_signal
 *   (8) the reference's only input, a BAM read through pysam (pyatac/fragments.pyx:21-25) -> natac_bam_open / natac_bam_open_device,
 *       or, where only a fragment file (fragments.tsv.gz) is left of it, natac_frag_open / natac_frag_open_device
 * Every entry point below names the reference code it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no exceptions, no C++/torch types.  Return value: 0 = ok, <0 = error class
 *     (NATAC_E_*); natac_last_error() gives the message (thread-local).
 *   - a context (natac_ctx) owns one HIP device + one stream; one host thread per context.
 *   - host pointers are caller-owned; the library copies.  Device outputs live in the batch until it is freed.
 *   - all float tracks are float64 like the reference (pyatac/fragments.pyx:9, chunkmat2d.py:20); insertion
 *     counts are int32.
 *   - fragments are (l, n) = (pos+4, |tlen|-8) of forward proper-pair reads (pyatac/fragments.pyx:25-31),
 *     packed per chunk as in nucleoatac_amd/packing.py and SORTED BY CENTRE l + (n-1)//2 inside a chunk.
 */
#ifndef NATAC_H
#define NATAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an entry point is added, removed or changes meaning (2: round 5 removed natac_run_nuc_occ, added natac_bg_tiling /
 * natac_store_set_budget / natac_store_declined, gave natac_store_adopt's n_hard == -1 a meaning; 3: round 6 added natac_batch_format_fetch_begin / _wait;
 * 4: added natac_insertion_seq_counts / natac_base_counts for `pyatac pwm`; 5: added natac_run_ins_smooth / natac_run_center_cov and their
 * tracks and profile slots for `pyatac ins` / `cov`; 6: added natac_run_pwm_track, its track and profile slot for `pyatac bias`; 7: added natac_region_counts
 * for `pyatac counts` and natac_site_seq_counts for `pyatac nucleotide`; 8: added natac_site_signal and NATAC_SIGNAL_SEG for `pyatac signal`;
 * 9: added natac_frag_open / natac_frag_open_device for fragment files; 10: added natac_frag_split / natac_frag_split_device; 11: added
 * natac_frag_open_cells / natac_bam_ref_cells and natac_region_cell_counts for `pyatac cellcounts`; 12: added natac_ctx_occ_route, and
 * natac_set_occ_model refuses alphas below 2^-500 under a model with a zero nfr probability; 13: added natac_frag_cells /
 * natac_frag_cells_device and natac_cells_counts / _read / _close for `pyatac cells`; 14: added natac_cell_site_qc for `pyatac cellqc`;
 * 15: added natac_enriched_regions for `pyatac peaks`; 16: added natac_sparse_lsi for `pyatac cluster`; 17: added natac_peaks_plan; 18: added natac_motif_scan for
 * `pyatac motifs`; 19: added natac_motif_deviations and natac_window_base_counts for `pyatac deviations`; 20: added
 * natac_motif_deviations_plan; 21: added natac_group_rank_sums and natac_group_rank_sums_plan for `pyatac markers`; 22: added
 * natac_window_pair_sums and natac_window_pair_sums_plan for `pyatac coaccess`; 23: added natac_gene_cell_scores and
 * natac_gene_cell_scores_plan for `pyatac genescores`; 24: added natac_knn and natac_knn_plan for `pyatac doublets`); the binding refuses
 * another version */
#define NATAC_ABI_VERSION 24

enum {
    NATAC_OK = 0,
    NATAC_E_ARG = -1,   /* bad argument / inconsistent sizes */
    NATAC_E_HIP = -2,   /* HIP runtime error (no device, launch failure, ...) */
    NATAC_E_STATE = -3, /* call order: constants not set, or an input the call reads holds nothing.  A per-base track holds
                         * something once the stage that writes it has run (natac_run_nuc: NUC_COV .. SMOOTH; natac_run_occ: OCC ..
                         * OCC_COV, OCC_PREFILL and the grids; natac_run_ins: INS) or natac_batch_set_track wrote it; each track
                         * counts on its own, and natac_batch_release_outputs empties them all */
    NATAC_E_NOMEM = -4
};

/* per-base tracks of a batch (concatenated over chunks in chunk order; chunk i occupies
 * [out_off[i], out_off[i+1]) ).  float64 unless noted. */
enum {
    NATAC_T_NUC_COV = 0,    /* CoverageTrack rows [vlower,vupper)   NucleosomeCalling.py:257-260 */
    NATAC_T_NFR_COV = 1,    /* CoverageTrack rows [0,vlower)        NucleosomeCalling.py:271-273 */
    NATAC_T_RAW = 2,        /* SignalTrack.calculateSignal           NucleosomeCalling.py:29-36  (nucleoatac_raw) */
    NATAC_T_BACKGROUND = 3, /* BiasTrack.calculateBackgroundSignal   NucleosomeCalling.py:49-64  (nucleoatac_background; an output only with
                             * --write_all: after the FFT kernel it is formed on the first download / track_ptr / writer request) */
    NATAC_T_NORM = 4,       /* NormSignalTrack                       NucleosomeCalling.py:38-43  (nucleoatac_signal) */
    NATAC_T_SMOOTH = 5,     /* NucChunk.smoothSignal                 NucleosomeCalling.py:274-283 (nucleoatac_signal.smooth; with smooth_sd 10
                             * and chunks up to 4,096 bases it is formed by natac_run_peaks, or on the first other request, from the
                             * T_NORM and the window natac_run_nuc ran with) */
    NATAC_T_OCC = 6,        /* OccupancyTrack.smoothed_vals AFTER call_peaks' in-place NaN fill (Occupancy.py:147-153, utils.py:86-91) */
    NATAC_T_OCC_LOWER = 7,  /* smoothed_lower */
    NATAC_T_OCC_UPPER = 8,  /* smoothed_upper */
    NATAC_T_OCC_COV = 9,    /* OccChunk.getCov                       Occupancy.py:221-224 */
    NATAC_T_INS = 10,       /* int32 insertion counts, getInsertions pyatac/fragments.pyx:43-67 */
    NATAC_T_OCC_PREFILL = 11, /* smoothed_vals BEFORE the NaN fill (formed on the first download / track_ptr request) */
    NATAC_T_INS_SMOOTH = 12,  /* gaussian-smoothed insertions, `pyatac ins --smooth`   pyatac/get_ins.py:20-32 */
    NATAC_T_CENTER_COV = 13,  /* fragment-centre coverage, `pyatac cov`               pyatac/get_cov.py:21-37 */
    NATAC_T_BIAS = 14,        /* log Tn5 bias of every base, `pyatac bias`            pyatac/bias.py:85-92 */
    NATAC_T_COUNT = 15
};

/* per-grid-point arrays of the occupancy MLE (one value per `step` bases; chunk i occupies
 * [grid_off[i], grid_off[i+1]) with grid point k at base halfstep + k*step):
 * OccupancyTrack.vals / lower_bound / upper_bound before smoothing (Occupancy.py:128-146). */
enum { NATAC_G_OCC = 0, NATAC_G_LOWER = 1, NATAC_G_UPPER = 2 };

/* kernels, for natac_profile_get */
enum {
    NATAC_K_FRAG_GATHER = 0, /* nuc_cov / nfr_cov / raw (sparse V-plot gather) */
    NATAC_K_BACKGROUND = 1,  /* dense bias x VMat correlation (dominant) */
    NATAC_K_SMOOTH_NUC = 2,
    NATAC_K_OCC_MLE = 3,
    NATAC_K_OCC_SMOOTH = 4,
    NATAC_K_OCC_FILL = 5,
    NATAC_K_INS = 6,
    NATAC_K_CAND = 7,
    NATAC_K_SIZE_HIST = 8,   /* insert-size histogram of natac_fragment_sizes */
    NATAC_K_INS_SMOOTH = 9,  /* natac_run_ins_smooth */
    NATAC_K_CENTER_COV = 10, /* natac_run_center_cov */
    NATAC_K_PWM_TRACK = 11,  /* natac_run_pwm_track */
    NATAC_K_COUNT = 12
};

typedef struct natac_ctx natac_ctx;
typedef struct natac_batch natac_batch;

/* ---- library / context ---------------------------------------------------------------- */
int natac_abi_version(void);
const char *natac_last_error(void);
int natac_device_count(int *count);
int natac_ctx_create(int device_id, natac_ctx **out);
void natac_ctx_destroy(natac_ctx *ctx);
int natac_ctx_sync(natac_ctx *ctx);
/* device name, CU count, global memory bytes of the context's device */
int natac_ctx_device_info(natac_ctx *ctx, char *name, size_t name_len, int *n_cu, size_t *mem_bytes);
/* which physical GPU the context computes on: the HIP device ordinal and its PCI bus id ("0000:05:00.0"); the multi-rank drivers
 * print both per rank and check that ranks meant to own a GPU each really do */
int natac_ctx_device_ids(natac_ctx *ctx, int *hip_device, char *pci_bus_id, size_t pci_len);

/* ---- run-level constants --------------------------------------------------------------- */
/* The three setters below may be called again at any time on a context that has run, with batches alive.  They wait for the
 * context's stream.  Two rules hold afterwards (tests/test_gpu_model_changes.py):
 *
 * A. Re-run equivalence.  After any sequence of natac_set_vmat, natac_set_sizes, natac_set_occ_model and changes of smooth_sd, a
 *    stage run on a live batch gives bit for bit what a fresh context and a fresh batch give for the same model and the same order
 *    of calls: tracks, grids, status words, peaks and statistics.  Everything the context and the batch keep between calls is a
 *    table derived from the model or from the batch's geometry, keyed on what it was derived from.  Each stage owns one bit of
 *    the status words and drops it before it launches (natac_batch_status), so a bit never outlives the run that raised it.
 *
 * B. No silent mixing.  A call that combines what an earlier stage left on the batch with the context's model takes the context's
 *    values and requires the geometry the stage ran with; it fails with NATAC_E_STATE, before any device work, when the geometry
 *    differs.  Setting a model of the same geometry again between a stage and its consumers is always allowed.
 *      natac_run_candidates, natac_run_candidates_cov, natac_run_peaks: the V-plot's (lower, upper, w) must be natac_run_nuc's.
 *        The template, the sizes and hence the statistics are those of the model that is set now.
 *      NATAC_T_OCC_PREFILL while it is still to be formed (any reader: download, track_ptr, format_track, natac_store_adopt) and
 *        natac_run_occ_peaks: (step, flank, upper) must be natac_run_occ's; the alpha grid, the cutoff and the probabilities may
 *        differ, none of these reads them.
 *    Tracks that are already formed (NATAC_T_BACKGROUND included: it is formed from what natac_run_nuc left, not from the model),
 *    the grids and the peaks of an earlier search stay readable as the run left them.  Outputs that only natac_batch_set_track
 *    wrote carry no geometry.  After a refusal, running the stage again is all it takes. */
/* VMat template (pyatac/VMat.py:24-37): mat[(upper-lower) x (2w+1)] row-major, insert sizes [lower,upper). */
int natac_set_vmat(natac_ctx *ctx, const double *mat, int lower, int upper, int w);
/* global insert-size distribution over [0, upper) used by BiasMat2D.normByInsertDist (chunkmat2d.py:154-156). */
int natac_set_sizes(natac_ctx *ctx, const double *sizes, int upper);
/* OccupancyCalcParams + OccupancyParameters (Occupancy.py:89-102, 175-193): nuc_probs / nfr_probs over
 * [0, upper) (already normalised), the alpha grid (np.linspace(0,1,101)), the chi2 cutoff, step (odd), flank.
 * With a model that has an nfr_prob of 0, a grid whose smallest positive alpha is below 2^-500 is refused (NATAC_E_ARG): the product
 * alpha * probability of such a size could leave the fp64 range. */
int natac_set_occ_model(natac_ctx *ctx, const double *nuc_probs, const double *nfr_probs, int upper,
                        const double *alphas, int n_alpha, double cutoff, int step, int flank);
/* Which occupancy kernels the model of the last natac_set_occ_model takes (reads context fields, launches nothing).  *fast: 1 when the
 * block-sum kernels natac_occ_gsum / natac_occ_decide run (the model qualifies and NATAC_OCC_GENERAL does not force natac_occ_mle), else 0;
 * *rn: factors between two renormalisations in natac_occ_decide, 16 or 4, 0 when not fast; *zero_flags: the flags word natac_occ_decide
 * gets (bit 0: some nuc_prob == 0, bit 1: some nfr_prob == 0 and the fast path treats such sizes).  Tests use it to assert that a model
 * reaches the arm they are written for. */
int natac_ctx_occ_route(natac_ctx *ctx, int32_t *fast, int32_t *rn, int32_t *zero_flags);

/* ---- batches of packed chunks ---------------------------------------------------------- */
/* Upload one batch (layout: nucleoatac_amd/packing.py).  bias_off/bias_log may be NULL (no FASTA: bias
 * matrix of ones, NucleosomeCalling.py:243-250).  bias_log covers [start-bias_left, end+bias_right). */
int natac_batch_create(natac_ctx *ctx, int32_t n_chunks, const int32_t *chunk_len, const int64_t *frag_off,
                       const int32_t *frag_lpos, const int32_t *frag_ilen, const int64_t *bias_off,
                       const double *bias_log, int32_t bias_left, int32_t bias_right, natac_batch **out);
/* The same batch with the Tn5 bias scored ON THE DEVICE from the genome sequence (InsertionBiasTrack.computeBias, pyatac/bias.py:85-92, as
 * the reference calls it per chunk, Occupancy.py:212-214 / NucleosomeCalling.py:246-248): seq[seq_off[i] .. seq_off[i+1]) = the upper-case
 * bases of [start - bias_left - up, end + bias_right + down) of chunk i (up + down + 1 = K, the PWM width); log_pwm[nrow x K] = log(PWM.mat),
 * nucleotides[nrow] its row letters (natac_pwm_bias).  One byte per base crosses PCIe instead of a float64 score down and up again. */
int natac_batch_create_from_seq(natac_ctx *ctx, int32_t n_chunks, const int32_t *chunk_len, const int64_t *frag_off,
                                const int32_t *frag_lpos, const int32_t *frag_ilen, const int64_t *seq_off, const uint8_t *seq,
                                const double *log_pwm, const uint8_t *nucleotides, int nrow, int K, int32_t bias_left,
                                int32_t bias_right, natac_batch **out);
void natac_batch_free(natac_batch *b);
int natac_batch_info(natac_batch *b, int64_t *total_bp, int64_t *total_grid, int64_t *n_frags);
/* How the background stage (NucleosomeCalling.py:49-64, the dense correlation of the bias matrix with the V-plot) tiles a chunk of
 * chunk_len bases with the V-plot that is set: n_tiles 512-point transforms per row pair, of which the first `extended` yield 16 more
 * outputs on each side (finished by an edge pass; chosen where that saves whole tiles).  0 tiles = the FFT path does not apply to
 * this V-plot (direct summation).  A function of the chunk's length and the model alone. */
int natac_bg_tiling(natac_ctx *ctx, int32_t chunk_len, int32_t *n_tiles, int32_t *extended);
/* Drop every output of the batch (per-base tracks, grid arrays, candidate / peak arrays) but keep its packed inputs resident:
 * for workloads whose outputs do not fit in HBM all at once (BASELINE configs[3] on one GPU: 3 Gbp x ~160 B/bp); the blocks go
 * back to the library's pool and are reused by the next batch's stages. */
int natac_batch_release_outputs(natac_batch *b);

/* NucChunk.process up to smoothSignal (NucleosomeCalling.py:328-334): fills NUC_COV, NFR_COV, RAW,
 * BACKGROUND, NORM, SMOOTH.  smooth_sd = NucParameters.smooth_sd (cli default 10).  Asynchronous. */
int natac_run_nuc(natac_batch *b, double smooth_sd);
/* OccChunk.process up to getCov + the call_peaks NaN fill (Occupancy.py:241-247): fills the grid arrays,
 * OCC, OCC_LOWER, OCC_UPPER, OCC_COV (OCC_PREFILL, the smoothed occupancy before the fill, on request).  Asynchronous. */
int natac_run_occ(natac_batch *b);
/* InsertionTrack.calculateInsertions (pyatac/tracks.py:164-168) for every chunk: fills INS. */
int natac_run_ins(natac_batch *b, int lower, int upper);
/* `pyatac ins --smooth S` for every chunk (_insHelperSmooth, pyatac/get_ins.py:20-32): the insertions of [start - h, end + h), h = M / 2,
 * (both ends of every fragment with lower <= ilen < upper; ends outside the chromosome count like any other) smoothed by
 * utils.smooth(..., window = "gaussian", mode = "valid", norm = True), pyatac/utils.py:23-52.  w[M] = scipy's gaussian(M, (M - 1) / 6.0)
 * with M = S, or S + 1 when S is even (M odd, 1 <= M <= 4001); wsum = the window's 'valid' normaliser np.convolve(w, ones(M),
 * 'valid')[0].  Every value is the fp64 sum of w[j] * count[x - h + j] divided by wsum.  The packing margin must hold every fragment
 * with an end within h of a chunk.  Fills INS_SMOOTH.  Synchronous. */
int natac_run_ins_smooth(natac_batch *b, int lower, int upper, const double *w, int M, double wsum);
/* `pyatac cov` for every chunk (_covHelper, pyatac/get_cov.py:21-37, CoverageTrack.calculateCoverage, tracks.py:209-222): the number of
 * fragment centres l + (ilen - 1) // 2 with lower <= ilen < upper within W / 2 of every base (the flat window of W taps, W + 1 when W is
 * even), times mult = scale / float(W), one fp64 multiply of an exact count.  1 <= W <= 4001.  The packing margin must hold every
 * fragment centred within W / 2 of a chunk.  Fills CENTER_COV.  Asynchronous. */
int natac_run_center_cov(natac_batch *b, int lower, int upper, int W, double mult);
/* `pyatac bias` for every chunk (InsertionBiasTrack.computeBias, pyatac/bias.py:85-92, after its slop and before its trim): value x of
 * chunk i is the sum over k < K of log_pwm[row(base x + k), k], where seq[seq_off[i] .. seq_off[i + 1]) holds the chunk_len[i] + K - 1
 * bases under the chunk's track (host memory; raw FASTA bytes: lower case counts as upper case, a base that is none of the row letters
 * adds 0).  log_pwm[nrow x K] = log(PWM.mat), nucleotides[nrow] its row letters, all different; nrow <= 255, nrow * K <= 4096.  Per row
 * a running sum over k, rows added in order: bit-identical to natac_pwm_bias on the same (upper-case) bases.  The batch needs no
 * fragments.  seq_off[0] != 0, a window of another length, K < 1, nrow < 1, a table entry that is not finite: NATAC_E_ARG and nothing
 * is launched.  Fills BIAS.  Synchronous. */
int natac_run_pwm_track(natac_batch *b, const int64_t *seq_off, const uint8_t *seq, const double *log_pwm, const uint8_t *nucleotides,
                        int nrow, int K);
/* Per-candidate statistics (needs natac_run_nuc first).  cand_chunk[k] = chunk index, cand_pos[k] = position
 * relative to the chunk start.  Outputs (host, length n_cand):
 *   lr   Nucleosome.getLR       NucleosomeCalling.py:110-122
 *   var  calculateCov closed form r*(sum p v^2 - (sum p v)^2), r = int(nuc_cov[pos])  multinomial_cov.pyx:20-31
 *   z    Nucleosome.getZScore   NucleosomeCalling.py:123-127   (norm_signal / sqrt(var)) */
int natac_run_candidates(natac_batch *b, int64_t n_cand, const int32_t *cand_chunk, const int32_t *cand_pos,
                         double *lr, double *var, double *z);
/* calculateCov (nucleoatac/multinomial_cov.pyx:20-31) at MANY candidates of the batch at once, in one of three arithmetic variants
 * (BASELINE configs[4]: "fp64 multinomial_cov path, tolerance sweep"; needs natac_run_nuc first).  Candidate k's probability
 * vector is SignalDistribution's p = B window / sum (NucleosomeCalling.py:70-76), v = the V-plot, r = int(nuc_cov[pos]) (:125).
 * mode 0 = closed form r (sum p v^2 - (sum p v)^2) in fp64 -- what natac_run_candidates reports; mode 1 = the .pyx's literal
 * O(N^2) pair sum in fp64; mode 2 = the closed form evaluated in fp32.  var[n_cand] on the host.
 * r is defined for every double a NUC_COV track can hold (natac_batch_set_track): the value truncated towards zero (0.99 and -0.5
 * give 0 and var = +0, 7.9 gives 7, -1.5 gives -1), saturated at INT_MIN / INT_MAX beyond the range of `int` (3e9 counts as
 * 2147483647), and a NaN coverage gives a NaN variance.  natac_run_candidates and natac_run_peaks form their var with the same r.
 * Only NUC_COV is read of the batch: with a bias track whose margins are shorter than natac_run_nuc asks for, exp(bias) counts as 0
 * outside the track (a window that lies outside it altogether gives NaN). */
int natac_run_candidates_cov(natac_batch *b, int64_t n_cand, const int32_t *cand_chunk, const int32_t *cand_pos, int mode,
                             double *var);
/* Candidate search + statistics entirely on the device (needs natac_run_nuc first):
 * utils.call_peaks(norm + smoothed, min_signal, sep, boundary, order) exactly as NucChunk.findAllNucs calls it
 * (nucleoatac/NucleosomeCalling.py:297-301, pyatac/utils.py:56-102), followed by LR / variance / z for every candidate.
 * jitter[n_jitter] is the reference's tie-break stream np.random.RandomState(25).uniform(0, 1e-12, n) generated by the
 * host (n_jitter >= longest chunk).  *n_cand receives the number of candidates (chunk order, ascending position);
 * fetch them with natac_download_peaks.  Batches whose longest chunk has at most 16,384 bases: a
 * chunk with more than 2,048 local maxima sets status bit 1 (list truncated; the drivers redo those chunks with utils.call_peaks on the
 * host).  Longer chunks (merged windows of tens of kb to Mb) keep their lists in device memory: no limit. */
int natac_run_peaks(natac_batch *b, double min_signal, int sep, int boundary, int order, const double *jitter,
                    int64_t n_jitter, int64_t *n_cand);
int natac_download_peaks(natac_batch *b, int64_t n_cand, int32_t *cand_chunk, int32_t *cand_pos, double *lr, double *var,
                         double *z);
/* The same peak search on ONE per-base track (no candidate statistics): utils.call_peaks(track, min_signal, sep, boundary,
 * order), e.g. OccChunk.callPeaks on NATAC_T_OCC (nucleoatac/Occupancy.py:225-231: sep = nuc_sep, min_signal = min_occ,
 * boundary = sep/2, order = 1).  Fetch positions with natac_download_peaks (lr / var / z may be NULL). */
int natac_run_track_peaks(natac_batch *b, int track, double min_signal, int sep, int boundary, int order,
                          const double *jitter, int64_t n_jitter, int64_t *n_peaks);
/* How the three searches above launch for a batch whose longest chunk has max_len bases (host only: no context, no GPU needed).
 * *kernel: 0 = a register variant natac_peaks_chunk_reg<*nj, *bt>, 1 = the segmented natac_peaks_chunk (*bt 256, *nj 0, *mask -1);
 * *mask: where the register variant keeps its row masks, 0 = registers, 1 = LDS with a two-phase survivor list, 2 = LDS, direct
 * test; *global_lists: the segmented kernel keeps the lists of its long chunks in device memory; *forms_smooth: natac_run_peaks
 * forms a pending NATAC_T_SMOOTH itself; *pk_cap: maxima per chunk held in LDS; lds_bytes[2]: dynamic LDS without / with that
 * smoothing.  NATAC_E_ARG for max_len < 1 or an order outside 1..255. */
int natac_peaks_plan(int32_t max_len, int32_t order, int32_t *kernel, int32_t *bt, int32_t *nj, int32_t *mask,
                     int32_t *global_lists, int32_t *forms_smooth, int32_t *pk_cap, int64_t *lds_bytes);
/* OccChunk.callPeaks + OccChunk.getNucDist for every chunk on the device (nucleoatac/Occupancy.py:225-240; needs natac_run_occ):
 * call_peaks(smoothed_vals, sep, min_signal = min_occ) as natac_run_track_peaks(NATAC_T_OCC, ...) does it, then per peak the
 * OccPeak values (occ, lower, upper, reads = cov) and keep = (lower > min_occ && reads > 0), and per chunk
 * nuc_dist[upper] = sum over its kept peaks of the window's insert-size histogram / its total, in peak order.  `jitter` as in
 * natac_run_peaks.  *n_peaks = number of call_peaks peaks (kept or not). */
int natac_run_occ_peaks(natac_batch *b, double min_occ, int sep, const double *jitter, int64_t n_jitter, int64_t *n_peaks);
int natac_download_occ_peaks(natac_batch *b, int64_t n_peaks, int32_t *chunk, int32_t *pos, double *occ, double *lower,
                             double *upper, double *reads, int32_t *keep);
/* float64[n_chunks x upper] (upper of natac_set_occ_model), row i = OccChunk.getNucDist() of chunk i */
int natac_download_nuc_dist(natac_batch *b, double *dst, size_t dst_bytes);
/* copy one per-base track to host (float64[total_bp], or int32[total_bp] for NATAC_T_INS). Synchronises. */
int natac_batch_download(natac_batch *b, int track, void *dst, size_t dst_bytes);
/* copy one per-grid-point array to host (float64[total_grid]). */
int natac_batch_download_grid(natac_batch *b, int which, double *dst, size_t dst_bytes);
/* overwrite one float64 per-base track of the batch with host values (total_bp doubles, chunk order): lets any track -- an
 * externally computed one, or a test pattern -- go through the device-side writer (natac_batch_format_track).  Only `track`
 * becomes readable: calls that read other tracks or the grids still need their stage (NATAC_E_STATE), and so do the candidate
 * statistics of a batch with a bias track (natac_run_nuc forms exp(bias)).  Overwriting NUC_COV leaves the BACKGROUND
 * natac_run_nuc computed as it was; natac_run_occ then takes OCC_COV from the fragments, not from host-written coverage. */
int natac_batch_set_track(natac_batch *b, int track, const double *vals, size_t n);
/* per-chunk status flags (int32[n_chunks]; 0 = ok, bit0 = occupancy likelihood undefined at some grid point
 * -- the reference would raise ValueError at Occupancy.py:118 --, bit1 = a peak search truncated the chunk's list of maxima).
 * Bit 0 is natac_run_occ's and describes its last run; bit 1 describes the last peak search (natac_run_peaks,
 * natac_run_track_peaks, natac_run_occ_peaks): each drops its bit for every chunk before it launches and leaves the other alone.
 * natac_batch_release_outputs clears both. */
int natac_batch_status(natac_batch *b, int32_t *dst, size_t dst_bytes);
/* raw device pointer of a per-base track (for zero-copy consumers); NULL if the track holds nothing (NATAC_E_STATE above). */
int natac_batch_track_ptr(natac_batch *b, int track, void **dptr);

/* ---- drop-in replacements of the Cython functions (host buffers in / out, synchronous) --- */
/* n_frags < 0 is refused (NATAC_E_ARG, "negative size") before any device work by the four fragment calls below; an insert size may
 * be zero or negative wherever [lower, upper) admits it (its right end is l + n - 1, its centre l + floor((n - 1) / 2)). */
/* makeFragmentMat, pyatac/fragments.pyx:17-40: mat[(upper-lower) x (end-start)] float64, zeroed + filled. */
int natac_make_fragment_mat(natac_ctx *ctx, int64_t n_frags, const int64_t *l, const int32_t *n, int64_t start,
                            int64_t end, int lower, int upper, double *mat);
/* getInsertions, pyatac/fragments.pyx:43-67: out[end-start] float64. */
int natac_get_insertions(natac_ctx *ctx, int64_t n_frags, const int64_t *l, const int32_t *n, int64_t start,
                         int64_t end, int lower, int upper, double *out);
/* getStrandedInsertions, pyatac/fragments.pyx:71-97: plus[end-start] = insertions at left fragment ends, minus[end-start] = at
 * right fragment ends (plus + minus == natac_get_insertions). */
int natac_get_stranded_insertions(natac_ctx *ctx, int64_t n_frags, const int64_t *l, const int32_t *n, int64_t start,
                                  int64_t end, int lower, int upper, double *plus, double *minus);
/* getFragmentSizesFromChunkList, pyatac/fragments.pyx:123-145 (one chromosome's fragments, its chunks):
 * sizes[upper-lower] float64 counts (not normalised).  lower may be negative: a size in [lower, 0) is counted into bin size - lower
 * like any other.  At most 1 << 20 bins. */
int natac_fragment_sizes(natac_ctx *ctx, int64_t n_frags, const int64_t *l, const int32_t *n, int32_t n_chunks,
                         const int64_t *chunk_start, const int64_t *chunk_end, int lower, int upper, double *sizes);
/* calculateCov, nucleoatac/multinomial_cov.pyx:20-31.  mode 0 = closed form O(N), mode 1 = literal O(N^2)
 * pair sum (same terms as the .pyx, tree-reduced).  r is truncated to int like the .pyx signature. */
int natac_calculate_cov(natac_ctx *ctx, const double *p, const double *v, int64_t n, int r, int mode, double *out);

/* ---- operator-level entry points behind the Track / BiasMat2D / bias / occupancy classes ------ */
/* utils.smooth, pyatac/utils.py:23-52, on one host array.  w[M] is the window (ones for 'flat', scipy's
 * gaussian(M, sd) otherwise; M odd).  mode 0 = 'valid' (out[n-M+1]), 1 = 'same' (out[n], needs n >= M).
 * norm != 0: NaN-aware normalisation (0 weight -> NaN).  Orientation: np.convolve(w, x), so out[t] = sum_k w[k] * x[t + M-1 - k]
 * ('valid'; 'same' has (M-1)/2 in place of M-1 and skips taps outside x): w[0] meets the rightmost value under the window.  An even M
 * and n < M are refused (NATAC_E_ARG). */
int natac_smooth(natac_ctx *ctx, const double *x, int64_t n, const double *w, int M, int mode, int norm, double *out);
/* BiasMat2D.makeBiasMat, pyatac/chunkmat2d.py:140-153 (log-scale track): mat[(upper-lower) x (end-start)].
 * bias_log[nb] starts at genomic coordinate track_start; returns NATAC_E_ARG if the track does not cover every cell that a row
 * i in [lower, upper) reads, start + x - (i-1)//2 and start + x + i//2 (the message names the sufficient [start - upper//2,
 * end + upper//2)).  nb < 0 is refused ("negative size") before any device work. */
int natac_make_bias_mat(natac_ctx *ctx, const double *bias_log, int64_t nb, int64_t track_start, int64_t start,
                        int64_t end, int lower, int upper, double *mat);
/* InsertionBiasTrack.computeBias, pyatac/bias.py:85-92: seq[n] (upper-case ASCII) covers [start-up, end+down);
 * log_pwm[nrow x K] = log(PWM.mat), nucleotides[nrow] the PWM's row letters; out[n-K+1]. */
int natac_pwm_bias(natac_ctx *ctx, const uint8_t *seq, int64_t n, const double *log_pwm, const uint8_t *nucleotides,
                   int nrow, int K, double *out);
/* _pwmHelper, pyatac/get_pwm.py:21-40, with InsertionTrack.calculateInsertions + getInsertionSequences (sym != 0) or
 * calculateStrandedInsertions + getStrandedInsertionSequences (sym == 0), pyatac/tracks.py:164-201 and fragments.pyx:43-97, summed over
 * a packed chunk list: chunk_len / frag_off / frag_lpos / frag_ilen as natac_pack_chunks gives them (lpos relative to the chunk start,
 * ATAC shift applied), seq[seq_off[k] .. seq_off[k+1]) = the upper-case bases of [start_k - flank, end_k + flank) (K - 1 more than the
 * chunk).  A fragment counts if lower <= ilen < upper; its ends l and l + ilen - 1 each count if they lie in the chunk.  counts[4 x K]
 * (rows A C G T, K = 2*flank + 1, other bases in no row) and n_ins = the number of counted ends are exact int64 sums, overwritten.
 * flank in [0, 1000].  kernel_ms (may be NULL): device time of the counting kernel alone. */
int natac_insertion_seq_counts(natac_ctx *ctx, int32_t n_chunks, const int32_t *chunk_len, const int64_t *frag_off, const int32_t *frag_lpos,
                               const int32_t *frag_ilen, const int64_t *seq_off, const uint8_t *seq, int flank, int lower, int upper, int sym,
                               int64_t *counts, int64_t *n_ins, double *kernel_ms);
/* the numerators of seq.getNucFreqs / getNucFreqsFromChunkList, pyatac/seq.py:47-72: counts[4] = the A, C, G, T bases (upper or lower
 * case) of seq[start[i] .. end[i]) summed over the n_ranges ranges, int64, overwritten; overlapping ranges count once per range. */
int natac_base_counts(natac_ctx *ctx, const uint8_t *seq, int64_t n, int32_t n_ranges, const int64_t *start, const int64_t *end,
                      int64_t *counts);
/* the per-range form of natac_base_counts, by the same rule: counts[n_ranges x 4] = the A, C, G, T bases (upper or lower case) of
 * seq[start[i] .. end[i]) for every range on its own, int64, overwritten; 0 <= start[i] <= end[i] <= n (NATAC_E_ARG names the range);
 * ranges may overlap, repeat, be empty and come in any order. */
int natac_window_base_counts(natac_ctx *ctx, const uint8_t *seq, int64_t n, int64_t n_ranges, const int64_t *start, const int64_t *end,
                             int64_t *counts);
/* get_counts, pyatac/get_counts.py:30-45, for the regions of one chromosome: pos[n_frags] (non-decreasing) and tlen[n_frags] are the
 * chromosome's forward proper-pair records as the FragmentStore holds them.  A record is the fragment l = pos + 4, ilen = tlen - 8
 * (atac != 0) or l = pos, ilen = tlen (atac == 0), r = l + ilen - 1, and counts for region i if lower <= ilen < upper and
 * (start[i] <= l < end[i] or start[i] <= r < end[i]); ilen == 0 gives r = l - 1 and counts by the same rule.  EVERY record is a
 * candidate: the reference's fetch(chrom, start - upper, end + upper) is a superset filter that only drops such a fragment when its
 * read is shorter than 3 bases, and the store keeps no read lengths.  Regions may overlap, repeat and come in any order; each is
 * counted on its own, end[i] >= start[i].  counts[n_regions] are exact int64, overwritten.  kernel_ms (may be NULL): device time of the
 * range search and the counting kernels. */
int natac_region_counts(natac_ctx *ctx, int64_t n_frags, const int64_t *pos, const int64_t *tlen, int64_t n_regions, const int64_t *start,
                        const int64_t *end, int lower, int upper, int atac, int64_t *counts, double *kernel_ms);
/* ---- the cell-by-region count matrix of one chromosome (this library's own; `pyatac cellcounts`) ----
 * pos / tlen as natac_region_counts takes them, cell[n_frags] in [0, n_cells) the cell of every record (natac_bam_ref_cells), n_cells in
 * [1, NATAC_SPLIT_MAX_BARCODES].  A record counts for a region EXACTLY by natac_region_counts' rule.  The result is CSR with one row per
 * region, in the given order: row_ptr[n_regions + 1] is always written; within a row col (the cell index) is strictly ascending and val
 * is the number of counting records of that cell, exact.  col == val == NULL with cap == 0 is a sizing call that writes row_ptr only;
 * otherwise cap >= row_ptr[n_regions] entries of col and val must exist, and a smaller cap returns NATAC_E_ARG with col and val untouched
 * (the sum of natac_region_counts bounds nnz, and so does the number of candidate records).  A row of more than 2^31 - 1 counting records
 * is refused (NATAC_E_ARG).  The operands are checked on the host (NATAC_E_ARG names the record or region): pos non-decreasing, cell in
 * range, end >= start.  n_regions == 0 or n_frags == 0 gives zeros and launches nothing.  Only integer atomics: the result is a pure
 * function of the inputs.  Rows go by their number of counting records h (csrc/natac_cellcounts.hpp): h <= NATAC_CELLCOUNT_WAVE_MAX is
 * sorted in the registers of one wave, h <= NATAC_CELLCOUNT_SHORT_MAX in the LDS of one workgroup, a longer row is counted into a dense
 * array of n_cells counters, one such row at a time.  kernel_ms (may be NULL): device time of all kernels of the call. */
#define NATAC_CELLCOUNT_WAVE_MAX 64
#define NATAC_CELLCOUNT_SHORT_MAX 4096
int natac_region_cell_counts(natac_ctx *ctx, int64_t n_frags, const int64_t *pos, const int64_t *tlen, const int32_t *cell, int32_t n_cells,
                             int64_t n_regions, const int64_t *start, const int64_t *end, int lower, int upper, int atac, int64_t *row_ptr,
                             int64_t cap, int32_t *col, int32_t *val, double *kernel_ms);
/* ---- per-cell TSS counts, the aggregate TSS profile and per-cell fragments in peaks of one chromosome (this library's own; `pyatac
 * cellqc`) ----
 * pos / tlen / cell / n_cells as natac_region_cell_counts takes them.  A record is the fragment l = pos + 4, ilen = tlen - 8,
 * r = l + ilen - 1 (the ATAC offsets of natac_region_counts).  EVERY record counts: there is no size filter.  Its two insertions are l and
 * r; ilen == 0 gives r = l - 1, ilen == 1 gives r == l, a negative ilen gives r < l - 1, and in all these cases both insertions count on
 * their own.
 *   Sites: site_center[n_sites] ascending (equal centres are separate sites), site_minus[i] != 0 a minus-strand site (NULL: all plus).  For
 *   an insertion x and a site (c, minus) let d = x - c, or c - x for a minus site.  When |d| <= flank the pair adds 1 to profile[d + flank],
 *   1 to tss_center[cell] if |d| <= center, and 1 to tss_flank[cell] if |d| > flank - edge.
 *   Peaks: [peak_start[j], peak_end[j]) disjoint and ascending (peak_end[j] >= peak_start[j], peak_start[j] >= peak_end[j - 1]: touching
 *   intervals are fine).  A record is in peaks if l or r lies in some interval; it adds 1 to in_peaks[cell], once.
 * tss_center / tss_flank / in_peaks [n_cells] and profile [2 * flank + 1] are exact int64, overwritten.  Only integer atomics are used: the
 * result is a pure function of the inputs, and the sum over any split of the sites, of the records or of the chromosomes into calls equals
 * the single call.  0 <= center, 1 <= edge, center + edge <= flank, 1 <= flank <= NATAC_CELLQC_MAX_FLANK.  The operands are checked on the
 * host (NATAC_E_ARG names the offending index, the outputs stay untouched): the flank / center / edge rule, pos non-decreasing, cell in
 * range, centres ascending, peaks disjoint.  n_sites == 0 skips the site part, n_peaks == 0 the peak part; with no records, or with neither
 * sites nor peaks, the results are zeros, nothing is launched and kernel_ms is 0.
 * The kernel (csrc/natac_cellqc.hpp) takes NATAC_CELLQC_BLOCK records per workgroup and step, one per thread.  The per-cell counts come
 * from bounds searched in site_center (the three classes are symmetric in d); the profile needs the pairs and is kept per workgroup as
 * 2 * flank + 1 32-bit counters in LDS: an insertion with at most NATAC_CELLQC_LANE_MAX sites in reach is walked by its lane, one with
 * more by its wave.  NATAC_CELLQC_MAX_FLANK rests on the LDS of a gfx950 CU: 5,001 counters are 20,004 bytes, so eight workgroups of four
 * waves -- the 32 waves a CU can hold -- fit its 160 KiB.  A workgroup adds at most 2 * NATAC_CELLQC_BLOCK * n_sites pairs per step, and it
 * flushes its counters into profile (64-bit atomics) every floor((2^32 - 1) / (2 * NATAC_CELLQC_BLOCK * n_sites)) steps, before one can
 * wrap; more than NATAC_CELLQC_SITE_CHUNK sites go through several launches, the peaks with the first.  A launch has at most
 * NATAC_CELLQC_MAX_BLOCKS workgroups: past NATAC_CELLQC_MAX_BLOCKS * NATAC_CELLQC_BLOCK records a workgroup takes further steps with its
 * counters carried over.  kernel_ms (may be NULL): device time of the kernels of the call; like the other outputs it is written only
 * behind the checks. */
#define NATAC_CELLQC_MAX_FLANK 2500
#define NATAC_CELLQC_BLOCK 256
#define NATAC_CELLQC_LANE_MAX 8
#define NATAC_CELLQC_MAX_BLOCKS 2048
#define NATAC_CELLQC_SITE_CHUNK 4194304
int natac_cell_site_qc(natac_ctx *ctx, int64_t n_frags, const int64_t *pos, const int64_t *tlen, const int32_t *cell, int32_t n_cells,
                       int64_t n_sites, const int64_t *site_center, const uint8_t *site_minus, int flank, int center, int edge,
                       int64_t n_peaks, const int64_t *peak_start, const int64_t *peak_end, int64_t *tss_center, int64_t *tss_flank,
                       int64_t *in_peaks, int64_t *profile, double *kernel_ms);
/* ---- the enriched regions of one chromosome (this library's own; `pyatac peaks`) ----
 * pos / tlen as natac_region_counts takes them (pos non-decreasing), chrom_len = n the chromosome's length.  EVERY record gives two
 * insertions, l = pos + 4 and r = pos + tlen - 5; there is no size filter; an insertion outside [0, n) is dropped on its own.  ins[x] is the
 * number of insertions at base x and C_w(x) the sum of ins[y] over |y - x| <= w, 0 <= y < n (the window is clipped at the ends).
 *   p(x) = C_half_width(x), s(x) = C_small(x), g(x) = C_large(x), 1 <= half_width <= small <= large <= NATAC_PEAKS_MAX_WINDOW.
 *   Base x is significant when p(x) >= min_pileup, s(x) <= thr_small[k] and g(x) <= thr_large[k], k = min(p(x), n_table - 1): the two
 *   int32 tables [n_table >= 2] and min_pileup >= 1 are all the statistics the device sees (the caller derives them from Poisson critical
 *   values; a negative entry admits nothing).
 *   Significant bases with at most max_gap >= 0 others between them are one region [first significant base, last + 1); a region shorter
 *   than min_length >= 1 is dropped.  summit = (a + b) / 2 with a / b the first / last base of the region where p is largest.
 * Per kept region, ascending: start, end, summit, pileup = p(summit), n_small = s(summit), n_large = g(summit).  *n_regions = the number
 * of kept regions; if that is more than capacity, the six arrays stay as they were and the caller comes again with room (nothing is ever
 * cut short).  n_found (may be NULL) = the regions before the length rule, n_significant (may be NULL) = the significant bases.
 * Refused (NATAC_E_ARG, every output untouched): unsorted pos and the other findings of the fragment check, a parameter outside the rules
 * above, NULL tables, n_table < 2, chrom_len < 1 or >= 2^31, n_frags >= 2^30.  With no records nothing is launched and the counts are 0.
 * The chromosome is worked through in segments of NATAC_PEAKS_SEGMENT bases (environment; default NATAC_PEAKS_SEGMENT_DEFAULT) with
 * halos of `large` bases, 21 bytes of device memory per base of a segment; the result does not depend on the segment size (a region
 * across borders is joined by a carried last significant base and by 64-bit atomic maxima of packed (p, base) keys).  The first sweep has
 * room for NATAC_PEAKS_FIRST_CAPACITY region starts and is run again with the counted number if there are more.  A region's piece of at
 * most NATAC_PEAKS_SHORT_MAX bases in a segment is searched by one wave, a longer one by a workgroup.  Only integer arithmetic and integer
 * atomics run on the device: the result is a pure function of the inputs (csrc/natac_peakcall.hpp).  kernel_ms (may be NULL): device time
 * from the first to the last kernel of the call, the host's steps between the sweeps included; written only behind the checks. */
#define NATAC_PEAKS_MAX_WINDOW 50000
#define NATAC_PEAKS_SEGMENT_DEFAULT 4194304
#define NATAC_PEAKS_SHORT_MAX 2048
#define NATAC_PEAKS_FIRST_CAPACITY 4096
int natac_enriched_regions(natac_ctx *ctx, int64_t n_frags, const int64_t *pos, const int64_t *tlen, int64_t chrom_len, int half_width,
                           int small, int large, int max_gap, int min_length, int min_pileup, int32_t n_table, const int32_t *thr_small,
                           const int32_t *thr_large, int64_t *n_regions, int64_t capacity, int64_t *start, int64_t *end, int64_t *summit,
                           int32_t *pileup, int32_t *n_small, int32_t *n_large, int64_t *n_found, int64_t *n_significant,
                           double *kernel_ms);
/* ---- the sites of integer position weight matrices in one chromosome (this library's own; `pyatac motifs`) ----
 * seq[n] is the chromosome as natac_base_counts takes it: ASCII, case kept.  start[i] <= end[i] (0 <= start, end <= n) are the n_windows
 * windows: they may overlap, repeat and come in any order; windows that overlap or abut are merged into SCAN INTERVALS.
 * Motif m has widths[m] = W columns (1 <= W <= NATAC_MOTIF_MAX_WIDTH) of four int32 scores, base order A C G T = 0 1 2 3; the columns of
 * all motifs follow each other in scores[4 * sum of widths]: S_m[j][b] = scores[4 * (widths[0] + .. + widths[m - 1] + j) + b].
 * thresholds[m] = T is an int32.  The integers S and T are all the statistics the device sees (the caller derives them from counts, a
 * background and a p-value: nucleoatac_amd/pyatac/get_motifs.py; NATAC_MOTIF_SCALE is the scale of its log-odds, 0.01 bit a unit).
 *   Scoring: motif m is scored at x when [x, x + W) lies inside ONE scan interval and all W bases are one of ACGTacgt (lower case counts
 *   as upper case; N and the IUPAC codes leave the window unscored).  With code(.) the base's number,
 *     fwd = sum_j S[j][code(seq[x + j])],   rev = sum_j S[W - 1 - j][3 - code(seq[x + j])]   (the reverse complement read on the forward
 *   strand), both exact int32.  A `+` hit is fwd >= T, a `-` hit is rev >= T; both can occur at one x.
 *   Hits: four arrays, motif (int32), start = x (int64), strand (uint8, 0 = `+`, 1 = `-`), score (int32), sorted by (motif, start, strand)
 *   by the device -- the host never sorts them.  A site appears once however many windows cover it.  *n_hits is always written; if it is
 *   more than capacity, the four arrays stay as they were and the caller comes again with room (NATAC_MOTIF_FIRST_CAPACITY is the binding's
 *   first guess).
 *   Counts: counts[n_windows x n_motifs], int32, row-major, always written: entry (i, m) = the hits of motif m with start[i] <= x and
 *   x + W_m <= end[i], per window: a site inside two overlapping windows counts in both, a site across the border of two abutting windows
 *   is a hit and counts in neither.
 * Refused (NATAC_E_ARG, every output untouched): a width outside the limits, more than NATAC_MOTIF_MAX_MOTIFS motifs, a NULL pointer where a
 * size is positive, a window outside [0, n) or with end < start, n < 1 or n >= 2^31, a motif whose sums of column minima or maxima leave
 * int32.  With no windows or no motifs nothing is launched and the counts are zero.
 * The kernels (csrc/natac_motifs.hpp): the chromosome is packed once per call to 2 bits a base plus a validity bit.  A wave takes
 * NATAC_MOTIF_TILE window starts at a time, a lane each, and NATAC_MOTIF_RUN_TILES such tiles in a row (twice that, and again, where
 * motifs x runs would pass 2^27 counters; NATAC_MOTIF_MAX_COUNTERS in the environment sets a smaller bound: tests); the motifs are worked in groups of at most NATAC_MOTIF_GROUP whose tables (at most 32 KiB) lie in LDS.  Per motif
 * the host takes one of two accumulators: both strands in the halves of one dword, offset by the column minima, when
 * sum_j (max_b S[j][b] - min_b S[j][b]) <= 65535, else two int32 sums.  Hits are counted per (motif, run), the counts prefix-summed, and
 * the marked (tile, motif) pairs scored again into their places.  Only integer arithmetic, no atomics: two calls give the same bytes.
 * kernel_ms (may be NULL): device time from the first to the last kernel of the call; written only behind the checks. */
#define NATAC_MOTIF_MAX_WIDTH 64
#define NATAC_MOTIF_MAX_MOTIFS 4096
#define NATAC_MOTIF_SCALE 100
#define NATAC_MOTIF_TILE 64
#define NATAC_MOTIF_RUN_TILES 16
#define NATAC_MOTIF_GROUP 64
#define NATAC_MOTIF_FIRST_CAPACITY 4194304
int natac_motif_scan(natac_ctx *ctx, const uint8_t *seq, int64_t n, int64_t n_windows, const int64_t *start, const int64_t *end,
                     int32_t n_motifs, const int32_t *widths, const int32_t *scores, const int32_t *thresholds, int64_t *n_hits,
                     int64_t capacity, int32_t *hit_motif, int64_t *hit_start, uint8_t *hit_strand, int32_t *hit_score, int32_t *counts,
                     double *kernel_ms);
/* ---- the truncated SVD of the weighted cell-by-window matrix (this library's own; `pyatac cluster`) ----
 * The counts come as natac_region_cell_counts writes them: m rows (windows), n columns (cells), row_ptr[m + 1] non-decreasing with
 * row_ptr[0] >= 0 (the entries are col / count [row_ptr[0], row_ptr[m])), col strictly ascending within a row and in [0, n), count >= 1.
 * row_weight[m] and col_scale[n] are finite and >= 0; a weight of 0 drops the row, a scale of 0 the column.  X is cells x windows (n x m):
 * for an entry of count a in window w and cell c, a' = 1 if binarize else a, t = a' * col_scale[c] * row_weight[w], and
 * X[c, w] = t (transform 0, linear) or log1p(t * scale) (transform 1, log; scale finite and >= 0).  1 <= r <= NATAC_LSI_MAX_R, r at most
 * the number of live rows and of live columns (so m == 0 or n == 0 is refused), n_iter >= 1, q0[m * r] row-major and finite.
 *   1. Q = orth(q0), the rows of dropped windows zeroed first;  2. n_iter times: Y = orth(X Q), Q = orth(X^T Y);
 *   3. Y = X Q, G = Y^T Y = W diag(lam) W^T, lam descending;     4. sigma = sqrt(lam), U = Y W / sigma, V = Q W.
 * orth is CholeskyQR2: the r x r Gram matrix on the device, its Cholesky factor on the host, the triangular solve on the device, twice.
 * Step 3's eigenproblem is a cyclic Jacobi on the host.  Outputs: sigma[r], U[n * r], V[m * r] row-major; dropped rows and columns have
 * zero vectors.  The signs of the components are whatever the iteration leaves (Context.sparse_lsi fixes them).
 * *status = 1 with NATAC_OK: a Cholesky pivot was at most r * eps * the largest diagonal entry of its Gram matrix (or an eigenvalue of
 * step 3 was not positive) -- the matrix has fewer than r independent directions.  The outputs are then zeros, nothing has faulted and
 * the context is as usable as before.
 * *status = 2 with NATAC_OK: the operands' size took a Gram matrix out of fp64's range -- an entry of one was not finite (singular values
 * above about 1e154, or q0 that large), or its largest diagonal entry was so small that the pivot floor r * eps * max(diag) lay below
 * DBL_MIN (singular values below about 1e-146 / sqrt(r), or q0 that small: the pivots would sit among the denormals and lose bits without
 * falling under the floor), or the block was not zero and all its squares were.  The outputs are zeros as for status 1.  Inside that range
 * every step scales with the operands and every threshold is relative: a power of two in row_weight (linear transform), one moved between
 * col_scale and scale (log), or one in q0 scales sigma (or nothing) exactly and changes no bit of U and V.  *status = 0 otherwise.
 * The operands are checked on the host before any launch (NATAC_E_ARG): row_ptr, col, count as above, r and n_iter, transform, negative
 * or non-finite weights, scales, scale or q0, a null pointer where a size is positive.
 * Both products run through one sparse-times-block kernel family (csrc/natac_lsi.hpp); for X Q the entry point makes a cell-order copy of
 * the weighted entries once per call (the order by a stable counting sort on the host, integers only; the weighting on the device).  A
 * row of the sparse operand goes by its number of entries L: L <= NATAC_LSI_SHORT_MAX a lane group, L <= NATAC_LSI_WAVE_MAX a wave,
 * longer a workgroup.  Every sum has a fixed shape and there are no floating-point atomics: two calls give the same bytes.
 * kernel_ms (may be NULL): device time from the first to the last kernel of the call, the host's r x r steps in between included. */
#define NATAC_LSI_MAX_R 64
#define NATAC_LSI_SHORT_MAX 32
#define NATAC_LSI_WAVE_MAX 4096
int natac_sparse_lsi(natac_ctx *ctx, int64_t m, int64_t n, const int64_t *row_ptr, const int32_t *col, const int32_t *count,
                     const double *row_weight, const double *col_scale, double scale, int transform, int binarize, int r, int n_iter,
                     const double *q0, double *sigma, double *U, double *V, int32_t *status, double *kernel_ms);
/* ---- per-cell motif accessibility deviations against background window sets (this library's own; `pyatac deviations`) ----
 * The command's rule, whole.  X is the windows x cells count matrix of `pyatac cellcounts`, H the windows x motifs hit matrix of
 * `pyatac motifs` over the same windows; window p is annotated with motif m when H[p, m] > 0.  Windows with row sum 0 and cells with
 * column sum 0 are dropped, then motifs left without an annotated window; P windows and N cells stay.  rs[p] is a row sum, d[c] a
 * column sum, T the total, T < 2^31.  gc[p] = (C + G) / (A + C + G + T) of the window's bases (natac_window_base_counts), 0.5 for a
 * window with no such base.
 * Background table (host, integers out): from n_g GC bins and n_a accessibility bins, while P / (n_g n_a) (floored) is below min_bin and
 * n_g n_a > 1 the larger of the two is lowered by 1, n_a on a tie.  The windows ranked by (gc, index) are cut into GC bins, bin k the
 * ranks [floor(k P / n_g), floor((k + 1) P / n_g)); inside each GC bin the windows ranked by (rs, index) are cut into n_a parts in the
 * same way.  A window's candidates are the windows of its cell of that grid, itself included, in ascending index order; with
 * r = numpy.random.default_rng(seed).random((B, P)), bg[b][p] = candidates(p)[int(r[b - 1, p] * len(candidates(p)))] for b = 1 .. B, and
 * bg[0] is the identity.
 * Device, integers: for b = 0 .. B, motif m and cell c,  O_b[m, c] = sum over the annotated p of X[bg[b][p], c]  and
 * E_b[m] = sum over the annotated p of rs[bg[b][p]], both exact.
 * Device, fp64, one rounded operation at a time, no contraction:  x = double(E_b[m]) * double(d[c]) / double(T),
 * Y_b = (double(O_b[m, c]) - x) / x,  raw = Y_0, and over k = 1 .. B in that order  delta = Y_k - mean,  mean += delta / k,
 * M2 += delta * (Y_k - mean)  (Welford's recurrence from zeros).
 * Host: sd = sqrt(bg_m2 / (B - 1)), deviation = raw - bg_mean, z = deviation / sd or NaN where sd == 0; a motif's variability is the
 * standard deviation (n - 1) of z over the cells whose z is finite; with a group table, the mean z per group and motif.
 *
 * This entry is the device part.  Operands: the counts as natac_region_cell_counts writes them after the dropping, m = P windows and
 * n = N cells, under the CSR rules of natac_sparse_lsi (count >= 1), every window and every cell with at least one entry and the total
 * below 2^31; the motif sets motif-major, mot_ptr[n_motifs + 1] from 0 and mot_win[] strictly ascending inside a set, no set empty;
 * bg[n_bg x m] int32 row-major, the sets 1 .. B = n_bg (set 0 is implied), every value in [0, m); 2 <= n_bg <= NATAC_DEVIATIONS_MAX_B.
 * Outputs: raw, bg_mean, bg_m2, float64 [n_motifs x n] each.  obs / expect (both or neither; may be NULL) are a testing output:
 * O_b as int64 [(n_bg + 1) x n_motifs x n] and E_b as int64 [(n_bg + 1) x n_motifs]; refused when (n_bg + 1) n_motifs n exceeds
 * NATAC_DEVIATIONS_MAX_DEBUG.  Everything is checked on the host before any launch; a failure returns NATAC_E_ARG, names the index and
 * leaves the outputs untouched.  With n_motifs == 0 nothing is launched.
 * Kernel (csrc/natac_deviations.hpp): a workgroup owns one motif and one tile of cells and loops over b itself; it gathers the rows
 * bg[b][p] of X restricted to its tile (the entry splits every row by tile once per call) into integer counters in LDS with LDS atomics --
 * 32-bit, or 64-bit when the largest motif times the largest count reaches 2^32 -- sums rs in int64 by a wave reduction, and behind a
 * barrier turns the counters into Y_b and advances mean and M2, which stay in LDS over b.  The tile is NATAC_DEVIATIONS_TILE cells, halved
 * while motifs x tiles is below twice the compute units; the environment's NATAC_DEVIATIONS_CELL_TILE (1 .. NATAC_DEVIATIONS_TILE) forces
 * one, for the tests.  Every integer sum is exact, the order over b is sequential per element and there are no floating-point atomics: two
 * calls give the same bytes, whatever the tile.  kernel_ms (may be NULL): device time of the call's kernel. */
#define NATAC_DEVIATIONS_TILE 4096
#define NATAC_DEVIATIONS_MAX_B 1024
#define NATAC_DEVIATIONS_MAX_DEBUG 16777216
int natac_motif_deviations(natac_ctx *ctx, int64_t m, int64_t n, const int64_t *row_ptr, const int32_t *col, const int32_t *count,
                           int32_t n_motifs, const int64_t *mot_ptr, const int32_t *mot_win, int32_t n_bg, const int32_t *bg, double *raw,
                           double *bg_mean, double *bg_m2, int64_t *obs, int64_t *expect, double *kernel_ms);
/* How natac_motif_deviations launches for a matrix of m windows, n cells and nnz entries, n_motifs motifs the largest of max_set windows,
 * the largest count max_count, on a device of n_cu compute units (host only: no context, no GPU needed; it reads
 * NATAC_DEVIATIONS_CELL_TILE as the call does).  *tile: the cells of a workgroup -- the forced one, else NATAC_DEVIATIONS_TILE halved, down
 * to 256, while n_motifs x tiles is below 2 n_cu, then evened out over that number of tiles to a multiple of 64; *n_tiles =
 * ceil(n / *tile); *lanes: the lanes of a wave that share a row's piece inside a tile, the smallest power of two with
 * lanes * m * n_tiles >= nnz, at most 64; *wide: 1 = 64-bit counters (max_set * max_count >= 2^32), 0 = 32-bit; *lds_bytes: a workgroup's
 * dynamic LDS, *tile * (16 + (8 or 4)) + 128.  NATAC_E_ARG for a size below 1, for m, n, max_set or max_count of 2^31 or more, and where
 * the call refuses the shape: n_motifs * n_tiles >= 2^31 or m * (n_tiles + 1) > 2^33. */
int natac_motif_deviations_plan(int64_t m, int64_t n, int64_t nnz, int32_t n_motifs, int64_t max_set, int64_t max_count, int32_t n_cu,
                                int32_t *tile, int64_t *n_tiles, int32_t *lanes, int32_t *wide, int64_t *lds_bytes);
/* ---- rank-sum marker windows per cell group (this library's own; `pyatac markers`) ----
 * The command's rule, whole: a Wilcoxon rank-sum test of depth-normalised accessibility, one group against all other kept cells, for
 * every window and every group.
 * Cells and groups.  X is the windows x cells count matrix of `pyatac cellcounts`.  A cell is kept when the group table lists its
 * barcode and its column sum is positive; unlisted cells are in no group and not in "the rest" either.  N cells stay,
 * 2 <= N <= NATAC_MARKERS_MAX_CELLS.  d[c] is the kept cell's column sum over all windows, 1 <= d[c] < 2^31; grp[c] is in [0, G),
 * G <= NATAC_MARKERS_MAX_GROUPS, and n_g is the group's number of kept cells.  A group with n_g = 0 or n_g = N gets NA everywhere.
 * Values and ranks.  Window p has L entries (c, a) among the kept cells and z0 = N - L cells at value 0.  The value of an entry is the
 * exact rational a / d[c]; order and ties are decided by comparing a_i * d_j with a_j * d_i in 64-bit integers (both factors are below
 * 2^31, so no product overflows).  Midranks, with less_i / eq_i counted among the window's entries and eq_i including i itself: a zero
 * cell has 2 * rank = z0 + 1, an entry has 2 * rank_i = 2 z0 + 2 less_i + eq_i + 1.
 * Device outputs, exact integers.  detected[p, g] int32: the entries of group g.  total[p, g] int64: the sum of their counts.
 * rank2[p, g] int64 = (n_g - detected)(z0 + 1) + the sum over the group's entries of 2 rank_i.  ties[p] int64 = (z0^3 - z0) + the sum over
 * the entries of (eq_i^2 - 1), which is the sum over tie groups of (t^3 - t) without a sort.  An empty row is legal: rank2 = n_g (N + 1),
 * ties = N^3 - N.
 * Host, fp64, one window and group at a time, with n_r = N - n_g:  U = rank2 / 2 - n_g (n_g + 1) / 2,  mu = n_g n_r / 2,
 * var = n_g n_r / 12 * ((N + 1) - ties / (N (N - 1))),  z = (U - mu - 0.5 sign(U - mu)) / sqrt(var), NaN where var == 0,
 * p = min(1, 2 * norm.sf(|z|)) (scipy's asymptotic two-sided test with tie and continuity correction),  auc = U / (n_g n_r),
 * pct_in = detected / n_g,  pct_rest = (row detected - detected) / n_r,
 * log2fc = log2(((total + 1) / D_g) / ((row total - total + 1) / D_r)) with D_g the sum of d over the group's cells and D_r the sum over
 * the rest (a pseudo-bulk ratio: integers in, no order-dependent float sum).  A window is tested when at least min_cells kept cells have
 * an entry; untested windows are NA and do not enter the correction.  q is Benjamini-Hochberg per group over that group's tested
 * windows with finite p, ties in p in index order, with a running minimum from the largest down.  A marker of g has q <= fdr,
 * log2fc >= min_log2fc and auc > 0.5.
 * Not done: bias-matched background cells, a logistic-regression or negative-binomial test, pairwise group contrasts, a test of motif
 * deviations.
 *
 * This entry is the device part.  Operands: the counts of the kept cells, m windows and n = N cells, under the CSR rules of
 * natac_sparse_lsi (count >= 1, columns strictly ascending in a row); empty rows are allowed.  depth[n] int64 is checked for [1, 2^31)
 * only -- it need not be the matrix's column sum.  group[n] int32 in [0, n_groups), 1 <= n_groups <= NATAC_MARKERS_MAX_GROUPS,
 * 2 <= n <= NATAC_MARKERS_MAX_CELLS, m * n_groups <= NATAC_MARKERS_MAX_OUT (Context.group_rank_sums cuts the rows into blocks under it;
 * the result does not depend on the cut).  Outputs: detected int32, total and rank2 int64, each [m x n_groups] row-major, ties int64[m];
 * arm_rows int64[3] (may be NULL): the rows the short, block and long arm took.  Everything is checked on the host before any launch; a
 * failure returns NATAC_E_ARG, names the index and leaves the outputs untouched.
 * Kernels (csrc/natac_markers.hpp), by a row's number of entries L: L <= short_max (NATAC_MARKERS_SHORT_CAP unless forced) a lane group
 * of 16 / 32 / 64 lanes, one entry a lane, all pairs through cross-lane reads; L <= block_max (NATAC_MARKERS_BLOCK_CAP unless forced) a
 * workgroup that sorts the row in LDS by the exact comparison and gives every entry the start and the length of its run of equal values
 * by two binary searches; longer rows are sorted chunk by chunk in LDS into a work buffer, and every entry's less / eq come from a
 * lower- and an upper-bound search in each sorted chunk of its row, a workgroup per chunk of entries.  The
 * per-group sums are integer counters in LDS, the partial sums of a long row meet in the outputs through global integer atomics; there
 * is no floating point on the device, so two calls give the same bytes under every threshold.  The environment's
 * NATAC_MARKERS_SHORT_MAX (1 .. NATAC_MARKERS_SHORT_CAP) and NATAC_MARKERS_BLOCK_MAX (1 .. NATAC_MARKERS_BLOCK_CAP; below short_max it
 * counts as short_max) force the thresholds, for the tests.  kernel_ms (may be NULL): device time of the call's kernels. */
#define NATAC_MARKERS_MAX_OUT 33554432
#define NATAC_MARKERS_MAX_CELLS 1048576
#define NATAC_MARKERS_MAX_GROUPS 255
#define NATAC_MARKERS_SHORT_CAP 64
#define NATAC_MARKERS_BLOCK_CAP 8192
int natac_group_rank_sums(natac_ctx *ctx, int64_t m, int64_t n, const int64_t *row_ptr, const int32_t *col, const int32_t *count,
                          const int64_t *depth, const int32_t *group, int32_t n_groups, int32_t *detected, int64_t *total, int64_t *rank2,
                          int64_t *ties, int64_t *arm_rows, double *kernel_ms);
/* How natac_group_rank_sums launches for a matrix of m windows, n cells and nnz entries whose longest row has longest_row entries, with
 * n_groups groups on a device of n_cu compute units (host only: no context, no GPU needed; it reads NATAC_MARKERS_SHORT_MAX and
 * NATAC_MARKERS_BLOCK_MAX as the call does).  *short_max, *block_max: a row of L entries takes the short arm when L <= *short_max, else
 * the block arm when L <= *block_max, else the long arm.  *lanes: the lanes of a row of the short arm, the least of 16 / 32 / 64 that
 * holds min(*short_max, longest_row).  *chunk: the entries the long arm sorts at once, the largest power of two up to
 * min(*block_max, 4096), at least 16.  wg[3]: the threads of a workgroup of the short, block and long arm.  lds_bytes[3]: a workgroup's
 * dynamic LDS -- short: (256 / *lanes) rows' counters of 20 bytes a group; block: one row's counters, 16 bytes and 9 bytes an entry of
 * the power of two at or above min(longest_row, *block_max) entries (at least 16); long: the larger of 8 bytes an entry of *chunk and one
 * row's counters + 16; the counters rounded up to 16 bytes, and 0 for the block and long arm when longest_row leaves them no row.
 * grid[2]: the workgroups of the short and the block kernel if every row took that arm, at most 8 n_cu each (both walk their rows with
 * that stride).  NATAC_E_ARG for m < 1, n
 * outside [2, NATAC_MARKERS_MAX_CELLS], longest_row above n or nnz, nnz above m n, n_groups outside [1, NATAC_MARKERS_MAX_GROUPS],
 * m * n_groups above NATAC_MARKERS_MAX_OUT, n_cu < 1. */
int natac_group_rank_sums_plan(int64_t m, int64_t n, int64_t nnz, int64_t longest_row, int32_t n_groups, int32_t n_cu, int32_t *short_max,
                               int32_t *block_max, int32_t *lanes, int32_t *chunk, int32_t *wg, int64_t *lds_bytes, int32_t *grid);
/* ---- co-accessible window pairs (this library's own; `pyatac coaccess`) ----
 * The command's rule, whole: the Pearson correlation over the cells of every two windows of one chromosome that lie within a genomic
 * distance of each other, with a t-test, Benjamini-Hochberg q-values and a list of links.
 * Cells.  X is the windows x cells count matrix of `pyatac cellcounts`.  A cell is kept when its column sum is positive.  With a group
 * table (--aggregate: the table `pyatac cluster` writes, at most 255 groups) the columns are first summed per group on the host: the
 * "cells" are then the groups that have a count, and unlisted barcodes are dropped (the metacell form).  With --binarize every entry
 * counts as 1, before the aggregation.  N cells stay, 3 <= N <= NATAC_COACCESS_MAX_CELLS.
 * Windows.  Window p has entries a[p, c] >= 1 and det[p] = their number, S1[p] = sum a, S2[p] = sum a^2, all int64 on the host.  A window
 * is tested when det[p] >= min_cells; its centre is (start + end) // 2.
 * Pairs.  Per chromosome the tested windows are ranked by (centre, index).  A pair is two tested windows of one chromosome whose centres
 * differ by at most max_distance (in [0, 10^8]); it is listed once, under the member that ranks first (its owner), in rank order of the
 * partner; the chromosomes go in order of first appearance in the region list.
 * Device outputs, exact integers, per pair (p, q):  sxy int64 = the sum over the cells of a[p, c] * a[q, c],  both int32 = the number of
 * cells with an entry in both.
 * The bound.  With a_max the largest count of the matrix and L_max the longest listed row, a call needs N * a_max^2 * L_max < 2^62: then
 * every sxy, N * sxy, S1[p] * S1[q] and N * S2 - S1^2 fit in int64.
 * Host, fp64, one pair at a time:  num = N * sxy - S1[p] * S1[q] and D[p] = N * S2[p] - S1[p]^2 in int64;
 * r = float(num) / sqrt(float(D[p]) * float(D[q])) clipped to [-1, 1], NaN where a D is 0;  t = r * sqrt((N - 2) / ((1 - r) * (1 + r)));
 * p = 2 * t.sf(|t|, N - 2), and 0 where |r| == 1;  q is Benjamini-Hochberg over all pairs with a finite p (as `markers` forms it).  A link
 * has r >= min_cor (in [-1, 1]) and q <= fdr (in (0, 1]).
 * Not done: kNN metacells picked by the command itself, a depth or GC covariate, graphical-lasso regularisation as in Cicero, a
 * cross-chromosome background, a peak-to-gene step (`genescores` has the genes, but the package has no expression input).
 *
 * This entry is the device part.  Operands: the counts as natac_group_rank_sums takes them -- CSR, m rows and n cells, count >= 1,
 * columns strictly ascending in a row, empty rows allowed; 1 <= n <= NATAC_COACCESS_MAX_CELLS, m < 2^31.  order[k] int32: the row ids of
 * the listed windows in rank sequence, in [0, m), not necessarily distinct; k < 2^31.  hi[k] int64: the partners of order[i] are
 * order[i + 1 .. hi[i]), i < hi[i] <= k.  pair_ptr[k + 1] int64: pair_ptr[0] == 0 and pair_ptr[i + 1] - pair_ptr[i] == hi[i] - i - 1; the
 * pairs of owner i start at pair_ptr[i], and pair_ptr[k] <= NATAC_COACCESS_MAX_PAIRS (Context.window_pair_sums cuts the owners into
 * blocks under it; the result does not depend on the cut).  Outputs: sxy int64 and both int32, [pair_ptr[k]] each; arm_owners int64[2]
 * (may be NULL): the owners with at least one partner that the table and the search arm took.  Everything is checked on the host before
 * any launch, the bound above included (its message names N, a_max and L_max); a failure returns NATAC_E_ARG, names the index and leaves
 * the outputs untouched.  k == 0 or pair_ptr[k] == 0 returns NATAC_OK without a launch.
 * Kernels (csrc/natac_coaccess.hpp): a workgroup of 256 threads owns one window at a time, at most 8 n_cu workgroups with a grid stride
 * over the owners; the owner's row sits in LDS and every partner row goes to a lane group of 16 / 32 / 64 lanes (the least that holds
 * ceil(listed entries / k)), a lane taking the partner's entries with that stride; the group's sums meet by cross-lane reads and one
 * lane stores the pair.  Table arm, n <= table_max (NATAC_COACCESS_TABLE_CAP unless forced): a dense LDS table of the owner's counts over
 * all cells, zeroed once per workgroup, written and cleared at the owner's columns only, one LDS read per partner entry.  Search arm,
 * any n: the owner's (cell, count) pairs in LDS, at most chunk (NATAC_COACCESS_CHUNK_CAP unless forced) at a time, a binary search per
 * partner entry; the first chunk of an owner stores the pair, later chunks add to it with plain loads and stores.  No atomics and no
 * floating point: two calls give the same bytes under every table_max and chunk.  The environment's NATAC_COACCESS_TABLE_MAX
 * (1 .. NATAC_COACCESS_TABLE_CAP) and NATAC_COACCESS_CHUNK (a power of two in 16 .. NATAC_COACCESS_CHUNK_CAP; any other value is ignored)
 * force them, for the tests.  kernel_ms (may be NULL): device time of the call's kernel. */
#define NATAC_COACCESS_MAX_PAIRS 33554432
#define NATAC_COACCESS_MAX_CELLS 1048576
#define NATAC_COACCESS_TABLE_CAP 16384
#define NATAC_COACCESS_CHUNK_CAP 8192
int natac_window_pair_sums(natac_ctx *ctx, int64_t m, int64_t n, const int64_t *row_ptr, const int32_t *col, const int32_t *count,
                           int64_t k, const int32_t *order, const int64_t *hi, const int64_t *pair_ptr,
                           int64_t *sxy, int32_t *both, int64_t *arm_owners, double *kernel_ms);
/* How natac_window_pair_sums launches for a matrix of m windows, n cells and nnz entries of which k windows are listed, with
 * listed_entries entries between them (counted with multiplicity), on a device of n_cu compute units (host only: no context, no GPU
 * needed; it reads NATAC_COACCESS_TABLE_MAX and NATAC_COACCESS_CHUNK as the call does).  *arm: 0 the table arm (n <= *table_max), 1 the
 * search arm.  *lanes: the lanes of a partner row, the least of 16 / 32 / 64 that holds ceil(listed_entries / k).  *chunk: the owner's
 * entries the search arm holds at once.  *wg: the threads of a workgroup.  *lds_bytes: a workgroup's dynamic LDS -- table: 4 n rounded
 * up to 16; search: 8 *chunk.  *grid: the workgroups of the launch if every listed window has a partner, min(k, 8 n_cu).  NATAC_E_ARG
 * for m or k outside [1, 2^31), n outside [1, NATAC_COACCESS_MAX_CELLS], nnz above m n, listed_entries above k n, n_cu < 1. */
int natac_window_pair_sums_plan(int64_t m, int64_t n, int64_t nnz, int64_t k, int64_t listed_entries, int32_t n_cu, int32_t *arm,
                                int32_t *table_max, int32_t *lanes, int32_t *chunk, int32_t *wg, int64_t *lds_bytes, int32_t *grid);
/* ---- distance-weighted gene activity per cell (this library's own; `pyatac genescores`) ----
 * The command's rule, whole: per gene and cell, the sum over the cell's Tn5 insertions around the gene of an integer weight that falls
 * with the distance to the gene body (the gene-score model ArchR made usual), as a sparse matrix in the layout of `pyatac cellcounts`.
 * Genes.  A BED row (chrom, start, end, name, strand), end - start >= 1; rows stay in file order, names need not be unique.
 * Extended body, with u = --upstream in [0, 2^20]:  [bs, be) = [max(0, start - u), end) for a plus gene, [start, end + u) for a minus gene.
 * Window, with 0 <= e_min <= e_max <= 2^20, per chromosome:  prev(g) = the largest be_h over the other genes h with be_h <= bs_g
 * (-infinity if none), next(g) = the smallest bs_h over the other genes with bs_h >= be_g (+infinity if none);
 * wl = max(0, max(bs - e_max, min(bs - e_min, prev))),  wh = min(be + e_max, max(be + e_min, next)):  the window reaches up to e_max on
 * either side, stops at the nearest gene that lies wholly beyond, and always reaches at least e_min; genes that overlap g do not limit
 * it, and --no_boundaries takes prev = -infinity, next = +infinity.  Integer work on the host.
 * Weights, with D = --decay in [1, 10^7] and U = --unit in [4, 65536]:  w[d] = int(rint(U * (exp(-d / D) + exp(-1)))) for d = 0 .. e_max,
 * int32, formed once on the host in fp64; every w[d] >= 1.
 * Records.  A record is the fragment l = pos + 4, ilen = tlen - 8, r = l + ilen - 1 (the ATAC offsets of natac_region_counts) and counts
 * when lower <= ilen < upper.  Its two insertions are l and r; each counts on its own, also when r == l or r == l - 1.
 * Score.  An insertion x with wl <= x < wh has the distance d = 0 when bs <= x < be, d = bs - x to the left of the body and
 * d = x - be + 1 to the right, and adds w[d] to entry (gene, cell).  An entry exists where at least one insertion hit; its value is the
 * exact integer sum.
 * Not done: gene-length scale factors (a constant per gene, without effect on a per-gene rank test), the 500-base tiles ArchR sums over,
 * a ceiling per tile, depth normalisation of the written values (`markers` divides by the column sum itself), an expression input,
 * peak-to-gene links, GTF or GFF parsing.
 *
 * This entry is the device part, one chromosome per call, and follows natac_region_cell_counts throughout.  Operands: pos[n_frags]
 * non-decreasing, tlen, cell in [0, n_cells), n_cells in [1, NATAC_SPLIT_MAX_BARCODES].  Per gene win_lo <= body_lo <= body_hi <= win_hi,
 * body_lo - win_lo < n_w and win_hi - body_hi < n_w; genes may overlap, repeat and come in any order.  1 <= n_w <= 2^20 + 1 and
 * 1 <= weight[d] <= NATAC_GENESCORES_MAX_WEIGHT.  0 <= lower < upper <= 50000.
 * Outputs: CSR with one row per gene in the given order, col (the cell) strictly ascending within a row, val the sum.  row_ptr[n_genes + 1]
 * is written by every call that passes the checks.  col == val == NULL with cap == 0 is the sizing call; a cap below row_ptr[n_genes]
 * returns NATAC_E_ARG with col and val untouched.  hits[n_genes] (may be NULL): the insertions that counted per gene.  arm_rows[2] (may
 * be NULL): the non-empty rows the short and the table arm took.  kernel_ms (may be NULL): device time from the first to the last kernel.
 * Checks: everything above on the host before any launch; a failure returns NATAC_E_ARG, names the index and leaves the outputs
 * untouched.  The one bound that needs the device, hits[g] * max(weight) < 2^31, is checked by the entry between the counting pass and
 * the first sum (the message names the gene, nothing is written): with it no 32-bit counter and no val can wrap.  n_genes == 0 or
 * n_frags == 0 writes zeros and launches nothing.
 * Kernels (csrc/natac_genescores.hpp).  The candidates of a row are one contiguous range of records (natac_region_ranges with
 * start = win_lo, end = win_hi).  Rows go by their hits h.  Short arm, h <= short_max (NATAC_GENESCORES_SHORT_CAP unless forced): one wave
 * per row, the (cell, weight) pairs sorted by cell by a bitonic network over the lanes, run heads by one ballot, a run's sum by a
 * segmented cross-lane scan.  Table arm, every other row: one workgroup of 256 threads per (row, cell tile); a tile is at most
 * NATAC_GENESCORES_TILE_CAP cells, one 32-bit LDS counter each, and there are ceil(n_cells / tile) tiles; the threads walk the row's
 * candidates and add with integer LDS atomics, then every thread scans its contiguous run of the tile's words and a block scan places
 * the (cell, value) pairs in ascending order.  Both arms run a count pass and, behind a scan of the counts, a fill pass; there is no
 * staging area.  No floating point, no global atomics on the sums: the same bytes from two calls, under every short_max and tile, and
 * from any split of the genes into calls.  The environment's NATAC_GENESCORES_SHORT_MAX (1 .. NATAC_GENESCORES_SHORT_CAP) and
 * NATAC_GENESCORES_TILE (a power of two in 16 .. NATAC_GENESCORES_TILE_CAP; any other value is ignored) force them, for the tests. */
#define NATAC_GENESCORES_SHORT_CAP 64
#define NATAC_GENESCORES_TILE_CAP 16384
#define NATAC_GENESCORES_MAX_WEIGHT 1048576
int natac_gene_cell_scores(natac_ctx *ctx, int64_t n_frags, const int64_t *pos, const int64_t *tlen, const int32_t *cell, int32_t n_cells,
                           int64_t n_genes, const int64_t *win_lo, const int64_t *win_hi, const int64_t *body_lo, const int64_t *body_hi,
                           int32_t n_w, const int32_t *weight, int lower, int upper,
                           int64_t *row_ptr, int64_t cap, int32_t *col, int32_t *val, int64_t *hits, int64_t *arm_rows, double *kernel_ms);
/* How natac_gene_cell_scores launches for n_genes genes and n_cells cells of which table_rows rows take the table arm, on a device of
 * n_cu compute units (host only: no context, no GPU needed; it reads NATAC_GENESCORES_SHORT_MAX and NATAC_GENESCORES_TILE as the call
 * does).  *short_max: rows of at most this many hits take the short arm.  *tile: the cells of a table tile -- unless forced, the least
 * power of two that holds n_cells, between 256 and NATAC_GENESCORES_TILE_CAP.  *n_tiles: ceil(n_cells / *tile).  *wg: the threads of a
 * workgroup.  *lds_bytes: a table workgroup's dynamic LDS, 4 *tile.  *grid: the workgroups of the table launch,
 * min(table_rows * *n_tiles, 8 n_cu).  NATAC_E_ARG for n_genes outside [1, 2^40), n_cells outside [1, NATAC_SPLIT_MAX_BARCODES],
 * table_rows outside [0, n_genes], n_cu < 1. */
int natac_gene_cell_scores_plan(int64_t n_genes, int32_t n_cells, int64_t table_rows, int32_t n_cu, int32_t *short_max, int32_t *tile,
                                int32_t *n_tiles, int32_t *wg, int64_t *lds_bytes, int32_t *grid);
/* `pyatac doublets` (this package's own command: the reference has no such tool): a doublet score per cell of a `cellcounts` matrix, by
 * the usual method -- simulate doublets by adding two cells' counts, put them into the LSI space of the real cells, and score every real
 * cell by the share of simulated doublets among its nearest neighbours (Scrublet's likelihood, ArchR's removal rule).
 * Space.  Everything up to V is `cluster`'s, with the same flags and checks: tfidf_weights, r = components + oversample <= 64, the same
 * natac_sparse_lsi call.  g = numpy.random.default_rng(seed); q0 = g.standard_normal((windows, r)) is drawn first, so the LSI is bit for
 * bit `cluster`'s for that seed.  N cells are kept (total > 0), N >= 2.
 * Simulated doublets.  S = int(rint(ratio * N)), ratio in (0, 8], S >= 1.  a = g.integers(0, N, S), then b = g.integers(0, N, S), index
 * the kept cells; a[i] == b[i] is allowed.  Doublet i has the counts x[a] + x[b] and the total total[a] + total[b]; with --binarize every
 * window of the union counts 1.
 * Projection (host, fp64).  Every column, real and simulated alike, goes through one function: the weighted entry is
 * t = a' * (1 / total) * row_weight[w], or log1p(10000 t) with --method log, the row weights those of the real cells, and
 * E = A V[:, :components] is one scipy.sparse CSR-times-dense product with sorted indices.  The real cells are projected this way too,
 * not taken from U sigma.  depth_correlation of the real rows against their totals decides the components kept, as in `cluster`;
 * P = unit_rows of the kept components has N + S rows, the real cells first, and d <= 64 columns.
 * Neighbours.  k = --neighbors in [1, 1024] if given, else max(1, int(rint(0.5 sqrt(N)))); k_adj = int(rint(k (1 + S / N))) clipped to
 * [1, min(1024, N + S - 1)] (the summary says when the cap of 1024 applied).  For every real cell: its k_adj nearest rows of P, itself
 * excluded, by natac_knn's rule below.
 * Score (host, fp64, in this order).  n_syn = the neighbours with index >= N; q = (n_syn + 1) / (k_adj + 2); rr = S / N;
 * rho = --expected_rate in (0, 0.5]; score = q * rho / rr / (1 - rho - q * (1 - rho - rho / rr)).  The denominator is positive for q < 1.
 * Flag.  --filter_ratio F and --max_score X exclude each other.  With --max_score a cell is flagged when score > X.  Otherwise, F in
 * [0, 100] (default 1.0): n_remove = min(N - 1, int(F * N * N / 100000)) and the first n_remove cells by (score descending, index
 * ascending) are flagged.  No knee or histogram threshold is searched for.
 * Not done: approximate search, ArchR's down-sampling of the simulated counts, an automatic threshold, UMAP or graph clustering on the
 * graph, writing V into `cluster`'s BASE.lsi.npz.
 *
 * natac_knn is the device part and a general exact k-nearest-neighbour search.  x[nr, dim] are the references and q[nq, dim] the queries,
 * both row-major fp64.  d2(i, j) starts at acc = 0; for c = 0 .. dim - 1 in order t = q[i, c] - x[j, c], then acc = acc + t * t, each of
 * the three operations rounded once, no contraction.  Reference j is excluded for query i when self_offset >= 0 and j == i + self_offset.
 * Row i of idx[nq, k] and dist2[nq, k] holds the k smallest references by (d2, j) ascending; with fewer than k references available the
 * tail is idx = -1, dist2 = +inf.  The rule is a sequence of IEEE operations and a total order: the result is exact.
 * Limits: 1 <= dim <= NATAC_KNN_MAX_DIM, 1 <= k <= NATAC_KNN_MAX_K, 1 <= nr <= NATAC_KNN_MAX_REFS, nq >= 0, nq * k <= NATAC_KNN_MAX_OUT
 * (Context.knn cuts the queries into blocks under it; the result does not depend on the cut), self_offset -1 or in [0, nr - nq], every
 * value finite with |v| <= 2^NATAC_KNN_MAX_EXP, so that no sum can overflow (64 * 2^1002 < 2^1024).  All checks run on the host before any
 * launch; a refusal is NATAC_E_ARG, names the array and the first bad index and leaves the outputs untouched.  nq == 0 returns NATAC_OK
 * without a launch.  arm_queries[2] (may be NULL): the queries the wave and the lds arm took.  kernel_ms (may be NULL): the kernel's
 * device time.
 * Kernel (csrc/natac_knn.hpp).  A workgroup of 4 waves owns a tile of queries, a wave its share of them, and walks the references in tiles
 * staged transposed and padded in LDS; a lane holds one reference and the accumulators of the wave's queries, whose coordinates are LDS
 * broadcast reads.  Per query the k-th best so far is a threshold; candidates below it are appended to a buffer by ballot and prefix
 * count, and a full buffer is reduced with the list to the k best by a bitonic sort on (bits of d2, j).  Wave arm, k <= wave_k_max (64
 * unless forced): the list is one entry per lane in registers.  Lds arm, larger k: list and buffer are one LDS array of the power of two
 * >= max(k + 64, 128) entries.  No scratch, no atomics: the same bytes from two calls and under every arm and tile.  The environment's
 * NATAC_KNN_WAVE_K_MAX (1 .. 64), NATAC_KNN_QUERY_TILE (a power of two in 4 .. 32) and NATAC_KNN_REF_TILE (a power of two in 64 .. 256)
 * force them, for the tests; a value outside its rule, or one whose LDS would pass NATAC_KNN_LDS_CAP, is ignored. */
#define NATAC_KNN_MAX_DIM 64
#define NATAC_KNN_MAX_K 1024
#define NATAC_KNN_MAX_REFS 16777216
#define NATAC_KNN_MAX_OUT 268435456
#define NATAC_KNN_MAX_EXP 500
#define NATAC_KNN_LDS_CAP 163840
int natac_knn(natac_ctx *ctx, int64_t nq, int64_t nr, int32_t dim, const double *q, const double *x, int64_t self_offset, int32_t k,
              int32_t *idx, double *dist2, int64_t *arm_queries, double *kernel_ms);
/* How natac_knn launches for nq queries against nr references of dim columns with k neighbours on a device of n_cu compute units (host
 * only: no context, no GPU needed; it reads the three NATAC_KNN_ variables as the call does).  *arm: 0 wave, 1 lds.  *wave_k_max: the
 * largest k of the wave arm.  *query_tile: the queries of a workgroup, 4 times a wave's 1, 2, 4 or 8 -- unless forced, 8 a wave, halved
 * while the query tiles are fewer than 4 n_cu (wave arm) or 8 n_cu (lds arm) or the workgroup takes more than 80 KiB of LDS.  *ref_tile: the references staged at a
 * time -- unless forced, the largest of 256, 128, 64 whose copy stays within 24 KiB.  *capacity: the candidates a query's buffer holds,
 * 64 (wave) or the array's entries minus k (lds).  *wg: the threads of a workgroup.  *lds_bytes: its dynamic LDS, at most
 * NATAC_KNN_LDS_CAP.  *grid: min(ceil(nq / *query_tile), 8 n_cu), at least 1; the workgroups stride over the query tiles.  NATAC_E_ARG
 * for the limits above and n_cu < 1. */
int natac_knn_plan(int64_t nq, int64_t nr, int32_t dim, int32_t k, int32_t n_cu, int32_t *arm, int32_t *wave_k_max, int32_t *query_tile,
                   int32_t *ref_tile, int32_t *capacity, int32_t *wg, int64_t *lds_bytes, int32_t *grid);
/* _nucleotideHelper, pyatac/get_nucleotide.py:19-38, with chunk.center / chunk.slop (pyatac/chunk.py:26-54) and seq.get_sequence /
 * seq_to_mat (pyatac/seq.py:11-45), for the sites of one chromosome: seq[n] is the chromosome as the FASTA has it, case included;
 * center[i] in [0, n) the centred site, minus[i] != 0 a minus-strand site (minus == NULL: all plus).  word = 1 counts the rows
 * A C G T, word = 2 the 16 rows of itertools.product("CGAT", repeat=2); K = up + down + 1 columns.  A plus site reads the bases
 * [center - up, center + down + word), a minus site [center - down - word + 1, center + up + 1) reversed, upper-case bases complemented
 * and lower-case ones not (the reference translates before it upper-cases); then every letter is upper-cased and column j counts the
 * word at j.  A site whose window leaves [0, n) is skipped whole.  counts[(4 or 16) x K] and n_used = the sites counted are exact
 * int64, overwritten.  up, down in [0, 524288].  kernel_ms (may be NULL): device time of the counting kernel. */
int natac_site_seq_counts(natac_ctx *ctx, const uint8_t *seq, int64_t n, int64_t n_sites, const int64_t *center, const uint8_t *minus,
                          int up, int down, int word, int64_t *counts, int64_t *n_used, double *kernel_ms);
/* sites per partial sum of natac_site_signal's aggregate: part of its documented summation order */
#define NATAC_SIGNAL_SEG 64
/* _signalHelper, pyatac/signal_around_sites.py:24-74, after the track has been read (pyatac/bedgraph.py:6-14): vals[n_vals] holds the
 * per-base values the sites need, NaN where no record covers a base.  Site i has K columns; in genomic orientation they are lead[i]
 * zeros, the len[i] values vals[src[i] ..], and zeros up to K (the reference pads a window clipped by a chromosome end with zeros,
 * signal_around_sites.py:42-47); minus[i] != 0 reverses the row (minus == NULL: all plus).  Then, by flags: 1 (--exp) v = exp(v), so a
 * padding zero becomes 1 and NaN stays; 2 (--positive) v < 0 becomes 0, NaN and -0.0 stay; 4 (--scale) NaN becomes 0 and the row is
 * divided by S + (S == 0), S = the sum of its absolute values.  mat (may be NULL) [n_sites x K] gets the rows; agg[K], overwritten,
 * their column sums with NaN as 0.  Both are deterministic: a column is added in site order from 0 over every segment of
 * NATAC_SIGNAL_SEG consecutive sites, the segment sums are added in segment order from 0, and S is added in an order that depends on
 * K alone; no floating-point atomics.  The operands are checked on the host (NATAC_E_ARG names the site): K in [1, 1048577],
 * len, lead >= 0, lead + len <= K, 0 <= src, src + len <= n_vals.  n_sites == 0 gives zeros and launches nothing.  kernel_ms (may be
 * NULL): device time of the kernels. */
int natac_site_signal(natac_ctx *ctx, const double *vals, int64_t n_vals, int64_t n_sites, const int64_t *src, const int32_t *len,
                      const int32_t *lead, const uint8_t *minus, int K, int flags, double *mat, double *agg, double *kernel_ms);
/* signal.correlate(sub, vmat, mode='valid')[0] as used by SignalTrack.calculateSignal / BiasTrack
 * (nucleoatac/NucleosomeCalling.py:34-36, 60-63): sub[R x ncol], vmat[R x W] row-major, out[ncol-W+1]. */
int natac_correlate_valid(natac_ctx *ctx, const double *sub, int64_t ncol, const double *vmat, int R, int W, double *out);
/* calculateOccupancy, nucleoatac/Occupancy.py:104-120, for one window: inserts[upper], bias[upper] with the model
 * set by natac_set_occ_model; out[3] = {occ, lower, upper}.  Returns NATAC_E_ARG with the message
 * "no alpha passes the likelihood-ratio test" where the reference raises ValueError (Occupancy.py:118). */
int natac_calculate_occupancy(natac_ctx *ctx, const double *inserts, const double *bias, double *out);

/* ---- native track writer (host side, multi-threaded) ------------- */
/* Track.write_track, pyatac/tracks.py:37-74, for n_chunks tracks at once (chunk i: chroms[i], chunk_start[i], values
 * vals[out_off[i] .. out_off[i+1]) ), run-length bedGraph text with python-2 float formatting, NaN runs skipped, and -- as in the
 * reference, whose loop overwrites prev_value with the NaN before flushing (tracks.py:56-66) -- a run of values directly followed
 * by a NaN is NOT written.  write_zero: bit 0 = write runs of 0 (the reference's write_zero), bit 1 = also keep runs that precede a
 * NaN (deviation from the reference, off by default).
 * compress: 0 = plain text, 1..9 = BGZF at that deflate level (bgzip-compatible; run_occ.py:130-136).  append != 0
 * appends to `path`; finish != 0 terminates a BGZF file with the EOF marker block.  n_threads <= 0: automatic.
 * No GPU involved; usable on the arrays natac_batch_download returns. */
int natac_write_bedgraph(const char *path, int append, int compress, int finish, int32_t n_chunks, const char *const *chroms,
                         const int64_t *chunk_start, const int64_t *out_off, const double *vals, int write_zero,
                         int n_threads, int64_t *bytes_written);

/* ---- device-side track writer (SURVEY.md section 8f row 1 moved onto the GPU) ------------------------------------------------- */
/* Track.write_track, pyatac/tracks.py:37-74, for one per-base track of a batch ON THE DEVICE: run-length detection (including the
 * reference's rule that a run directly followed by a NaN is not written, tracks.py:56-66), python-2 `str(float)` ('%.12g' with exact
 * 192-bit integer arithmetic) and the line layout `chrom \t start \t end \t value \n`, chunk i on names[chrom_id[i]] at chunk_start[i].
 * compress = 0: the text itself; compress != 0: BGZF members of <= 0xff00 text bytes each (no EOF marker; the bgzip step of
 * run_occ.py:130-136) from a line-structured LZ77 + a Huffman code built for this text (csrc/natac_deflate.hpp).  write_zero as
 * in natac_write_bedgraph.  The result stays on the device until the next call; fetch it with natac_batch_format_fetch.
 * n_bytes = size of the result, n_text_bytes = size of the text, n_lines = lines written, n_hard = values whose 12th digit could
 * not be decided from the truncated power-of-ten table (only |v| >= 1e12 or < 1e-44 can; the caller then formats this track
 * with natac_write_bedgraph instead).  Byte-identical to natac_write_bedgraph's text when n_hard == 0. */
int natac_batch_format_track(natac_batch *b, int track, const int32_t *chrom_id, const char *const *names, int32_t n_names,
                             const int64_t *chunk_start, int write_zero, int compress, int64_t *n_bytes, int64_t *n_text_bytes,
                             int64_t *n_lines, int32_t *n_hard);
int natac_batch_format_fetch(natac_batch *b, void *dst, size_t dst_bytes);
/* The same without waiting: _begin starts the copy of the last natac_batch_format_track result into `dst` (pinned host memory) on a
 * second stream and returns; the batch may format its next track at once (the reference's writer processes likewise take track after
 * track, run_occ.py:130-136).  `dst` holds the result after natac_batch_format_fetch_wait, which waits for every copy begun on the
 * batch; natac_batch_free and natac_batch_release_outputs wait too.  The tabix records of a result (natac_batch_format_index_*) must be
 * fetched before the next natac_batch_format_track, as with the blocking fetch. */
int natac_batch_format_fetch_begin(natac_batch *b, void *dst, size_t dst_bytes);
int natac_batch_format_fetch_wait(natac_batch *b);
/* The .tbi of a file assembled from natac_batch_format_track(compress) results, WITHOUT re-reading the file (the reference runs
 * pysam.tabix_index(..., preset="bed") over every finished file, run_occ.py:136-139).  The device reduces the lines of a result to runs
 * of records per 16-kb leaf bin (one per ~16 kb instead of one per base): natac_batch_format_index_size / _fetch return the runs
 * of the LAST result -- chromosome id, [beg, end), record count, text offsets [t0, t1) -- and the member start offsets
 * member_pos[n_members + 1] inside the result (n_text = bytes of text in it: the last member is partial).  natac_tbi_push enters them into an incremental index once the caller knows at
 * which byte `file_offset` of the .gz the result is written (results may be produced out of order by several contexts and
 * written in order by one writer); natac_tbi_write serialises the same index natac_tabix_index builds from the finished file. */
typedef struct natac_tbi natac_tbi;
int natac_tbi_create(natac_tbi **out);
void natac_tbi_free(natac_tbi *t);
int natac_batch_format_index_size(natac_batch *b, int64_t *n_groups, int64_t *n_members, int64_t *n_text);
int natac_batch_format_index_fetch(natac_batch *b, int32_t *cid, int64_t *beg, int64_t *end, int64_t *count, uint64_t *t0, uint64_t *t1,
                                   uint64_t *member_pos);
int natac_tbi_push(natac_tbi *t, int64_t n, const char *const *names, int32_t n_names, const int32_t *cid, const int64_t *beg,
                   const int64_t *end, const int64_t *count, const uint64_t *t0, const uint64_t *t1, const uint64_t *member_pos,
                   int64_t n_members, int64_t n_text, int64_t file_offset);
int natac_tbi_write(natac_tbi *t, const char *tbi_path, int64_t *n_records);
/* the device formatter on arbitrary doubles (validation): out_off[i] .. out_off[i+1] = python-2 str(vals[i]); out_cap >= 24 n */
int natac_format_doubles(natac_ctx *ctx, const double *vals, int64_t n, char *out, size_t out_cap, int64_t *out_off, int32_t *n_hard);
/* host restatement of the device BGZF encoder (no GPU): text + line start offsets -> the members natac_batch_format_track(compress)
 * produces for the same text, byte for byte */
int natac_bgzf_lines_host(const char *text, int64_t n, const int64_t *line_off, int64_t n_lines, void *out, size_t out_cap,
                          int64_t *n_bytes);

/* BED-like rows with python-2 float columns, written natively: row r = names[chrom_id[r]] \t start[r] \t end[r] (\t vals[r][c])* --
 * the text of OccPeak.asBed / Nucleosome.asBed (nucleoatac/Occupancy.py:166-171, NucleosomeCalling.py:195-199) for millions of rows.
 * vals is row-major [n_rows x n_cols] (n_cols <= 32), NaN prints as "nan".  append != 0 appends to `path`. */
int natac_write_bed_rows(const char *path, int append, int64_t n_rows, const int32_t *chrom_id, const char *const *names,
                         int32_t n_names, const int64_t *start, const int64_t *end, const double *vals, int32_t n_cols);

/* the same with one more text column at the end of every row, labels[label_id[r]] -- the rows of nucmap_combined.bed
 * (MergedNuc.asBed, nucleoatac/merge.py:23-30: chrom start end occ occ_lower occ_upper reads source) */
int natac_write_bed_rows_labeled(const char *path, int append, int64_t n_rows, const int32_t *chrom_id, const char *const *names,
                                 int32_t n_names, const int64_t *start, const int64_t *end, const double *vals, int32_t n_cols,
                                 const int32_t *label_id, const char *const *labels, int32_t n_labels);

/* bgzip: compress a text file into BGZF members of <= 0xff00 input bytes + the EOF marker (the reference's
 * pysam.tabix_compress, pyatac/utils.py:135-141 / run_nuc.py:204-214). */
int natac_bgzip_file(const char *src, const char *dst, int level, int n_threads);
/* tabix: write the .tbi index ("bed" preset: columns 1/2/3, 0-based half-open, '#' comments) of a BGZF-compressed,
 * position-sorted BED / bedGraph file (the reference's pysam.tabix_index(..., preset="bed"), same call sites).
 * tbi_path NULL: `path` + ".tbi".  n_records (may be NULL) receives the number of indexed lines. */
int natac_tabix_index(const char *path, const char *tbi_path, int n_threads, int64_t *n_records);

/* region reads through the index (pysam.TabixFile.fetch as used by Track.read_track, pyatac/tracks.py:75-87): out[x - start] =
 * the value column (1-based, 4 for bedGraph) of the records of `chrom` overlapping [start, end); bases without a record keep
 * `empty`.  One handle per file and thread. */
typedef struct natac_tbx natac_tbx;
int natac_tbx_open(const char *path, natac_tbx **out);
void natac_tbx_close(natac_tbx *t);
int natac_tbx_read_values(natac_tbx *t, const char *chrom, int64_t start, int64_t end, int value_col, double empty, double *out,
                          int64_t *n_records);
/* the same for n regions in one call (the three occupancy tracks of every chunk of a batch: NucChunk.getOcc,
 * nucleoatac/NucleosomeCalling.py:284-293, NFRChunk.getOcc, NFRCalling.py:63-68): region i = names[chrom_id[i]]:[start[i], end[i]),
 * written to out[out_off[i] ...].  n_threads cursors of the handle take contiguous runs of the list (0 = up to 64); a cursor keeps
 * the members it inflated last, so position-sorted lists inflate and parse every member once. */
int natac_tbx_read_regions(natac_tbx *t, int64_t n, const int32_t *chrom_id, const char *const *names, int32_t n_names,
                           const int64_t *start, const int64_t *end, int value_col, double empty, double *out, const int64_t *out_off,
                           int n_threads, int64_t *n_records);

/* ---- host-side packing of a chunk list (what replaces the per-chunk bamHandle.fetch of pyatac/fragments.pyx:21-36) ---- */
/* pos[c] / tlen[c]: the forward proper-pair reads of chromosome c (natac_bam_ref_reads), pos ascending.  chrom_id[i] < 0: a
 * chunk on a chromosome without reads.  Attached to chunk i are the reads with pos in [start - margin - shift, end + margin)
 * (shift = 4 when atac), as l = pos + shift - start, n = |tlen| - (8 when atac), ordered by centre l + (n-1)//2 (stable).
 * Call once with lpos == NULL: fills frag_off[0..n_chunks] and first[0..n_chunks) (count pass); allocate
 * frag_off[n_chunks] entries and call again with lpos / ilen to fill them (multi-threaded). */
int natac_pack_chunks(int32_t n_chunks, const int64_t *chunk_start, const int64_t *chunk_end, const int32_t *chrom_id, int32_t n_chroms,
                      const int64_t *const *pos, const int64_t *const *tlen, const int64_t *n_per_chrom, int64_t margin, int atac,
                      int64_t *frag_off, int64_t *first, int32_t *lpos, int32_t *ilen, int n_threads);

/* ---- native BAM -> fragment arrays extractor (host side) -------------- */
/* Decode a BAM once (streaming: bounded windows of compressed data, parallel BGZF inflate per window, records may straddle
 * windows; peak memory is independent of the file size) into per-reference arrays of the reads pyatac/fragments.pyx:25 keeps
 * (`is_proper_pair and not is_reverse`): pos = leftmost 0-based coordinate, tlen = |template length|, in file order. */
typedef struct natac_bam natac_bam;
int natac_bam_open(const char *path, int n_threads, natac_bam **out);
void natac_bam_close(natac_bam *bam);
int natac_bam_counts(natac_bam *bam, int32_t *n_refs, int64_t *n_records, int64_t *n_kept);
int natac_bam_ref_info(natac_bam *bam, int32_t ref, char *name, size_t name_len, int64_t *length, int64_t *n_reads);
int natac_bam_ref_reads(natac_bam *bam, int32_t ref, int64_t *pos, int64_t *tlen, int64_t n);
/* The same extraction with the BGZF members inflated and the records walked ON THE DEVICE (csrc/natac_bgzf_dev.hpp: the file in
 * windows, one lane per member; csrc/natac_bam_dev.hpp: the record chain through the members is confirmed link by link from the end
 * of the header, so the result is exactly natac_bam_open's).  A file whose chain cannot be confirmed -- or a HIP failure such as no
 * memory for a window -- sends the file through the host decoder inside this call; *on_device (may be NULL) tells which one
 * answered.  Damaged files fail with the host decoder's messages. */
int natac_bam_open_device(natac_ctx *ctx, const char *path, natac_bam **out, int *on_device);
/* ---- fragment file (fragments.tsv.gz: Cell Ranger ATAC, the ENCODE pipeline, chromap, sinto, SnapATAC / ArchR) -> the same handle ----
 * THE FORMAT RULE (nucleoatac_amd/pyatac/fragments.py restates it; csrc/natac_fragfile.hpp: parse_line is it).
 * Lines: a line ends in '\n', a '\r' directly before it is dropped; a last line without '\n' is a line; empty lines and lines whose
 *   first byte is '#' are skipped.
 * Fields: every other line is a data line: fields separated by TAB only, at least three; fields after the third are ignored whatever
 *   bytes they hold (barcode, duplicate count: one line is one fragment, identical lines are separate fragments).  chrom is 1-255
 *   bytes; start and end are 1-10 ASCII digits (no sign, no blanks), value <= 2^31 - 1, end >= start.
 * Mapping: [start, end) is the insertion-to-insertion interval the reference's ATAC offsets produce (pyatac/fragments.pyx:26-31:
 *   l = start, ilen = end - start), so the stored record is pos = start - 4 (may be negative), tlen = end - start + 8; end == start is
 *   kept (the BAM path admits ilen == 0 too).  A file written with the +4/-5 convention is one base shorter at the right end than the
 *   reference's +4/-4 reading of the same BAM; nothing is corrected: the writer's convention is not recorded in the file.
 * Chromosomes: numbered in order of first appearance; one that comes back later in an unsorted file keeps its id, its records in file
 *   order.  There is no sequence dictionary: a chromosome's length is the largest end on it.
 * Errors: a malformed data line fails the call with "<path>: line <N>: <reason>", N 1-based and counting skipped lines, one fixed
 *   reason per cause (fewer than three fields, empty chromosome name, chromosome name longer than 255 bytes, start / end not a
 *   number, number out of range, end before start); nothing is returned.
 * The container is chosen by magic bytes: BGZF, any other gzip (several members allowed), or plain text.  The result does not depend
 * on n_threads (0 = the machine's cores, at most 64).  natac_bam_counts / _ref_info / _ref_reads / _close serve the handle, with
 * n_records = n_kept = the number of data lines. */
int natac_frag_open(const char *path, int n_threads, natac_bam **out);
/* The same with a BGZF file's members inflated (CRC-32 checked) and its text split into lines, parsed and compacted ON THE DEVICE
 * (csrc/natac_bgzf_dev.hpp, csrc/natac_fragfile_dev.hpp: PlainJob).  The host decoder answers inside this call for another container,
 * any malformed line or damaged member (so the message is natac_frag_open's by construction), a line longer than a window, more than
 * 65,536 chromosome runs in a window, or a HIP failure; *on_device (may be NULL) tells which one answered. */
int natac_frag_open_device(natac_ctx *ctx, const char *path, natac_bam **out, int *on_device);
/* ---- a fragment file split by cell barcode: one pass, one handle per cell group (a cluster, a sample, a QC whitelist) ----
 * THE SPLIT RULE (csrc/natac_fragfile.hpp: split_line is it; nucleoatac_amd/pyatac/fragments.py restates it).
 * Validation: every line is classified exactly as by natac_frag_open (same checks, same order, same reasons, same line numbers); a data
 *   line that passes them but has fewer than four fields is malformed: "no barcode field", checked last.
 * Barcode: the bytes between the third TAB and the fourth, or the line's end (the '\r' before a '\n' dropped first; a last line without
 *   '\n' keeps its '\r').  Compared byte for byte: no trimming, no case folding, a "-1" suffix is part of it.  A line whose barcode is
 *   empty, longer than 255 bytes or not in the table is UNASSIGNED: validated, counted, in no group, and no error.
 * Table: n_barcodes >= 1 distinct barcodes of 1-255 bytes, bc_bytes[bc_off[k] .. bc_off[k + 1]) (bc_off[0] == 0), each with a group
 *   bc_group[k] in [0, n_groups), n_groups in [1, NATAC_SPLIT_MAX_GROUPS].  Two equal barcodes: NATAC_E_ARG naming both entries.  At most
 *   NATAC_SPLIT_MAX_BARCODES barcodes (NATAC_E_ARG beyond); the device takes tables of up to 4,194,304, the host path answers for larger.
 * Result: out[n_groups] handles.  Every group has the SAME chromosome list (first appearance over all data lines of the file, assigned
 *   or not) and the same lengths (largest end over all data lines of the chromosome), so groups are comparable; a chromosome on which
 *   a group has nothing is present and empty.  A group's records are its lines (pos = start - 4, tlen = end - start + 8) in file order
 *   within each chromosome; a chromosome that comes back appends behind its earlier records; ties keep file order.  natac_bam_counts:
 *   n_records = the file's data lines, n_kept = the group's.  bc_count[n_barcodes] (may be NULL) = data lines per listed barcode,
 *   *n_unassigned (may be NULL) = data lines in no group.
 * Lookup: a hash of the barcode into an open-addressing table built once; a slot matches only after its bytes compared equal; the table
 *   always has an empty slot and the probe loop is bounded by the slot count.  NATAC_SPLIT_HASH_BITS=k keeps the low k bits of the hash
 *   only (tests: k = 3 makes nearly every lookup walk a chain of equal hashes).
 * Containers, windows (NATAC_BAM_WINDOW), slices and errors as natac_frag_open: the result and the first error do not depend on
 * n_threads or the window.  On any error every out[g] is NULL. */
#define NATAC_SPLIT_MAX_GROUPS 255
#define NATAC_SPLIT_MAX_BARCODES 8388608
int natac_frag_split(const char *path, int n_threads, int64_t n_barcodes, const void *bc_bytes, const int64_t *bc_off, const int32_t *bc_group,
                     int32_t n_groups, natac_bam **out, int64_t *bc_count, int64_t *n_unassigned);
/* The same with a BGZF file inflated, split into lines and parsed ON THE DEVICE as by natac_frag_open_device, every data line's barcode
 * looked up and counted there, and each window's assigned lines partitioned by group there (stable; unassigned lines never come back to
 * the host).  The host path answers inside this call for everything natac_frag_open_device hands over, for a line without a barcode
 * field, for a table of more than 4,194,304 barcodes, and for a window in which groups x chromosome runs exceeds 1,048,576;
 * *on_device (may be NULL) tells which one answered. */
int natac_frag_split_device(natac_ctx *ctx, const char *path, int64_t n_barcodes, const void *bc_bytes, const int64_t *bc_off, const int32_t *bc_group,
                            int32_t n_groups, natac_bam **out, int64_t *bc_count, int64_t *n_unassigned, int *on_device);
/* ---- a cell-tagged read: the one-group case of THE SPLIT RULE that also keeps which cell every kept record belongs to ----
 * The table is natac_frag_split's without groups (the same limits, NATAC_SPLIT_MAX_BARCODES, and the same error for two equal barcodes).
 * Every line is validated by split_line, with natac_frag_split's reasons and line numbers; a line whose barcode is empty, longer than
 * 255 bytes or unlisted is unassigned and dropped (no error); every data line counts towards its chromosome's length.  *out is ONE handle
 * (NULL on any error) whose kept records carry cell = the index of their barcode in the table: natac_bam_ref_cells copies the
 * n_reads cell indices of a reference, in the order of natac_bam_ref_reads (file order within the chromosome).  bc_count / n_unassigned
 * as natac_frag_split.  Host path only: the result does not depend on n_threads or NATAC_BAM_WINDOW.  natac_bam_ref_cells on a handle of
 * any other open call is NATAC_E_ARG. */
int natac_frag_open_cells(const char *path, int n_threads, int64_t n_barcodes, const void *bc_bytes, const int64_t *bc_off, natac_bam **out,
                          int64_t *bc_count, int64_t *n_unassigned);
int natac_bam_ref_cells(natac_bam *bam, int32_t ref, int32_t *cell);
/* ---- the cells of a fragment file: which barcodes it holds, in order of first appearance, with per-cell QC counts ----
 * THE CELLS RULE (csrc/natac_fragfile.hpp: barcode_line is it; nucleoatac_amd/pyatac/fragments.py restates it).
 * Validation and the barcode: every line is validated exactly as by natac_frag_split (the same checks, order, reasons and line numbers,
 *   "no barcode field" checked last), and the barcode is the fourth field as THE SPLIT RULE defines it (the '\r' before a '\n' dropped
 *   first, a last line without '\n' keeps its '\r'; compared byte for byte).
 * Cells: a data line whose barcode is 1-255 bytes long belongs to the cell of that barcode.  Cells are numbered in order of first
 *   appearance over the file's data lines: file order, not hash or thread order.  A data line whose barcode is empty or longer than 255
 *   bytes is UNASSIGNED: validated, counted in n_unassigned, and no error.
 * Counters: with ilen = end - start of the line, cell k has three exact int64 counters: n_frag[k] = its data lines, n_nfr[k] = those with
 *   ilen < nfr_upper, n_mono[k] = those with nfr_upper <= ilen < mono_upper.  0 < nfr_upper < mono_upper, NATAC_E_ARG otherwise (147 and
 *   294 are the binding's defaults: the usual nucleosome-free and mono-nucleosome classes).  One line is one fragment whatever its fifth
 *   column says.
 * Limits: more than NATAC_SPLIT_MAX_BARCODES distinct barcodes fails the call with "<path>: line <N>: more than 8388608 distinct
 *   barcodes", N the line on which the limit was passed.
 * Invariance: the result is a function of the file's bytes and the two bounds only: not of n_threads, NATAC_BAM_WINDOW,
 *   NATAC_FRAG_DEV_WINDOW, the BGZF member size, the container, or which path answered.
 * Containers, windows, slices and the first error as natac_frag_split.  *out is a handle (NULL on any error):
 *   natac_cells_counts: n_cells, the total barcode bytes, n_data (the file's data lines) and n_unassigned (each may be NULL);
 *   natac_cells_read: bc_bytes[total bytes] and bc_off[n_cells + 1] (cell k is bc_bytes[bc_off[k] .. bc_off[k + 1])), n_frag / n_nfr /
 *     n_mono[n_cells]; n_cells and n_bytes must be the handle's (NATAC_E_ARG otherwise), any array may be NULL;
 *   natac_cells_close. */
typedef struct natac_cells natac_cells;
int natac_frag_cells(const char *path, int n_threads, int32_t nfr_upper, int32_t mono_upper, natac_cells **out);
/* The same with a BGZF file inflated and split into lines ON THE DEVICE as by natac_frag_open_device, and the barcode table built
 * there from the file itself (csrc/natac_fragfile_dev.hpp, CellsJob: an open-addressing table in device memory that lives across
 * windows; a slot is claimed by the smallest line of a window, and only matches after the bytes compared equal; NATAC_SPLIT_HASH_BITS
 * applies).  The table has a FIXED size: 8,388,608 slots (NATAC_CELLS_DEV_SLOTS=<power of two> sets another: tests), of which at most
 * half are taken.  The host path answers inside this call for everything natac_frag_open_device hands over, for a line without a
 * barcode field, for a full table (more than slots / 2 barcodes: more than 4,194,304 by default), for more than 268,435,455 lines in
 * a window and for a HIP failure; *on_device (may be NULL) tells which one answered. */
int natac_frag_cells_device(natac_ctx *ctx, const char *path, int32_t nfr_upper, int32_t mono_upper, natac_cells **out, int *on_device);
int natac_cells_counts(natac_cells *cells, int64_t *n_cells, int64_t *n_bytes, int64_t *n_data, int64_t *n_unassigned);
int natac_cells_read(natac_cells *cells, int64_t n_cells, int64_t n_bytes, void *bc_bytes, int64_t *bc_off, int64_t *n_frag, int64_t *n_nfr,
                     int64_t *n_mono);
void natac_cells_close(natac_cells *cells);
/* test entry: the device's raw-deflate decoder run on the host (one BGZF member payload -> isize bytes); returns its error code */
int natac_inflate_raw_host(const void *src, size_t csize, void *out, size_t isize);

/* ---- objective + finite-difference gradient of K Nucleosome.getFuzz fits (host side; reference NucleosomeCalling.py:92-97, 176-184 as
 * scipy's L-BFGS-B sees them through its numerical differentiation).  nucleoatac/fuzzfit.py advances many fits in lockstep and
 * calls this once per round.  X0, lb, ub: [K][n] (n = 3, 6 or 9); sig, xs: [K][M] padded; lens[K]; exp_loop / exp_data: numpy's own
 * inner loop of float64 exp (the values must be numpy's to the last bit: csrc/natac_fuzzfit.hpp); work: (2 n + n / 3 + 1) K M doubles. */
int natac_fuzz_evaluate(int32_t K, int32_t n, int32_t M, const double *X0, const double *lb, const double *ub, const double *sig,
                        const double *xs, const int64_t *lens, void *exp_loop, void *exp_data, double *work, double *f, double *g);

/* ---- a (gzipped) BED-like table read into columns (host side): what `nucleoatac merge` parses row by row (nucleoatac/merge.py:36-64).
 * cols: 0-based indices of the columns parsed as float64 (correctly rounded, like python's float()); column 0 = chromosome (names in
 * order of first appearance), 1 / 2 = start / end.  BGZF, plain gzip and plain text alike; empty lines are skipped. */
typedef struct natac_bedtab natac_bedtab;
int natac_bedtab_open(const char *path, const int32_t *cols, int32_t n_cols, natac_bedtab **out);
void natac_bedtab_close(natac_bedtab *t);
int natac_bedtab_dims(natac_bedtab *t, int64_t *n_rows, int32_t *n_names);
int natac_bedtab_name(natac_bedtab *t, int32_t i, char *name, size_t name_len);
int natac_bedtab_fetch(natac_bedtab *t, int32_t *chrom_id, int64_t *start, int64_t *end, double *vals);   /* vals: [n_rows][n_cols] */

/* ---- native FASTA loader (host side): the genome as one upper-case byte array per record, what pyatac/seq.py:11-22 /
 * pyatac/bias.py:85-92 fetch region by region through pysam.FastaFile.  Plain-text FASTA; record names end at the first blank. */
typedef struct natac_fasta natac_fasta;
int natac_fasta_open(const char *path, int n_threads, natac_fasta **out);
void natac_fasta_close(natac_fasta *fa);
int natac_fasta_count(natac_fasta *fa, int32_t *n_records);
int natac_fasta_info(natac_fasta *fa, int32_t record, char *name, size_t name_len, int64_t *length);
int natac_fasta_read(natac_fasta *fa, int32_t record, void *out, int64_t n);     /* n must equal the record's length */

/* ---- pinned host memory + device memory pool ---------------------------------------------------------- */
/* Page-locked host buffers (hipHostMalloc): uploads from / downloads into them run at full PCIe rate and asynchronously to
 * the host.  Any caller-owned host pointer of this ABI may be pinned or pageable; results are identical. */
int natac_host_alloc(size_t bytes, void **out);
int natac_host_free(void *p);
/* The library keeps freed device blocks in a per-device cache (hipMalloc / hipFree synchronise the device, which would
 * stall other contexts' overlapping copies); this returns every cached block to the driver. */
int natac_pool_trim(void);

/* ---- profiling (HIP events on the context's stream) ------------------------------------ */
int natac_profile_enable(natac_ctx *ctx, int on);
/* total milliseconds and launch count of kernel class `k` since the last reset */
int natac_profile_get(natac_ctx *ctx, int k, double *ms_total, int64_t *launches);
int natac_profile_reset(natac_ctx *ctx);
/* Resident tracks between the stages of ONE process (`nucleoatac run` = occ -> vprocess -> nuc -> merge -> nfr, cli.py:34-64 of the
 * reference).  The reference hands the occupancy tracks from `occ` to `nuc` / `nfr` through files: Track.write_track + bgzip, then
 * tabix reads per chunk (NucChunk.getOcc, NucleosomeCalling.py:284-293; NFRChunk.getOcc, NFRCalling.py:64-67).  Inside one process the
 * values can stay in HBM instead -- exactly the values a reader of the file would get:
 *   natac_store_adopt   a COPY of the batch's tracks as the file shows them: every run rounded to its twelve printed digits
 *                       (float('%.12g' % v)), NaN where Track.write_track writes no line (write_zero as in natac_batch_format_track);
 *                       returns the segment id, or -1 with *n_hard > 0 when a value cannot be rounded exactly on the device
 *                       (|v| < 1e-11, >= 1e34): nothing is kept and the caller reads the file for these regions; -1 with
                       *n_hard == -1 when the store's HBM budget declines the segment (below) -- same consequence;
 *   natac_store_set_budget  the store never fills the device: a segment is adopted only while the store stays below max_bytes
 *                       (< 0: no cap; env NATAC_STORE_MAX_BYTES) AND the device keeps min_free_bytes for the pipeline's batches
 *                       (< 0: a quarter of the device's memory; env NATAC_STORE_MIN_FREE_BYTES), counting the blocks the library
 *                       caches as free.  The first refusal closes the store: later sub-batches go through the files unasked;
 *   natac_store_read    ranges [offset, offset + length) of slot `slot` (the i-th adopted track) of the named segments, concatenated
 *                       into `out` (host): whole chunks for nfr's gap statistics, single positions for nuc's calls.
 *   natac_store_declined  how many segments the budget declined.
 * Offsets are positions in the batch's flat per-base layout (chunk k starts at out_off[k]).  Thread-safe. */
typedef struct natac_store natac_store;
int natac_store_create(natac_store **out);
void natac_store_free(natac_store *s);
int natac_store_adopt(natac_store *s, natac_batch *b, int32_t n_tracks, const int32_t *tracks, int write_zero, int64_t *segment,
                      int32_t *n_hard);
int natac_store_read(natac_store *s, natac_ctx *ctx, int64_t n, const int64_t *segment, const int64_t *offset, const int64_t *length,
                     int32_t slot, double *out, size_t out_values);
int natac_store_info(natac_store *s, int64_t *n_segments, int64_t *bytes);
int natac_store_set_budget(natac_store *s, int64_t max_bytes, int64_t min_free_bytes);
int natac_store_declined(natac_store *s, int64_t *n_declined);

/* Shader-clock trace (measurement aid, SURVEY.md section 8d asks for achieved rates against peaks that assume a clock): a one-wave
 * sampler kernel on its own stream notes (wall time, shader cycle counter) every interval_us while other launches run; between
 * two samples cycles / time = the clock the chip ran at.  _stop ends it and returns the number of samples and of profiled launches
 * (natac_profile_enable) that fell into the trace; _fetch returns the samples (ms since the trace start, cycle counter) and for every
 * such launch its NATAC_K_* class and its start / end on the same time axis. */
int natac_clock_trace_start(natac_ctx *ctx, int max_samples, int interval_us);
int natac_clock_trace_stop(natac_ctx *ctx, int64_t *n_samples, int64_t *n_intervals);
int natac_clock_trace_fetch(natac_ctx *ctx, int64_t n_samples, double *t_ms, double *cycles, int64_t n_intervals, int32_t *iv_kernel,
                            double *iv_t0_ms, double *iv_t1_ms);
/* stream-ordered timer: natac_timer_start records an event, natac_timer_stop records + syncs + returns ms */
int natac_timer_start(natac_ctx *ctx);
int natac_timer_stop(natac_ctx *ctx, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* NATAC_H */
