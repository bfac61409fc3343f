// natac_dropins.hpp -- the per-call entry points over kernels of natac_kernels.hpp: the drop-ins for the reference's Cython functions
// (natac_make_fragment_mat, natac_get_insertions, natac_get_stranded_insertions, natac_fragment_sizes, natac_calculate_cov) and the
// operator-level calls (natac_smooth, natac_make_bias_mat, natac_pwm_bias, natac_correlate_valid, natac_calculate_occupancy).
// Each is one DeviceCall: operands up, the launch, the result down.
#pragma once
#include "natac_runtime.hpp"

using namespace natac;

extern "C" {

/* ---------------- Cython-function drop-ins ---------------- */

int natac_make_fragment_mat(natac_ctx *c, int64_t nf, const int64_t *l, const int32_t *n, int64_t start, int64_t end, int lower,
                            int upper, double *mat) {
    if (!c || !mat || (nf > 0 && (!l || !n))) return fail(NATAC_E_ARG, "null argument");
    if (end <= start || upper <= lower) return fail(NATAC_E_ARG, "empty matrix");
    if (nf < 0) return fail(NATAC_E_ARG, "negative size");
    const long long ncol = end - start, nrow = upper - lower;
    if (ncol > 0x7fffffffLL) return fail(NATAC_E_ARG, "region too long");
    DeviceCall dc(c, "make_fragment_mat");
    const long long *d_l = dc.upload((const long long *)l, (size_t)nf);
    const int *d_n = dc.upload(n, (size_t)nf);
    double *d_m = dc.zeroed<double>((size_t)(nrow * ncol));
    if (dc.ok() && nf > 0) {
        int blocks = (int)std::min<long long>((nf + 255) / 256, 4096);
        hipLaunchKernelGGL(natac_fragment_mat, dim3(blocks), dim3(256), 0, c->stream, d_l, d_n, (long long)nf, (long long)start,
                           (int)ncol, lower, (int)nrow, d_m);
        dc.launched();
    }
    dc.fetch(mat, d_m, (size_t)(nrow * ncol));
    return dc.finish();
}

int natac_get_insertions(natac_ctx *c, int64_t nf, const int64_t *l, const int32_t *n, int64_t start, int64_t end, int lower,
                         int upper, double *out) {
    if (!c || !out || (nf > 0 && (!l || !n))) return fail(NATAC_E_ARG, "null argument");
    if (nf < 0) return fail(NATAC_E_ARG, "negative size");
    if (end <= start) return fail(NATAC_E_ARG, "empty region");
    const long long npos = end - start;
    if (npos > 0x7fffffffLL) return fail(NATAC_E_ARG, "region too long");
    DeviceCall dc(c, "get_insertions");
    const long long *d_l = dc.upload((const long long *)l, (size_t)nf);
    const int *d_n = dc.upload(n, (size_t)nf);
    int *d_i = dc.zeroed<int>((size_t)npos);
    double *d_o = dc.alloc<double>((size_t)npos);
    if (dc.ok()) {
        if (nf > 0) {
            int blocks = (int)std::min<long long>((nf + 255) / 256, 4096);
            hipLaunchKernelGGL(natac_insertions_region, dim3(blocks), dim3(256), 0, c->stream, d_l, d_n, (long long)nf,
                               (long long)start, (int)npos, lower, upper, d_i);
        }
        int blocks = (int)std::min<long long>((npos + 255) / 256, 4096);
        hipLaunchKernelGGL(natac_i32_to_f64, dim3(blocks), dim3(256), 0, c->stream, d_i, d_o, npos);
        dc.launched();
    }
    dc.fetch(out, d_o, (size_t)npos);
    return dc.finish();
}

int natac_get_stranded_insertions(natac_ctx *c, int64_t nf, const int64_t *l, const int32_t *n, int64_t start, int64_t end, int lower,
                                  int upper, double *plus, double *minus) {
    if (!c || !plus || !minus || (nf > 0 && (!l || !n))) return fail(NATAC_E_ARG, "null argument");
    if (nf < 0) return fail(NATAC_E_ARG, "negative size");
    if (end <= start) return fail(NATAC_E_ARG, "empty region");
    const long long npos = end - start;
    if (npos > 0x3fffffffLL) return fail(NATAC_E_ARG, "region too long");
    DeviceCall dc(c, "get_stranded_insertions");
    const long long *d_l = dc.upload((const long long *)l, (size_t)nf);
    const int *d_n = dc.upload(n, (size_t)nf);
    int *d_i = dc.zeroed<int>((size_t)2 * npos);
    double *d_o = dc.alloc<double>((size_t)2 * npos);
    if (dc.ok()) {
        if (nf > 0) {
            int blocks = (int)std::min<long long>((nf + 255) / 256, 4096);
            hipLaunchKernelGGL(natac_stranded_insertions_region, dim3(blocks), dim3(256), 0, c->stream, d_l, d_n, (long long)nf,
                               (long long)start, (int)npos, lower, upper, d_i, d_i + npos);
        }
        int blocks = (int)std::min<long long>((2 * npos + 255) / 256, 4096);
        hipLaunchKernelGGL(natac_i32_to_f64, dim3(blocks), dim3(256), 0, c->stream, d_i, d_o, 2 * npos);
        dc.launched();
    }
    dc.fetch(plus, d_o, (size_t)npos);
    dc.fetch(minus, d_o + npos, (size_t)npos);
    return dc.finish();
}

int natac_fragment_sizes(natac_ctx *c, int64_t nf, const int64_t *l, const int32_t *n, int32_t nchunks, const int64_t *cs,
                         const int64_t *ce, int lower, int upper, double *sizes) {
    if (!c || !sizes || (nf > 0 && (!l || !n)) || (nchunks > 0 && (!cs || !ce))) return fail(NATAC_E_ARG, "null argument");
    if (upper <= lower) return fail(NATAC_E_ARG, "upper <= lower");
    if (nf < 0 || nchunks < 0) return fail(NATAC_E_ARG, "negative size");
    const int nb = upper - lower;
    if (nb > (1 << 20)) return fail(NATAC_E_ARG, "size range too wide");
    // chunk starts and ends sorted independently: #{cs <= x} - #{ce <= x} chunks contain x (see natac_size_hist);
    // an inverted interval (end < start) contains nothing, like the reference's `center >= start and center < end`
    std::vector<long long> hs((size_t)nchunks), he((size_t)nchunks);
    for (int k = 0; k < nchunks; ++k) { hs[k] = cs[k]; he[k] = std::max<long long>(ce[k], cs[k]); }
    std::sort(hs.begin(), hs.end());
    std::sort(he.begin(), he.end());
    DeviceCall dc(c, "fragment_sizes");
    const long long *d_l = dc.upload((const long long *)l, (size_t)nf);
    const int *d_n = dc.upload(n, (size_t)nf);
    const long long *d_cs = dc.upload(hs.data(), (size_t)nchunks), *d_ce = dc.upload(he.data(), (size_t)nchunks);
    unsigned long long *d_h = dc.zeroed<unsigned long long>((size_t)nb);
    std::vector<unsigned long long> h((size_t)nb, 0);
    if (dc.ok() && nf > 0 && nchunks > 0) {
        dc.prof_begin(NATAC_K_SIZE_HIST);
        const long long nseg = (nf + SIZE_SEG - 1) / SIZE_SEG;
        const int blocks = (int)std::min<long long>(nseg, 8192);
        const int use_lds = nb <= 8192 ? 1 : 0;
        const size_t lds = (size_t)2 * SIZE_STAGE * sizeof(long long) + (use_lds ? (size_t)nb * sizeof(unsigned) : 0);
        hipLaunchKernelGGL(natac_size_hist, dim3(blocks), dim3(256), lds, c->stream, d_l, d_n, (long long)nf, d_cs, d_ce, (int)nchunks,
                           lower, upper, use_lds, d_h);
        dc.prof_end();
        dc.launched();
    }
    dc.fetch(h.data(), d_h, (size_t)nb);
    const int rc = dc.finish();
    if (rc) return rc;
    for (int i = 0; i < nb; ++i) sizes[i] = (double)h[i];
    return NATAC_OK;
}

int natac_calculate_cov(natac_ctx *c, const double *p, const double *v, int64_t n, int r, int mode, double *out) {
    if (!c || !p || !v || !out) return fail(NATAC_E_ARG, "null argument");
    if (n <= 0) return fail(NATAC_E_ARG, "p and v must be non-empty");
    if (mode != 0 && mode != 1) return fail(NATAC_E_ARG, "mode must be 0 (closed form) or 1 (literal)");
    DeviceCall dc(c, "calculate_cov");
    const double *d_p = dc.upload(p, (size_t)n), *d_v = dc.upload(v, (size_t)n);
    const int blocks = mode == 0 ? (int)std::min<int64_t>((n + 255) / 256, 1024) : (int)std::min<int64_t>(n, 4096);
    double *d_part = dc.alloc<double>((size_t)2 * blocks);
    std::vector<double> part((size_t)2 * blocks);
    if (dc.ok()) {
        if (mode == 0)
            hipLaunchKernelGGL(natac_cov_closed, dim3(blocks), dim3(256), 0, c->stream, d_p, d_v, (long long)n, d_part);
        else
            hipLaunchKernelGGL(natac_cov_literal, dim3(blocks), dim3(256), 0, c->stream, d_p, d_v, (long long)n, d_part);
        dc.launched();
    }
    dc.fetch(part.data(), d_part, (size_t)(mode == 0 ? 2 : 1) * blocks);
    const int rc = dc.finish();
    if (rc) return rc;
    if (mode == 0) {
        double s1 = 0, s2 = 0;
        for (int i = 0; i < blocks; ++i) { s1 += part[2 * i]; s2 += part[2 * i + 1]; }
        *out = (s1 - s2 * s2) * r;
    } else {
        double s = 0;
        for (int i = 0; i < blocks; ++i) s += part[i];
        *out = s * r;
    }
    return NATAC_OK;
}

/* ---------------- operator-level entry points ---------------- */

int natac_smooth(natac_ctx *c, const double *x, int64_t n, const double *w, int M, int mode, int norm, double *out) {
    if (!c || !x || !w || !out) return fail(NATAC_E_ARG, "null argument");
    if (M < 1 || M % 2 != 1) return fail(NATAC_E_ARG, "window length must be odd (got %d)", M);
    if (mode != 0 && mode != 1) return fail(NATAC_E_ARG, "mode must be 0 (valid) or 1 (same)");
    if (n < M) return fail(NATAC_E_ARG, "signal (%lld) shorter than the window (%d)", (long long)n, M);
    const long long nout = mode == 0 ? n - M + 1 : n;
    DeviceCall dc(c, "smooth");
    const double *d_x = dc.upload(x, (size_t)n), *d_w = dc.upload(w, (size_t)M);
    double *d_y = dc.alloc<double>((size_t)nout);
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_smooth1d, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, c->stream, d_x, (long long)n, d_w, M, mode,
                           norm, d_y, nout);
        dc.launched();
    }
    dc.fetch(out, d_y, (size_t)nout);
    return dc.finish();
}

int natac_make_bias_mat(natac_ctx *c, const double *bias_log, int64_t nb, int64_t track_start, int64_t start, int64_t end,
                        int lower, int upper, double *mat) {
    if (!c || !bias_log || !mat) return fail(NATAC_E_ARG, "null argument");
    if (nb < 0) return fail(NATAC_E_ARG, "negative size");
    if (end <= start || upper <= lower || lower < 0) return fail(NATAC_E_ARG, "empty matrix");
    const long long ncol = end - start, nrow = upper - lower;
    if (ncol > 0x7fffffffLL) return fail(NATAC_E_ARG, "region too long");
    DeviceCall dc(c, "make_bias_mat");
    const double *d_b = dc.upload(bias_log, (size_t)nb);
    double *d_m = dc.alloc<double>((size_t)(nrow * ncol));
    int *d_oob = dc.zeroed<int>(1), oob = 0;
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_bias_mat_dense, dim3((unsigned)((nrow * ncol + 255) / 256)), dim3(256), 0, c->stream, d_b, (long long)nb,
                           (long long)(start - track_start), (int)ncol, lower, (int)nrow, d_m, d_oob);
        dc.launched();
    }
    dc.fetch(mat, d_m, (size_t)(nrow * ncol));
    dc.fetch(&oob, d_oob, 1);
    const int rc = dc.finish();
    if (rc) return rc;
    if (oob) return fail(NATAC_E_ARG, "bias track does not cover [start - upper//2, end + upper//2)");
    return NATAC_OK;
}

int natac_pwm_bias(natac_ctx *c, const uint8_t *seq, int64_t n, const double *log_pwm, const uint8_t *nucleotides, int nrow, int K,
                   double *out) {
    if (!c || !seq || !log_pwm || !nucleotides || !out) return fail(NATAC_E_ARG, "null argument");
    if (nrow < 1 || K < 1 || n < K) return fail(NATAC_E_ARG, "sequence shorter than the PWM");
    const long long nout = n - K + 1;
    DeviceCall dc(c, "pwm_bias");
    const unsigned char *d_s = dc.upload((const unsigned char *)seq, (size_t)n);
    const unsigned char *d_n = dc.upload((const unsigned char *)nucleotides, (size_t)nrow);
    const double *d_p = dc.upload(log_pwm, (size_t)nrow * K);
    double *d_o = dc.alloc<double>((size_t)nout);
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_pwm_score, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, c->stream, d_s, (long long)n, d_p, d_n, nrow, K,
                           d_o);
        dc.launched();
    }
    dc.fetch(out, d_o, (size_t)nout);
    return dc.finish();
}

int natac_correlate_valid(natac_ctx *c, const double *sub, int64_t ncol, const double *vmat, int R, int W, double *out) {
    if (!c || !sub || !vmat || !out) return fail(NATAC_E_ARG, "null argument");
    if (R < 1 || W < 1 || ncol < W) return fail(NATAC_E_ARG, "matrix narrower than the template");
    const long long nout = ncol - W + 1;
    DeviceCall dc(c, "correlate_valid");
    const double *d_s = dc.upload(sub, (size_t)R * ncol), *d_v = dc.upload(vmat, (size_t)R * W);
    double *d_o = dc.alloc<double>((size_t)nout);
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_correlate_dense, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, c->stream, d_s, (long long)ncol, d_v, R, W,
                           d_o, nout);
        dc.launched();
    }
    dc.fetch(out, d_o, (size_t)nout);
    return dc.finish();
}

int natac_calculate_occupancy(natac_ctx *c, const double *inserts, const double *bias, double *out) {
    if (!c || !inserts || !bias || !out) return fail(NATAC_E_ARG, "null argument");
    if (!c->have_occ) return fail(NATAC_E_STATE, "natac_set_occ_model has not been called");
    DeviceCall dc(c, "calculate_occupancy");
    const double *d_i = dc.upload(inserts, (size_t)c->occ_upper), *d_b = dc.upload(bias, (size_t)c->occ_upper);
    double *d_o = dc.alloc<double>(3);
    int *d_s = dc.alloc<int>(1), st = 0;
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_occupancy_single, dim3(1), dim3(128), 0, c->stream, d_i, d_b, make_occ(c), d_o, d_s);
        dc.launched();
    }
    dc.fetch(out, d_o, 3);
    dc.fetch(&st, d_s, 1);
    const int rc = dc.finish();
    if (rc) return rc;
    if (st) return fail(NATAC_E_ARG, "no alpha passes the likelihood-ratio test");
    return NATAC_OK;
}

}  // extern "C"
