// natac_profile.hpp -- what measures the library from inside: the event profile per kernel kind (natac_profile_*; prof_begin / prof_end
// in natac_runtime.hpp feed it), the stream timer (natac_timer_*) and the shader-clock trace (natac_clock_trace_*) with its sampler kernel.
#pragma once
#include "natac_runtime.hpp"

// one wave; lane 0 notes (constant-rate wall ticks since its start, shader cycle counter) every `interval` wall ticks and sleeps in
// between: the slope between two samples is the clock the CU ran at -- under whatever else the chip is executing meanwhile
__global__ void __launch_bounds__(64) natac_clock_sampler(long long *__restrict__ buf, int cap, long long interval) {
    if (threadIdx.x) return;
    const long long w0 = wall_clock64();
    long long next = w0;
    int i = 0;
    for (; i < cap; ++i) {
        long long w;
        do {
            __builtin_amdgcn_s_sleep(64);
            w = wall_clock64();
        } while (w < next);
        buf[2 + 2 * i] = w - w0;
        buf[3 + 2 * i] = clock64();
        next = w + interval;
        if (__hip_atomic_load(buf + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) { ++i; break; }
    }
    buf[0] = i;
}

extern "C" {

int natac_profile_enable(natac_ctx *c, int on) {
    if (!c) return fail(NATAC_E_ARG, "ctx is NULL");
    c->profiling = on != 0;
    return NATAC_OK;
}
int natac_profile_get(natac_ctx *c, int k, double *ms_total, int64_t *launches) {
    if (!c || k < 0 || k >= NATAC_K_COUNT) return fail(NATAC_E_ARG, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    prof_collect(c);
    if (ms_total) *ms_total = c->prof_ms[k];
    if (launches) *launches = c->prof_n[k];
    return NATAC_OK;
}
int natac_profile_reset(natac_ctx *c) {
    if (!c) return fail(NATAC_E_ARG, "ctx is NULL");
    HIPCHK(sync_all(c));
    prof_collect(c);
    for (int i = 0; i < NATAC_K_COUNT; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; }
    return NATAC_OK;
}
int natac_timer_start(natac_ctx *c) {
    if (!c) return fail(NATAC_E_ARG, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->t0, c->stream));
    return NATAC_OK;
}
int natac_timer_stop(natac_ctx *c, double *ms) {
    if (!c || !ms) return fail(NATAC_E_ARG, "null argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->t1, c->stream));
    HIPCHK(hipEventSynchronize(c->t1));
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, c->t0, c->t1));
    *ms = f;
    prof_collect(c);
    return NATAC_OK;
}

/* ---------------- shader-clock trace ---------------- */

int natac_clock_trace_start(natac_ctx *c, int max_samples, int interval_us) {
    if (!c || max_samples < 2 || interval_us < 1) return fail(NATAC_E_ARG, "bad argument");
    if (c->ck_active) return fail(NATAC_E_STATE, "a clock trace is already running");
    HIPCHK(hipSetDevice(c->device));
    int khz = 0;
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    if (khz <= 0) return fail(NATAC_E_HIP, "the device reports no wall clock rate");
    if (!c->ck_stream) HIPCHK(hipStreamCreateWithFlags(&c->ck_stream, hipStreamNonBlocking));
    if (!c->ck_start) HIPCHK(hipEventCreate(&c->ck_start));
    if (c->ck_cap < max_samples) {
        if (c->d_ck) (void)hipFree(c->d_ck);
        c->d_ck = nullptr;
        HIPCHK(hipMalloc((void **)&c->d_ck, (2 + 2 * (size_t)max_samples) * sizeof(long long)));
        c->ck_cap = max_samples;
    }
    HIPCHK(hipMemsetAsync(c->d_ck, 0, 2 * sizeof(long long), c->ck_stream));
    HIPCHK(hipEventRecord(c->ck_start, c->ck_stream));
    hipLaunchKernelGGL(natac_clock_sampler, dim3(1), dim3(64), 0, c->ck_stream, c->d_ck, max_samples,
                       (long long)khz * interval_us / 1000);
    HIPCHK(hipGetLastError());
    c->ck_iv.clear();
    c->ck_active = true;
    return NATAC_OK;
}

int natac_clock_trace_stop(natac_ctx *c, int64_t *n_samples, int64_t *n_intervals) {
    if (!c) return fail(NATAC_E_ARG, "ctx is NULL");
    if (!c->ck_active) return fail(NATAC_E_STATE, "no clock trace is running");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    prof_collect(c);                     // intervals of the launches profiled since the start
    const long long one = 1;
    HIPCHK(hipMemcpy(c->d_ck + 1, &one, sizeof one, hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(c->ck_stream));
    long long n = 0;
    HIPCHK(hipMemcpy(&n, c->d_ck, sizeof n, hipMemcpyDeviceToHost));
    c->ck_active = false;
    if (n_samples) *n_samples = n;
    if (n_intervals) *n_intervals = (int64_t)c->ck_iv.size();
    return NATAC_OK;
}

int natac_clock_trace_fetch(natac_ctx *c, int64_t n_samples, double *t_ms, double *cycles, int64_t n_intervals, int32_t *iv_kernel,
                            double *iv_t0_ms, double *iv_t1_ms) {
    if (!c || (n_samples > 0 && (!t_ms || !cycles)) || (n_intervals > 0 && (!iv_kernel || !iv_t0_ms || !iv_t1_ms)))
        return fail(NATAC_E_ARG, "null argument");
    if (c->ck_active) return fail(NATAC_E_STATE, "stop the clock trace first");
    if (n_samples > c->ck_cap || n_intervals > (int64_t)c->ck_iv.size()) return fail(NATAC_E_ARG, "more than was recorded");
    HIPCHK(hipSetDevice(c->device));
    int khz = 0;
    HIPCHK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    std::vector<long long> h(2 * (size_t)n_samples);
    if (n_samples) HIPCHK(hipMemcpy(h.data(), c->d_ck + 2, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n_samples; ++i) {
        t_ms[i] = (double)h[2 * i] / (double)khz;
        cycles[i] = (double)h[2 * i + 1];
    }
    for (int64_t i = 0; i < n_intervals; ++i) {
        iv_kernel[i] = c->ck_iv[(size_t)i].k;
        iv_t0_ms[i] = c->ck_iv[(size_t)i].t0;
        iv_t1_ms[i] = c->ck_iv[(size_t)i].t1;
    }
    return NATAC_OK;
}

}  // extern "C"
