// natac_store.hpp -- tracks that stay in HBM between the stages of one process (natac_store_*): a batch's finished tracks are adopted as the
// values their file would hold (natac_textz.hpp: tz_as_written) and later stages read regions of them instead of the files.
#pragma once
#include "natac_trackio.hpp"

struct natac_store {
    struct Seg { PoolBuf<double> p[4]; int n_tracks; long long n; int device; };
    std::mutex mu;
    std::vector<Seg> segs;
    // HBM budget: the store is a convenience next to the files, it must never be what fills the device.  A segment is adopted only
    // while the store stays below max_bytes AND the device keeps min_free bytes (default: a quarter of its memory) for the batches
    // of the pipeline; the first refusal closes the store (later sub-batches go through the files without asking again).
    long long bytes = 0, max_bytes = -1, min_free = -1, declined = 0;
    bool closed = false;
};

extern "C" {

int natac_store_create(natac_store **out) {
    if (!out) return fail(NATAC_E_ARG, "out is NULL");
    natac_store *s = new natac_store();
    const char *e = getenv("NATAC_STORE_MAX_BYTES");
    if (e && *e) s->max_bytes = atoll(e);
    e = getenv("NATAC_STORE_MIN_FREE_BYTES");
    if (e && *e) s->min_free = atoll(e);
    *out = s;
    return NATAC_OK;
}

int natac_store_set_budget(natac_store *s, int64_t max_bytes, int64_t min_free_bytes) {
    if (!s) return fail(NATAC_E_ARG, "store is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    s->max_bytes = max_bytes;
    s->min_free = min_free_bytes;
    s->closed = false;
    return NATAC_OK;
}

void natac_store_free(natac_store *s) {
    delete s;
}

int natac_store_adopt(natac_store *s, natac_batch *b, int32_t n_tracks, const int32_t *tracks, int write_zero, int64_t *segment,
                      int32_t *n_hard) {
    using namespace natac_textz;
    if (!s || !b || !tracks || !segment || n_tracks < 1 || n_tracks > 4) return fail(NATAC_E_ARG, "bad argument");
    *segment = -1;
    if (n_hard) *n_hard = 0;
    natac_ctx *c = b->ctx;
    int rc;
    for (int i = 0; i < n_tracks; ++i) {
        if (tracks[i] == NATAC_T_INS) return fail(NATAC_E_ARG, "float64 tracks only");
        if ((rc = need_track(b, tracks[i]))) return rc;
    }
    HIPCHK(hipSetDevice(c->device));
    if (b->total_bp >= 0xffffffffLL) return fail(NATAC_E_ARG, "batch too long (%lld bases)", b->total_bp);
    {   // budget first: nothing is launched or allocated for a segment the store will not keep
        const long long need = (long long)n_tracks * b->total_bp * (long long)sizeof(double);
        size_t avail = 0, total = 0;
        HIPCHK(pool_mem_info(c->device, &avail, &total));
        std::lock_guard<std::mutex> lk(s->mu);
        const long long min_free = s->min_free >= 0 ? s->min_free : (long long)(total / 4);
        // run tables + one pass of scratch ride on top of the segment itself while it is formed
        const long long scratch = 2 * b->total_bp * (long long)sizeof(int) + (1 << 20);
        if (s->closed || (s->max_bytes >= 0 && s->bytes + need > s->max_bytes) || (long long)avail - need - scratch < min_free) {
            s->closed = true;
            ++s->declined;
            if (n_hard) *n_hard = -1;      // declined: budget (the caller reads the files, as for n_hard > 0)
            return NATAC_OK;
        }
    }
    if ((rc = ensure_text_tables(c))) return rc;
    HIPCHK(sync_all(c));
    // declared before the scope: an early exit drains the stream before the segment's tracks and the run tables go back
    natac_store::Seg seg{{}, n_tracks, b->total_bp, c->device};
    PoolBuf<unsigned int> d_R;
    PoolBuf<int> d_C;
    int hard = 0;
    DeviceCall dc(c, "store_adopt");
    const int nt = b->n_tiles256;
    int *d_hard = dc.zeroed<int>(1), *d_tc = dc.alloc<int>((size_t)nt);
    unsigned long long *d_tb = dc.alloc<unsigned long long>((size_t)nt + 1);
    for (int i = 0; i < n_tracks && dc.ok(); ++i) {
        TextJob job;
        job.vals = b->d_track[tracks[i]]; job.out_off = b->d_out_off; job.chunk_len = b->d_len; job.tiles = b->d_tiles256; job.ntiles = nt;
        job.chrom_id = nullptr; job.chunk_start = nullptr; job.names = nullptr; job.name_off = nullptr; job.p10 = c->d_p10;
        job.write_zero = write_zero & 1; job.keep_before_nan = (write_zero >> 1) & 1;
        hipLaunchKernelGGL(tz_flags_count, dim3(nt), dim3(256), 0, c->stream, job, d_tc);
        dev_scan(c, d_tc, (long long)nt, d_tb, dc);
        unsigned long long nruns = 0;
        dc.fetch(&nruns, d_tb + nt, 1);
        if ((rc = dc.sync())) return rc;
        d_R.reset(); d_C.reset();
        if ((rc = dev_alloc(d_R, (size_t)nruns)) || (rc = dev_alloc(d_C, (size_t)nruns))) return rc;
        hipLaunchKernelGGL(tz_scatter_runs, dim3(nt), dim3(256), 0, c->stream, job, d_tb, d_R, d_C);
        if ((rc = dev_alloc(seg.p[i], (size_t)b->total_bp))) return rc;
        hipLaunchKernelGGL(tz_as_written, dim3((unsigned)((nruns + 255) / 256)), dim3(256), 0, c->stream, job, (long long)nruns, d_R, d_C,
                           seg.p[i], d_hard);
        dc.launched();
    }
    dc.fetch(&hard, d_hard, 1);
    if ((rc = dc.finish())) return rc;
    if (n_hard) *n_hard = hard;
    // a value the device cannot round like the text round trip would: nothing is adopted (the tracks go back), the caller reads the file
    if (hard) return NATAC_OK;
    std::lock_guard<std::mutex> lk(s->mu);
    s->segs.push_back(std::move(seg));
    s->bytes += (long long)n_tracks * b->total_bp * (long long)sizeof(double);
    *segment = (int64_t)s->segs.size() - 1;
    return NATAC_OK;
}

int natac_store_read(natac_store *s, natac_ctx *c, int64_t n, const int64_t *segment, const int64_t *offset, const int64_t *length,
                     int32_t slot, double *out, size_t out_values) {
    using namespace natac_textz;
    if (!s || !c || n < 0 || (n > 0 && (!segment || !offset || !length || !out))) return fail(NATAC_E_ARG, "null argument");
    if (n == 0) return NATAC_OK;
    DeviceCall dc(c, "store_read");
    if (!dc.ok()) return dc.finish();
    std::vector<StoreRegion> reg((size_t)n);
    long long total = 0;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        for (int64_t j = 0; j < n; ++j) {
            if (segment[j] < 0 || segment[j] >= (int64_t)s->segs.size()) return fail(NATAC_E_ARG, "region %lld: no segment %lld", (long long)j, (long long)segment[j]);
            const natac_store::Seg &g = s->segs[(size_t)segment[j]];
            if (slot < 0 || slot >= g.n_tracks) return fail(NATAC_E_ARG, "segment %lld holds %d tracks", (long long)segment[j], g.n_tracks);
            if (g.device != c->device) return fail(NATAC_E_ARG, "segment %lld lives on device %d", (long long)segment[j], g.device);
            if (offset[j] < 0 || length[j] < 0 || offset[j] + length[j] > g.n)
                return fail(NATAC_E_ARG, "region %lld: [%lld, +%lld) outside its segment (%lld values)", (long long)j, (long long)offset[j], (long long)length[j], g.n);
            reg[(size_t)j] = {g.p[slot] + offset[j], total, (long long)length[j]};
            total += length[j];
        }
    }
    if ((size_t)total != out_values) return fail(NATAC_E_ARG, "destination holds %zu values, the regions %lld", out_values, total);
    if (total == 0) return NATAC_OK;
    const StoreRegion *d_reg = dc.upload(reg.data(), reg.size());
    double *d_out = dc.alloc<double>((size_t)total);
    if (dc.ok()) {
        hipLaunchKernelGGL(tz_store_gather, dim3((unsigned)n), dim3(256), 0, c->stream, d_reg, d_out);
        dc.launched();
    }
    dc.fetch(out, d_out, (size_t)total);
    return dc.finish();
}

int natac_store_info(natac_store *s, int64_t *n_segments, int64_t *bytes) {
    if (!s) return fail(NATAC_E_ARG, "store is NULL");
    std::lock_guard<std::mutex> lk(s->mu);
    long long by = 0;
    for (auto &g : s->segs) by += (long long)g.n_tracks * g.n * (long long)sizeof(double);
    if (n_segments) *n_segments = (int64_t)s->segs.size();
    if (bytes) *bytes = by;
    return NATAC_OK;
}

int natac_store_declined(natac_store *s, int64_t *n_declined) {
    if (!s || !n_declined) return fail(NATAC_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    *n_declined = s->declined;
    return NATAC_OK;
}

}  // extern "C"
