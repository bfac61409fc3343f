// natac_trackio.hpp -- the host side of the track files: the device track writer (natac_batch_format_*: the kernels of natac_textz.hpp
// form a batch's bedGraph text and its BGZF members, natac_tbi_* collects their tabix records), its host counterparts
// (natac_format_doubles, natac_bgzf_lines_host, natac_write_bed*, natac_bgzip_file, natac_tabix_index) and the indexed reader (natac_tbx_*).
#pragma once
#include "natac_runtime.hpp"
#include "natac_cores.hpp"
#include "natac_tabix.hpp"
#include "natac_writer.hpp"

#include <cstring>
#include <thread>

using namespace natac;

/* ---------------- device-side track writer (natac_textfmt.hpp, natac_deflate.hpp, natac_textz.hpp) ---------------- */

static int ensure_text_tables(natac_ctx *c) {
    if (c->d_p10 && c->d_crc) return NATAC_OK;
    int rc;
    if (!c->d_p10 && (rc = dev_upload(c, c->d_p10, natac_text::H_P10, sizeof(natac_text::H_P10) / sizeof(natac_text::P10)))) return rc;
    if (!c->d_crc) {
        natac_deflate::CrcTables t;
        natac_deflate::crc_init(t);
        if ((rc = dev_upload(c, c->d_crc, &t, 1))) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return NATAC_OK;
}

// text / BGZF of a device array of per-base values laid out like the batch's tracks.  Result stays in b->d_fmt_out.
static int format_values(natac_batch *b, const double *d_vals, const int32_t *chrom_id, const char *const *names, int32_t n_names,
                         const int64_t *chunk_start, int write_zero, int compress, int64_t *n_bytes, int64_t *n_text_bytes, int64_t *n_lines,
                         int32_t *n_hard) {
    using namespace natac_textz;
    natac_ctx *c = b->ctx;
    int rc = ensure_text_tables(c);
    if (rc) return rc;
    b->d_fmt_out.reset();
    b->fmt_bytes = -1;
    b->fmt_groups.clear();
    b->fmt_member_pos.clear();
    b->fmt_names.assign(names, names + n_names);
    // name table
    std::vector<char> cat;
    std::vector<int> noff(1, 0);
    for (int i = 0; i < n_names; ++i) {
        const size_t l = names[i] ? strlen(names[i]) : 0;
        if (l == 0 || l > 64) return fail(NATAC_E_ARG, "chromosome name %d must have 1..64 characters", i);
        cat.insert(cat.end(), names[i], names[i] + l);
        noff.push_back((int)cat.size());
    }
    // longest line this call can form: name + two coordinates + value text + 4 separators.  tz_write_lines stages the 256 lines of a
    // workgroup in LDS; sized for THIS bound (typically ~52 bytes per line) instead of the format's 160 it keeps 8 waves per SIMD
    // resident instead of 3.
    size_t max_name = 0;
    long long max_coord = 0, min_coord = 0;
    for (int i = 0; i < b->nc; ++i) {
        if (chrom_id[i] < 0 || chrom_id[i] >= n_names) return fail(NATAC_E_ARG, "chunk %d: chromosome id %d out of range", i, chrom_id[i]);
        max_name = std::max(max_name, (size_t)(noff[chrom_id[i] + 1] - noff[chrom_id[i]]));
        max_coord = std::max<long long>(max_coord, (long long)chunk_start[i] + b->h_len[i]);
        min_coord = std::min<long long>(min_coord, (long long)chunk_start[i]);
    }
    const int line_cap = std::min<int>(MAX_LINE, (int)max_name + 2 * std::max(natac_text::digits_i64(max_coord), natac_text::digits_i64(min_coord)) + VTXT + 4);
    if (b->total_bp >= 0xffffffffLL) return fail(NATAC_E_ARG, "batch too long for the device writer (%lld bases)", b->total_bp);
    DeviceCall dc(c, "format_track");
    char *d_names = dc.upload(cat.data(), cat.size());
    int *d_noff = dc.upload(noff.data(), noff.size());
    int *d_cid = dc.upload(chrom_id, (size_t)b->nc);
    long long *d_cs = dc.upload((const long long *)chunk_start, (size_t)b->nc);
    int *d_hard = dc.zeroed<int>(1);
    TextJob job;
    job.vals = d_vals; job.out_off = b->d_out_off; job.chunk_len = b->d_len; job.tiles = b->d_tiles256; job.ntiles = b->n_tiles256;
    job.chrom_id = d_cid; job.chunk_start = d_cs; job.names = d_names; job.name_off = d_noff; job.p10 = c->d_p10;
    job.write_zero = write_zero & 1; job.keep_before_nan = (write_zero >> 1) & 1;
    const int nt = b->n_tiles256;
    int *d_tc = dc.alloc<int>((size_t)nt);
    unsigned long long *d_tb = dc.alloc<unsigned long long>((size_t)nt + 1);
    if (dc.ok()) {
        hipLaunchKernelGGL(tz_flags_count, dim3(nt), dim3(256), 0, c->stream, job, d_tc);
        dev_scan(c, d_tc, (long long)nt, d_tb, dc);
    }
    unsigned long long nruns = 0;
    dc.fetch(&nruns, d_tb + nt, 1);
    if ((rc = dc.sync())) return rc;
    unsigned int *d_R = dc.alloc<unsigned int>((size_t)nruns);
    int *d_C = dc.alloc<int>((size_t)nruns);
    unsigned char *d_len8 = dc.alloc<unsigned char>((size_t)nruns);
    const unsigned rb = (unsigned)((nruns + 255) / 256);
    unsigned long long *d_vtxt = dc.alloc<unsigned long long>((size_t)nruns * (natac_textz::VTXT / 8));   // text of every run's value (tz_line_len -> tz_write_lines)
    unsigned long long *d_boff = dc.alloc<unsigned long long>((size_t)nruns + 1);
    unsigned long long *d_lidx = dc.alloc<unsigned long long>((size_t)nruns + 1);
    if (dc.ok()) {
        hipLaunchKernelGGL(tz_scatter_runs, dim3(nt), dim3(256), 0, c->stream, job, d_tb, d_R, d_C);
        hipLaunchKernelGGL(tz_line_len, dim3(rb), dim3(256), 0, c->stream, job, (long long)nruns, d_R, d_C, d_len8, d_hard, d_vtxt);
        dev_scan2(c, d_len8, (long long)nruns, d_boff, d_lidx, dc);
    }
    unsigned long long n_text = 0, nlines = 0;
    int hard = 0;
    dc.fetch(&n_text, d_boff + nruns, 1);
    dc.fetch(&nlines, d_lidx + nruns, 1);
    dc.fetch(&hard, d_hard, 1);
    if ((rc = dc.sync())) return rc;
    b->fmt_text_bytes = (long long)n_text;
    if (n_text_bytes) *n_text_bytes = (int64_t)n_text;
    if (n_lines) *n_lines = (int64_t)nlines;
    if (n_hard) *n_hard = hard;
    if (n_text == 0) { b->fmt_bytes = 0; if (n_bytes) *n_bytes = 0; return NATAC_OK; }
    unsigned char *d_text = nullptr;
    if (compress) {
        d_text = dc.alloc<unsigned char>((size_t)n_text + 64);
    } else {           // the text is the result: written in place (a failed call leaves fmt_bytes at -1)
        if ((rc = dev_alloc(b->d_fmt_out, (size_t)n_text + 64))) return rc;
        d_text = b->d_fmt_out;
    }
    long long *d_line_off = dc.alloc<long long>((size_t)nlines + 1);
    int *d_lcid = nullptr;
    long long *d_lbeg = nullptr, *d_lend = nullptr;
    if (compress) {
        d_lcid = dc.alloc<int>((size_t)nlines);
        d_lbeg = dc.alloc<long long>((size_t)nlines);
        d_lend = dc.alloc<long long>((size_t)nlines);
    }
    if (dc.ok()) {
        hipLaunchKernelGGL(tz_write_lines, dim3(rb), dim3(256), (size_t)256 * line_cap + 32, c->stream, job, (long long)nruns, d_R, d_C, d_len8, d_boff, d_lidx, d_vtxt, d_text,
                           d_line_off, d_lcid, d_lbeg, d_lend);
        dc.launched();
    }
    if (!compress) {
        if ((rc = dc.finish())) return rc;
        b->fmt_bytes = (long long)n_text;
        if (n_bytes) *n_bytes = (int64_t)n_text;
        return NATAC_OK;
    }
    namespace nd = natac_deflate;
    const long long nblk = ((long long)n_text + nd::BLK - 1) / nd::BLK;
    unsigned int *d_hist = dc.zeroed<unsigned int>((size_t)nd::NLL + nd::ND);
    // line segments per member -> offsets of the per-segment records pass A of the emit kernel leaves for its pass B
    unsigned int *d_nseg = dc.alloc<unsigned int>((size_t)nblk);
    unsigned long long *d_segbase = dc.alloc<unsigned long long>((size_t)nblk + 1);
    long long *d_k0 = dc.alloc<long long>((size_t)nblk);
    unsigned short *d_segbits = dc.alloc<unsigned short>((size_t)nlines + (size_t)nblk + 64);  // every line once + one more per straddled member border
    unsigned int *d_stage = dc.alloc<unsigned int>((size_t)nblk * STAGE_WORDS);                // the lines' finished bits between the emit kernel's two passes
    // token histogram of a sample of the members (every member of a small batch): natac_deflate.hpp, sample_stride
    const int stride = nd::sample_stride(nblk);
    const long long counted = (nblk + stride - 1) / stride;
    const size_t lds_count = 65536 + (nd::NLL + nd::ND) * sizeof(unsigned int);
    if (dc.ok()) {
        hipLaunchKernelGGL(tz_member_nseg, dim3((unsigned)((nblk + 255) / 256)), dim3(256), 0, c->stream, d_line_off, (long long)nlines,
                           (long long)n_text, nblk, d_nseg, d_k0);
        dev_scan(c, d_nseg, nblk, d_segbase, dc);
    }
    if (dc.ok()) {
        hipLaunchKernelGGL(tz_count_tokens, dim3((unsigned)counted), dim3(TZ_THREADS), lds_count, c->stream, d_text, (long long)n_text, d_line_off,
                           (long long)nlines, stride, d_nseg, d_k0, d_hist);
        dc.launched();
    }
    unsigned int hist[nd::NLL + nd::ND];
    dc.fetch(hist, d_hist, (size_t)nd::NLL + nd::ND);
    if ((rc = dc.sync())) return rc;
    nd::finish_hist(hist, hist + nd::NLL, counted, stride);      // one end-of-block per counted member; a code for every symbol when sampled
    nd::Codes codes;
    if (!nd::build_codes(hist, hist + nd::NLL, codes)) return fail(NATAC_E_ARG, "format_track: Huffman table description too long");
    nd::Codes *d_codes = dc.upload(&codes, 1);
    unsigned char *d_regions = dc.zeroed<unsigned char>((size_t)nblk * nd::REGION);
    unsigned int *d_sizes = dc.alloc<unsigned int>((size_t)nblk);
    unsigned long long *d_pos = dc.alloc<unsigned long long>((size_t)nblk + 1);
    const size_t lds_emit = 65536 + ((sizeof(nd::Codes) + 15) & ~(size_t)15);
    if (dc.ok()) {
        hipLaunchKernelGGL(tz_emit_members, dim3((unsigned)nblk), dim3(TZ_THREADS), lds_emit, c->stream, d_text, (long long)n_text, d_line_off,
                           (long long)nlines, d_nseg, d_k0, d_segbase, d_stage, d_segbits, d_codes, c->d_crc, d_regions, d_sizes);
        dc.launched();
    }
    if (dc.ok()) dev_scan(c, d_sizes, nblk, d_pos, dc);
    b->fmt_member_pos.resize((size_t)nblk + 1);
    dc.fetch(b->fmt_member_pos.data(), d_pos, (size_t)nblk + 1);
    {   // tabix records: runs of lines per leaf bin (tz_group_*)
        const unsigned lb = (unsigned)((nlines + 255) / 256);
        unsigned char *d_gf = dc.alloc<unsigned char>((size_t)nlines);
        unsigned long long *d_gidx = dc.alloc<unsigned long long>((size_t)nlines + 1);
        if (dc.ok()) {
            hipLaunchKernelGGL(tz_group_flags, dim3(lb), dim3(256), 0, c->stream, (long long)nlines, d_lcid, d_lbeg, d_lend, d_gf);
            dev_scan(c, d_gf, (long long)nlines, d_gidx, dc);
        }
        unsigned long long ngroups = 0;
        dc.fetch(&ngroups, d_gidx + nlines, 1);
        if ((rc = dc.sync())) return rc;
        long long *d_first = dc.alloc<long long>((size_t)ngroups);
        GroupRec *d_rec = dc.alloc<GroupRec>((size_t)ngroups);
        if (dc.ok()) {
            hipLaunchKernelGGL(tz_group_starts, dim3(lb), dim3(256), 0, c->stream, (long long)nlines, d_gf, d_gidx, d_first);
            hipLaunchKernelGGL(tz_group_records, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, c->stream, (long long)ngroups, d_first,
                               (long long)nlines, d_lcid, d_lbeg, d_lend, d_line_off, (long long)n_text, d_rec);
            dc.launched();
        }
        b->fmt_groups.resize((size_t)ngroups);
        dc.fetch(b->fmt_groups.data(), d_rec, (size_t)ngroups);
    }
    if ((rc = dc.sync())) return rc;
    const unsigned long long total = b->fmt_member_pos[(size_t)nblk];
    if ((rc = dev_alloc(b->d_fmt_out, (size_t)total + 64))) return rc;
    hipLaunchKernelGGL(tz_compact, dim3((unsigned)nblk), dim3(256), 0, c->stream, d_regions, d_sizes, d_pos, b->d_fmt_out);
    dc.launched();
    if ((rc = dc.finish())) return rc;
    b->fmt_bytes = (long long)total;
    if (n_bytes) *n_bytes = (int64_t)total;
    return NATAC_OK;
}

extern "C" {

/* ---------------- device-side track writer: entry points (helpers above extern "C") ---------------- */

int natac_batch_format_track(natac_batch *b, int track, const int32_t *chrom_id, const char *const *names, int32_t n_names,
                             const int64_t *chunk_start, int write_zero, int compress, int64_t *n_bytes, int64_t *n_text_bytes,
                             int64_t *n_lines, int32_t *n_hard) {
    if (!b || !chrom_id || !names || !chunk_start || n_names <= 0) return fail(NATAC_E_ARG, "null argument");
    int rc = need_track(b, track);
    if (rc) return rc;
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_all(c));
    if (track != NATAC_T_INS)
        return format_values(b, b->d_track[track], chrom_id, names, n_names, chunk_start, write_zero, compress, n_bytes, n_text_bytes, n_lines,
                             n_hard);
    DeviceCall dc(c, "format_track");
    double *d_tmp = dc.alloc<double>((size_t)b->total_bp);   // insertion counts are int32 on the device; the writer takes float64 like the reference's track
    if (!dc.ok()) return dc.finish();
    const int blocks = (int)std::min<long long>((b->total_bp + 255) / 256, 65536);
    hipLaunchKernelGGL(natac_i32_to_f64, dim3(blocks), dim3(256), 0, c->stream, (const int *)b->d_track[NATAC_T_INS].get(), d_tmp, b->total_bp);
    dc.launched();
    rc = format_values(b, d_tmp, chrom_id, names, n_names, chunk_start, write_zero, compress, n_bytes, n_text_bytes, n_lines, n_hard);
    const int rc_end = dc.finish();
    return rc ? rc : rc_end;
}

// results handed to natac_batch_format_fetch_begin: wait for their copies, give the device buffers back
static int fmt_pending_wait(natac_batch *b) {
    hipError_t first = hipSuccess;
    for (auto &p : b->fmt_pending) {
        hipError_t e = hipEventSynchronize(p.second);
        if (e != hipSuccess && first == hipSuccess) first = e;
        (void)hipEventDestroy(p.second);
        p.first.reset();
    }
    b->fmt_pending.clear();
    if (first != hipSuccess) return fail(NATAC_E_HIP, "format_fetch: %s", hipGetErrorString(first));
    return NATAC_OK;
}

int natac_batch_format_fetch_begin(natac_batch *b, void *dst, size_t dst_bytes) {
    if (!b || (!dst && dst_bytes)) return fail(NATAC_E_ARG, "null argument");
    if (b->fmt_bytes < 0) return fail(NATAC_E_STATE, "natac_batch_format_track has not run");
    if ((long long)dst_bytes < b->fmt_bytes) return fail(NATAC_E_ARG, "destination holds %zu bytes, result has %lld", dst_bytes, b->fmt_bytes);
    if (b->fmt_bytes == 0) return NATAC_OK;
    if (!b->d_fmt_out) return fail(NATAC_E_STATE, "the result has already been handed to natac_batch_format_fetch_begin");
    natac_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->device));
    if (!c->copy_stream) HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    // natac_batch_format_track returns with its stream drained: the result is complete, the copy needs no event from it
    hipEvent_t ev = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipMemcpyAsync(dst, b->d_fmt_out, (size_t)b->fmt_bytes, hipMemcpyDeviceToHost, c->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(ev, c->copy_stream);
    if (e != hipSuccess) { (void)hipEventDestroy(ev); return fail(NATAC_E_HIP, "format_fetch_begin: %s", hipGetErrorString(e)); }
    b->fmt_pending.emplace_back(std::move(b->d_fmt_out), ev);   // the buffer is the copy's until natac_batch_format_fetch_wait
    // fmt_bytes stays: the result's tabix records are still to be fetched; a second fetch of the bytes finds d_fmt_out empty
    return NATAC_OK;
}

int natac_batch_format_fetch_wait(natac_batch *b) {
    if (!b) return fail(NATAC_E_ARG, "batch is NULL");
    HIPCHK(hipSetDevice(b->ctx->device));
    return fmt_pending_wait(b);
}

int natac_batch_format_fetch(natac_batch *b, void *dst, size_t dst_bytes) {
    if (!b || (!dst && dst_bytes)) return fail(NATAC_E_ARG, "null argument");
    if (b->fmt_bytes < 0) return fail(NATAC_E_STATE, "natac_batch_format_track has not run");
    if ((long long)dst_bytes < b->fmt_bytes) return fail(NATAC_E_ARG, "destination holds %zu bytes, result has %lld", dst_bytes, b->fmt_bytes);
    if (b->fmt_bytes == 0) return NATAC_OK;
    if (!b->d_fmt_out) return fail(NATAC_E_STATE, "the result has already been handed to natac_batch_format_fetch_begin");
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipMemcpyAsync(dst, b->d_fmt_out, (size_t)b->fmt_bytes, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    return NATAC_OK;
}

struct natac_tbi { natac_tabix::Builder bld; };

int natac_tbi_create(natac_tbi **out) {
    if (!out) return fail(NATAC_E_ARG, "null argument");
    *out = new natac_tbi();
    return NATAC_OK;
}
void natac_tbi_free(natac_tbi *t) { delete t; }

static int tbi_push_groups(natac_tbi *t, int64_t n, const char *const *names, int32_t n_names, const int32_t *cid, const int64_t *beg,
                           const int64_t *end, const int64_t *count, const uint64_t *t0, const uint64_t *t1, const uint64_t *member_pos,
                           int64_t n_members, int64_t n_text, int64_t file_offset) {
    const size_t nblk = (size_t)n_members;
    // virtual offset of a text position: member start in the file << 16 | offset inside the member; a position at a member's end
    // belongs to the start of the next member (for the last one: whatever the caller writes next -- more members or the EOF block)
    auto voff = [&](uint64_t toff) -> uint64_t {
        if (toff >= (uint64_t)n_text) return ((uint64_t)file_offset + member_pos[nblk]) << 16;      // the end of the last (partial) member
        const size_t m = (size_t)(toff / natac_deflate::BLK);
        return (((uint64_t)file_offset + member_pos[m]) << 16) | (toff - (uint64_t)m * natac_deflate::BLK);
    };
    for (int64_t i = 0; i < n; ++i) {
        if (cid[i] < 0 || cid[i] >= n_names) return fail(NATAC_E_ARG, "record with chromosome id %d", cid[i]);
        const char *nm = names[cid[i]];
        if (!t->bld.push(nm, strlen(nm), beg[i], end[i], voff(t0[i]), voff(t1[i]), count[i])) return fail(NATAC_E_ARG, "tabix index: %s", t->bld.err.c_str());
    }
    return NATAC_OK;
}

int natac_batch_format_index_size(natac_batch *b, int64_t *n_groups, int64_t *n_members, int64_t *n_text) {
    if (!b || !n_groups || !n_members || !n_text) return fail(NATAC_E_ARG, "null argument");
    *n_text = b->fmt_text_bytes;
    if (b->fmt_bytes < 0) return fail(NATAC_E_STATE, "natac_batch_format_track has not run");
    *n_groups = (int64_t)b->fmt_groups.size();
    *n_members = b->fmt_member_pos.empty() ? 0 : (int64_t)b->fmt_member_pos.size() - 1;
    return NATAC_OK;
}

int natac_batch_format_index_fetch(natac_batch *b, int32_t *cid, int64_t *beg, int64_t *end, int64_t *count, uint64_t *t0, uint64_t *t1,
                                   uint64_t *member_pos) {
    if (!b) return fail(NATAC_E_ARG, "null argument");
    if (b->fmt_bytes < 0) return fail(NATAC_E_STATE, "natac_batch_format_track has not run");
    const size_t n = b->fmt_groups.size();
    if (n && (!cid || !beg || !end || !count || !t0 || !t1)) return fail(NATAC_E_ARG, "null argument");
    for (size_t i = 0; i < n; ++i) {
        const auto &g = b->fmt_groups[i];
        cid[i] = g.cid; beg[i] = g.beg; end[i] = g.end; count[i] = g.count; t0[i] = g.t0; t1[i] = g.t1;
    }
    if (!b->fmt_member_pos.empty()) {
        if (!member_pos) return fail(NATAC_E_ARG, "null argument");
        memcpy(member_pos, b->fmt_member_pos.data(), b->fmt_member_pos.size() * sizeof(uint64_t));
    }
    return NATAC_OK;
}

int natac_tbi_push(natac_tbi *t, int64_t n, const char *const *names, int32_t n_names, const int32_t *cid, const int64_t *beg,
                   const int64_t *end, const int64_t *count, const uint64_t *t0, const uint64_t *t1, const uint64_t *member_pos,
                   int64_t n_members, int64_t n_text, int64_t file_offset) {
    if (!t || n < 0 || n_members < 0 || file_offset < 0 || n_text < 0) return fail(NATAC_E_ARG, "bad argument");
    if (n == 0) return NATAC_OK;
    if (!names || !cid || !beg || !end || !count || !t0 || !t1 || !member_pos) return fail(NATAC_E_ARG, "null argument");
    return tbi_push_groups(t, n, names, n_names, cid, beg, end, count, t0, t1, member_pos, n_members, n_text, file_offset);
}

int natac_tbi_write(natac_tbi *t, const char *tbi_path, int64_t *n_records) {
    if (!t || !tbi_path) return fail(NATAC_E_ARG, "null argument");
    const int rc = t->bld.write(tbi_path);
    if (rc) return fail(NATAC_E_ARG, "cannot write %s (code %d)", tbi_path, rc);
    if (n_records) *n_records = t->bld.nrec;
    return NATAC_OK;
}

int natac_format_doubles(natac_ctx *c, const double *vals, int64_t n, char *out, size_t out_cap, int64_t *out_off, int32_t *n_hard) {
    if (!c || !vals || !out || !out_off || n <= 0) return fail(NATAC_E_ARG, "bad argument");
    if (out_cap < (size_t)n * natac_text::MAX_VALUE_CHARS) return fail(NATAC_E_ARG, "out must hold %d bytes per value", natac_text::MAX_VALUE_CHARS);
    DeviceCall dc(c, "format_doubles");
    if (!dc.ok()) return dc.finish();
    int rc = ensure_text_tables(c);
    if (rc) return rc;
    std::vector<int> len((size_t)n + 1);
    std::vector<char> raw((size_t)n * natac_text::MAX_VALUE_CHARS);
    const double *d_v = dc.upload(vals, (size_t)n);
    char *d_o = dc.alloc<char>(raw.size());
    int *d_len = dc.alloc<int>((size_t)n + 1), *d_hard = d_len + n;      // the lengths, then the count of undecidable values
    dc.zero(d_hard, 1);
    if (dc.ok()) {
        hipLaunchKernelGGL(natac_textz::tz_format_values, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d_v, (long long)n, c->d_p10, d_o,
                           d_len, d_hard);
        dc.launched();
    }
    dc.fetch(len.data(), d_len, (size_t)n + 1);
    dc.fetch(raw.data(), d_o, raw.size());
    if ((rc = dc.finish())) return rc;
    long long o = 0;
    for (int64_t i = 0; i < n; ++i) {
        out_off[i] = o;
        memcpy(out + o, raw.data() + (size_t)i * natac_text::MAX_VALUE_CHARS, (size_t)len[(size_t)i]);
        o += len[(size_t)i];
    }
    out_off[n] = o;
    if (n_hard) *n_hard = len[(size_t)n];
    return NATAC_OK;
}

int natac_bgzf_lines_host(const char *text, int64_t n, const int64_t *line_off, int64_t n_lines, void *out, size_t out_cap, int64_t *n_bytes) {
    if (!text || !line_off || !n_bytes || n < 0 || n_lines < 0) return fail(NATAC_E_ARG, "bad argument");
    std::string res;
    if (!natac_deflate::bgzf_lines_host((const unsigned char *)text, n, (const long long *)line_off, n_lines, res))
        return fail(NATAC_E_ARG, "Huffman table description too long");
    *n_bytes = (int64_t)res.size();
    if (res.size() > out_cap) return fail(NATAC_E_ARG, "destination holds %zu bytes, result has %zu", out_cap, res.size());
    if (out && !res.empty()) memcpy(out, res.data(), res.size());
    return NATAC_OK;
}

/* ---------------- native track writer + bgzip ---------------- */

int natac_write_bedgraph(const char *path, int append, int compress, int finish, int32_t n_chunks, const char *const *chroms,
                         const int64_t *chunk_start, const int64_t *out_off, const double *vals, int write_zero, int n_threads,
                         int64_t *bytes_written) {
    if (!path || n_chunks < 0 || (n_chunks > 0 && (!chroms || !chunk_start || !out_off || !vals)))
        return fail(NATAC_E_ARG, "null argument");
    if (compress < 0 || compress > 9) return fail(NATAC_E_ARG, "compress must be 0 (text) or a deflate level 1..9");
    for (int i = 0; i < n_chunks; ++i) {
        if (!chroms[i] || std::strlen(chroms[i]) > 100) return fail(NATAC_E_ARG, "bad chromosome name for chunk %d", i);
        if (out_off[i + 1] < out_off[i]) return fail(NATAC_E_ARG, "out_off must be non-decreasing");
    }
    const int rc = natac_writer::write_bedgraph(path, append != 0, compress, finish != 0, n_chunks, chroms, chunk_start, out_off, vals,
                                                (write_zero & 1) != 0, n_threads, bytes_written, (write_zero & 2) != 0);
    if (rc == 1) return fail(NATAC_E_ARG, "cannot open %s", path);
    if (rc == 2) return fail(NATAC_E_ARG, "write to %s failed", path);
    if (rc == 3) return fail(NATAC_E_NOMEM, "deflate failed");
    return NATAC_OK;
}

int natac_write_bed_rows(const char *path, int append, int64_t n_rows, const int32_t *chrom_id, const char *const *names, int32_t n_names,
                         const int64_t *start, const int64_t *end, const double *vals, int32_t n_cols) {
    if (!path || n_rows < 0 || n_cols < 0 || n_cols > 32) return fail(NATAC_E_ARG, "bad argument");
    if (n_rows > 0 && (!chrom_id || !names || !start || !end || (n_cols > 0 && !vals))) return fail(NATAC_E_ARG, "null argument");
    for (int64_t r = 0; r < n_rows; ++r)
        if (chrom_id[r] < 0 || chrom_id[r] >= n_names) return fail(NATAC_E_ARG, "row %lld: chromosome id %d out of range", (long long)r, chrom_id[r]);
    const int rc = natac_writer::write_bed_rows(path, append != 0, n_rows, chrom_id, names, start, end, vals, n_cols);
    if (rc == 1) return fail(NATAC_E_ARG, "cannot open %s", path);
    if (rc) return fail(NATAC_E_ARG, "write error on %s", path);
    return NATAC_OK;
}

int natac_write_bed_rows_labeled(const char *path, int append, int64_t n_rows, const int32_t *chrom_id, const char *const *names, int32_t n_names,
                                 const int64_t *start, const int64_t *end, const double *vals, int32_t n_cols, const int32_t *label_id,
                                 const char *const *labels, int32_t n_labels) {
    if (!path || n_rows < 0 || n_cols < 0 || n_cols > 32) return fail(NATAC_E_ARG, "bad argument");
    if (n_rows > 0 && (!chrom_id || !names || !start || !end || (n_cols > 0 && !vals) || !label_id || !labels)) return fail(NATAC_E_ARG, "null argument");
    for (int64_t r = 0; r < n_rows; ++r) {
        if (chrom_id[r] < 0 || chrom_id[r] >= n_names) return fail(NATAC_E_ARG, "row %lld: chromosome id %d out of range", (long long)r, chrom_id[r]);
        if (label_id[r] < 0 || label_id[r] >= n_labels) return fail(NATAC_E_ARG, "row %lld: label id %d out of range", (long long)r, label_id[r]);
    }
    const int rc = natac_writer::write_bed_rows(path, append != 0, n_rows, chrom_id, names, start, end, vals, n_cols, label_id, labels);
    if (rc == 1) return fail(NATAC_E_ARG, "cannot open %s", path);
    if (rc) return fail(NATAC_E_ARG, "write error on %s", path);
    return NATAC_OK;
}

int natac_bgzip_file(const char *src, const char *dst, int level, int n_threads) {
    if (!src || !dst) return fail(NATAC_E_ARG, "null argument");
    if (level < 1 || level > 9) return fail(NATAC_E_ARG, "level must be 1..9");
    std::string text;
    {
        FILE *f = std::fopen(src, "rb");
        if (!f) return fail(NATAC_E_ARG, "cannot open %s", src);
        std::fseek(f, 0, SEEK_END);
        const long sz = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        text.resize((size_t)sz);
        const bool ok = sz == 0 || std::fread(&text[0], 1, (size_t)sz, f) == (size_t)sz;
        std::fclose(f);
        if (!ok) return fail(NATAC_E_ARG, "cannot read %s", src);
    }
    const size_t BLK = 0xff00, nblk = (text.size() + BLK - 1) / BLK;
    if (n_threads <= 0) n_threads = natac_cores::default_threads(64);
    n_threads = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_threads, (nblk + 15) / 16));
    std::vector<std::string> parts(n_threads);
    std::vector<int> bad(n_threads, 0);
    auto work = [&](int t) {   // contiguous block ranges so that the parts concatenate in file order
        const size_t b0 = nblk * t / n_threads, b1 = nblk * (t + 1) / n_threads;
        natac_writer::Deflater df;                // one z_stream per thread, deflateReset per member
        parts[t].reserve((b1 - b0) * 24000);
        for (size_t b = b0; b < b1; ++b)
            if (!natac_writer::bgzf_block(parts[t], (const unsigned char *)text.data() + b * BLK, std::min(BLK, text.size() - b * BLK), level, &df)) {
                bad[t] = 1;
                return;
            }
    };
    {
        std::vector<std::thread> th;
        for (int t = 1; t < n_threads; ++t) th.emplace_back(work, t);
        work(0);
        for (auto &x : th) x.join();
    }
    for (int b : bad) if (b) return fail(NATAC_E_NOMEM, "deflate failed");
    FILE *f = std::fopen(dst, "wb");
    if (!f) return fail(NATAC_E_ARG, "cannot open %s", dst);
    bool ok = true;
    for (auto &p : parts) ok = ok && (p.empty() || std::fwrite(p.data(), 1, p.size(), f) == p.size());
    ok = ok && std::fwrite(natac_writer::BGZF_EOF, 1, 28, f) == 28;
    if (std::fclose(f) != 0 || !ok) return fail(NATAC_E_ARG, "write to %s failed", dst);
    return NATAC_OK;
}

int natac_tabix_index(const char *path, const char *tbi_path, int n_threads, int64_t *n_records) {
    if (!path) return fail(NATAC_E_ARG, "path is NULL");
    std::string msg;
    const int rc = natac_tabix::index_bed(path, tbi_path, n_threads, n_records, &msg);
    switch (rc) {
        case 0: return NATAC_OK;
        case 1: return fail(NATAC_E_ARG, "cannot read %s", path);
        case 2: return fail(NATAC_E_ARG, "%s is not a BGZF file", path);
        case 3: return fail(NATAC_E_NOMEM, "inflate / deflate failed on %s", path);
        case 4: return fail(NATAC_E_ARG, "%s: %s", path, msg.c_str());
        default: return fail(NATAC_E_ARG, "cannot write the index of %s", path);
    }
}

struct natac_tbx { natac_tabix::Reader *impl = nullptr; };

int natac_tbx_open(const char *path, natac_tbx **out) {
    if (!path || !out) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    natac_tabix::Reader *r = nullptr;
    const int rc = natac_tabix::open_reader(path, &r);
    if (rc == 1) return fail(NATAC_E_ARG, "cannot open %s (or its .tbi)", path);
    if (rc) return fail(NATAC_E_ARG, "%s.tbi is not a tabix index", path);
    natac_tbx *t = new natac_tbx();
    t->impl = r;
    *out = t;
    return NATAC_OK;
}

void natac_tbx_close(natac_tbx *t) {
    if (!t) return;
    natac_tabix::close_reader(t->impl);
    delete t;
}

int natac_tbx_read_values(natac_tbx *t, const char *chrom, int64_t start, int64_t end, int value_col, double empty, double *out,
                          int64_t *n_records) {
    if (!t || !chrom || (end > start && !out)) return fail(NATAC_E_ARG, "null argument");
    if (value_col < 1 || value_col > 8) return fail(NATAC_E_ARG, "value_col must be 1..8");
    const int64_t n = natac_tabix::read_values(t->impl, chrom, start, end, value_col, empty, out);
    if (n < 0) return fail(NATAC_E_ARG, "read error in the indexed file");
    if (n_records) *n_records = n;
    return NATAC_OK;
}

int natac_tbx_read_regions(natac_tbx *t, int64_t n, const int32_t *chrom_id, const char *const *names, int32_t n_names,
                           const int64_t *start, const int64_t *end, int value_col, double empty, double *out, const int64_t *out_off,
                           int n_threads, int64_t *n_records) {
    if (!t || n < 0 || (n > 0 && (!chrom_id || !names || !start || !end || !out_off))) return fail(NATAC_E_ARG, "null argument");
    if (value_col < 1 || value_col > 8) return fail(NATAC_E_ARG, "value_col must be 1..8");
    for (int64_t i = 0; i < n; ++i) {
        if (chrom_id[i] < 0 || chrom_id[i] >= n_names) return fail(NATAC_E_ARG, "region %lld: chromosome index out of range", (long long)i);
        if (end[i] > start[i] && !out) return fail(NATAC_E_ARG, "null output");
    }
    const int64_t u = natac_tabix::read_regions(t->impl, n, chrom_id, names, n_names, start, end, value_col, empty, out, out_off, n_threads);
    if (u < 0) return fail(NATAC_E_ARG, "read error in the indexed file");
    if (n_records) *n_records = u;
    return NATAC_OK;
}

}  // extern "C"
