// natac_files.hpp -- the handles over the library's input files: BED-like tables (natac_bedtab_*), FASTA (natac_fasta_*), BAM and
// fragment files into one fragment handle (natac_bam_*, natac_frag_open*, natac_frag_split*: the device decoders of natac_bam_dev.hpp
// and natac_fragfile_dev.hpp where the file is BGZF, the host decoders otherwise), the cells of a fragment file (natac_frag_cells*,
// natac_cells_*), and the host-only helpers next to them (natac_pack_chunks, natac_fuzz_evaluate, natac_inflate_raw_host).
#pragma once
#include "natac_runtime.hpp"
#include "natac_bam.hpp"
#include "natac_bam_dev.hpp"
#include "natac_bedtab.hpp"
#include "natac_fasta.hpp"
#include "natac_fragfile.hpp"
#include "natac_fragfile_dev.hpp"
#include "natac_fuzzfit.hpp"
#include "natac_pack.hpp"

#include <cstring>
#include <memory>

struct natac_bam {
    natac_bamio::Bam *impl = nullptr;
};

struct natac_cells {
    natac_fragio::Cells table;
};

extern "C" {

int natac_pack_chunks(int32_t n_chunks, const int64_t *chunk_start, const int64_t *chunk_end, const int32_t *chrom_id, int32_t n_chroms,
                      const int64_t *const *pos, const int64_t *const *tlen, const int64_t *n_per_chrom, int64_t margin, int atac,
                      int64_t *frag_off, int64_t *first, int32_t *lpos, int32_t *ilen, int n_threads) {
    if (n_chunks < 0 || n_chroms < 0 || margin < 0) return fail(NATAC_E_ARG, "bad sizes");
    if (n_chunks > 0 && (!chunk_start || !chunk_end || !chrom_id || !frag_off || !first)) return fail(NATAC_E_ARG, "null argument");
    if (n_chroms > 0 && (!pos || !tlen || !n_per_chrom)) return fail(NATAC_E_ARG, "null argument");
    for (int32_t i = 0; i < n_chunks; ++i) {
        if (chrom_id[i] >= n_chroms) return fail(NATAC_E_ARG, "chunk %d: chromosome id %d out of range", i, chrom_id[i]);
        if (chunk_end[i] < chunk_start[i]) return fail(NATAC_E_ARG, "chunk %d: end < start", i);
    }
    const int shift = atac ? 4 : 0, trim = atac ? 8 : 0;
    if (!lpos || !ilen) {
        if (!frag_off) return fail(NATAC_E_ARG, "null argument");
        if (n_chunks == 0) { if (frag_off) frag_off[0] = 0; return NATAC_OK; }
        natac_pack::count(n_chunks, chunk_start, chunk_end, chrom_id, pos, n_per_chrom, margin, shift, frag_off, first);
        return NATAC_OK;
    }
    if (n_chunks == 0) return NATAC_OK;
    natac_pack::fill(n_chunks, chunk_start, chrom_id, pos, tlen, frag_off, first, shift, trim, lpos, ilen, n_threads);
    return NATAC_OK;
}

int natac_fuzz_evaluate(int32_t K, int32_t n, int32_t M, const double *X0, const double *lb, const double *ub, const double *sig,
                        const double *xs, const int64_t *lens, void *exp_loop, void *exp_data, double *work, double *f, double *g) {
    if (K < 0 || M < 0 || (n != 3 && n != 6 && n != 9)) return fail(NATAC_E_ARG, "n must be 3, 6 or 9");
    if (K == 0) return NATAC_OK;
    if (!X0 || !lb || !ub || !sig || !xs || !lens || !exp_loop || !work || !f || !g) return fail(NATAC_E_ARG, "null argument");
    for (int k = 0; k < K; ++k)
        if (lens[k] < 0 || lens[k] > M) return fail(NATAC_E_ARG, "fit %d: window length out of range", k);
    natac_fuzzfit::evaluate(K, n, M, X0, lb, ub, sig, xs, lens, (natac_fuzzfit::ufunc_loop)exp_loop, exp_data, work, f, g);
    return NATAC_OK;
}

/* ---------------- BED-like table reader ---------------- */

struct natac_bedtab { natac_bedtabio::Table impl; };

int natac_bedtab_open(const char *path, const int32_t *cols, int32_t n_cols, natac_bedtab **out) {
    if (!path || !out || n_cols < 0 || n_cols > 32 || (n_cols > 0 && !cols)) return fail(NATAC_E_ARG, "bad argument");
    *out = nullptr;
    for (int c = 0; c < n_cols; ++c)
        if (cols[c] < 0 || cols[c] > 4095) return fail(NATAC_E_ARG, "column index out of range");
    natac_bedtab *t = new natac_bedtab();
    std::string err;
    const int rc = natac_bedtabio::load(path, cols, n_cols, &t->impl, err);
    if (rc) { delete t; return fail(NATAC_E_ARG, "%s: %s", path, err.c_str()); }
    *out = t;
    return NATAC_OK;
}

void natac_bedtab_close(natac_bedtab *t) { delete t; }

int natac_bedtab_dims(natac_bedtab *t, int64_t *n_rows, int32_t *n_names) {
    if (!t) return fail(NATAC_E_ARG, "table is NULL");
    if (n_rows) *n_rows = (int64_t)t->impl.chrom_id.size();
    if (n_names) *n_names = (int32_t)t->impl.names.size();
    return NATAC_OK;
}

int natac_bedtab_name(natac_bedtab *t, int32_t i, char *name, size_t name_len) {
    if (!t || !name) return fail(NATAC_E_ARG, "null argument");
    if (i < 0 || (size_t)i >= t->impl.names.size()) return fail(NATAC_E_ARG, "name index out of range");
    const std::string &s = t->impl.names[(size_t)i];
    if (s.size() + 1 > name_len) return fail(NATAC_E_ARG, "name longer than the buffer");
    std::memcpy(name, s.c_str(), s.size() + 1);
    return NATAC_OK;
}

int natac_bedtab_fetch(natac_bedtab *t, int32_t *chrom_id, int64_t *start, int64_t *end, double *vals) {
    if (!t) return fail(NATAC_E_ARG, "table is NULL");
    const size_t n = t->impl.chrom_id.size();
    if (n && (!chrom_id || !start || !end || (t->impl.n_cols && !vals))) return fail(NATAC_E_ARG, "null argument");
    if (n) {
        std::memcpy(chrom_id, t->impl.chrom_id.data(), n * sizeof(int32_t));
        std::memcpy(start, t->impl.start.data(), n * sizeof(int64_t));
        std::memcpy(end, t->impl.end.data(), n * sizeof(int64_t));
        if (t->impl.n_cols) std::memcpy(vals, t->impl.vals.data(), n * (size_t)t->impl.n_cols * sizeof(double));
    }
    return NATAC_OK;
}

/* ---------------- native FASTA loader ---------------- */

struct natac_fasta { natac_fastaio::Fasta *impl = nullptr; };

int natac_fasta_open(const char *path, int n_threads, natac_fasta **out) {
    if (!path || !out) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    std::string err;
    natac_fastaio::Fasta *impl = natac_fastaio::load(path, n_threads, err);
    if (!impl) return fail(NATAC_E_ARG, "%s: %s", path, err.c_str());
    natac_fasta *h = new natac_fasta();
    h->impl = impl;
    *out = h;
    return NATAC_OK;
}

void natac_fasta_close(natac_fasta *fa) {
    if (!fa) return;
    delete fa->impl;
    delete fa;
}

int natac_fasta_count(natac_fasta *fa, int32_t *n_records) {
    if (!fa || !n_records) return fail(NATAC_E_ARG, "null argument");
    *n_records = (int32_t)fa->impl->recs.size();
    return NATAC_OK;
}

int natac_fasta_info(natac_fasta *fa, int32_t record, char *name, size_t name_len, int64_t *length) {
    if (!fa) return fail(NATAC_E_ARG, "fasta is NULL");
    if (record < 0 || (size_t)record >= fa->impl->recs.size()) return fail(NATAC_E_ARG, "record out of range");
    const natac_fastaio::Record &r = fa->impl->recs[(size_t)record];
    if (name && name_len) {
        if (r.name.size() + 1 > name_len) return fail(NATAC_E_ARG, "record name longer than the buffer");
        std::memcpy(name, r.name.c_str(), r.name.size() + 1);
    }
    if (length) *length = r.length;
    return NATAC_OK;
}

int natac_fasta_read(natac_fasta *fa, int32_t record, void *out, int64_t n) {
    if (!fa) return fail(NATAC_E_ARG, "fasta is NULL");
    if (record < 0 || (size_t)record >= fa->impl->recs.size()) return fail(NATAC_E_ARG, "record out of range");
    if (n != fa->impl->recs[(size_t)record].length || (n > 0 && !out)) return fail(NATAC_E_ARG, "buffer does not match the record's length");
    natac_fastaio::read_record(fa->impl, (size_t)record, (unsigned char *)out);
    return NATAC_OK;
}

/* ---------------- native BAM extractor ---------------- */

// compressed bytes per window; the environment overrides (tests)
static size_t env_window(const char *name, size_t window) {
    if (const char *e = getenv(name)) { const long long v = atoll(e); if (v > 0) window = (size_t)v; }
    return window;
}
static size_t host_window() { return env_window("NATAC_BAM_WINDOW", (size_t)48 << 20); }              // the host decoders' streaming window
static size_t bam_dev_window() { return env_window("NATAC_BAM_DEV_WINDOW", (size_t)8 << 30); }        // a device window of a BAM
static size_t frag_dev_window() { return env_window("NATAC_FRAG_DEV_WINDOW", (size_t)1 << 30); }      // ... of a fragment file

// is the file a sequence of BGZF members (the device decoders' container; anything else is the host decoders')
static bool path_is_bgzf(const char *path) {
    bool bgzf = false;
    if (FILE *f = std::fopen(path, "rb")) {
        unsigned char magic[1040];
        bgzf = natac_fragio::is_bgzf(magic, std::fread(magic, 1, sizeof magic, f));
        std::fclose(f);
    }
    return bgzf;
}

// a decoder's end: the handle, or the decoder's message
static int bam_handle(natac_bamio::Bam *impl, const char *path, const std::string &err, natac_bam **out) {
    if (!impl) return fail(NATAC_E_ARG, "%s: %s", path, err.c_str());
    *out = new natac_bam();
    (*out)->impl = impl;
    return NATAC_OK;
}

int natac_bam_open(const char *path, int n_threads, natac_bam **out) {
    if (!path || !out) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    std::string err;
    natac_bamio::Bam *impl = natac_bamio::decode(path, n_threads, err, host_window());
    return bam_handle(impl, path, err, out);
}

int natac_bam_open_device(natac_ctx *c, const char *path, natac_bam **out, int *on_device) {
    if (!c || !path || !out) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    HIPCHK(hipSetDevice(c->device));
    std::string err;
    bool undecided = false;
    natac_bamio::Bam *impl = natac_bamdev::decode_device(path, c->stream, err, &undecided, bam_dev_window());
    if (on_device) *on_device = impl ? 1 : 0;
    if (!impl && undecided) impl = natac_bamio::decode(path, 0, err, host_window());      // the chain of record starts was not confirmed: the host decoder answers
    return bam_handle(impl, path, err, out);
}

/* ---------------- fragment files (fragments.tsv.gz) into the same handle ---------------- */

int natac_frag_open(const char *path, int n_threads, natac_bam **out) {
    if (!path || !out) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    std::string err;
    natac_bamio::Bam *impl = natac_fragio::decode(path, n_threads, err, host_window());
    return bam_handle(impl, path, err, out);
}

int natac_frag_open_device(natac_ctx *c, const char *path, natac_bam **out, int *on_device) {
    if (!c || !path || !out) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    if (on_device) *on_device = 0;
    HIPCHK(hipSetDevice(c->device));
    natac_bamio::Bam *impl = nullptr;
    std::string err;
    if (path_is_bgzf(path)) {                         // other containers are the host decoder's
        std::string why;
        impl = natac_fragdev::decode_plain(path, c->stream, why, frag_dev_window());
        if (impl && on_device) *on_device = 1;
    }
    // not BGZF, a malformed line, a damaged file, a line longer than a window, too many runs or a HIP failure: the host decoder answers
    if (!impl) impl = natac_fragio::decode(path, 0, err, host_window());
    return bam_handle(impl, path, err, out);
}

/* ---------------- a fragment file split by cell barcode into one handle per group ---------------- */

static int frag_split_table(int64_t n_barcodes, const void *bc_bytes, const int64_t *bc_off, const int32_t *bc_group, int32_t n_groups, natac_bam **out,
                            natac_fragio::SplitTableHost &table) {
    for (int32_t g = 0; g < n_groups && g < NATAC_SPLIT_MAX_GROUPS; ++g) out[g] = nullptr;
    std::string err;
    if (!table.build(n_barcodes, (const unsigned char *)bc_bytes, bc_off, bc_group, n_groups, NATAC_SPLIT_MAX_GROUPS, NATAC_SPLIT_MAX_BARCODES, err))
        return fail(NATAC_E_ARG, "%s", err.c_str());
    return NATAC_OK;
}

static int frag_split_host(const char *path, int n_threads, const natac_fragio::SplitTableHost &table, natac_bam **out, int64_t *bc_count,
                           int64_t *n_unassigned) {
    std::vector<natac_bamio::Bam *> impl((size_t)table.n_groups, nullptr);
    std::string err;
    if (!natac_fragio::decode_split(path, n_threads, table, impl.data(), bc_count, n_unassigned, err, host_window()))
        return fail(NATAC_E_ARG, "%s: %s", path, err.c_str());
    for (int g = 0; g < table.n_groups; ++g) {
        out[g] = new natac_bam();
        out[g]->impl = impl[(size_t)g];
    }
    return NATAC_OK;
}

int natac_frag_split(const char *path, int n_threads, int64_t n_barcodes, const void *bc_bytes, const int64_t *bc_off, const int32_t *bc_group,
                     int32_t n_groups, natac_bam **out, int64_t *bc_count, int64_t *n_unassigned) {
    if (!path || !out || !bc_bytes || !bc_off || !bc_group) return fail(NATAC_E_ARG, "null argument");
    natac_fragio::SplitTableHost table;
    if (const int rc = frag_split_table(n_barcodes, bc_bytes, bc_off, bc_group, n_groups, out, table)) return rc;
    return frag_split_host(path, n_threads, table, out, bc_count, n_unassigned);
}

int natac_frag_open_cells(const char *path, int n_threads, int64_t n_barcodes, const void *bc_bytes, const int64_t *bc_off, natac_bam **out,
                          int64_t *bc_count, int64_t *n_unassigned) {
    if (!path || !out || !bc_bytes || !bc_off) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    if (n_barcodes < 1 || n_barcodes > NATAC_SPLIT_MAX_BARCODES)       // (before the group array below is sized by it)
        return fail(NATAC_E_ARG, "n_barcodes must be in [1, %d]", NATAC_SPLIT_MAX_BARCODES);
    const std::vector<int32_t> one_group((size_t)n_barcodes, 0);
    natac_fragio::SplitTableHost table;
    if (const int rc = frag_split_table(n_barcodes, bc_bytes, bc_off, one_group.data(), 1, out, table)) return rc;
    natac_bamio::Bam *impl = nullptr;
    std::string err;
    if (!natac_fragio::decode_split(path, n_threads, table, &impl, bc_count, n_unassigned, err, host_window(), true))
        return fail(NATAC_E_ARG, "%s: %s", path, err.c_str());
    impl->tagged = true;
    *out = new natac_bam();
    (*out)->impl = impl;
    return NATAC_OK;
}

int natac_frag_split_device(natac_ctx *c, const char *path, int64_t n_barcodes, const void *bc_bytes, const int64_t *bc_off, const int32_t *bc_group,
                            int32_t n_groups, natac_bam **out, int64_t *bc_count, int64_t *n_unassigned, int *on_device) {
    if (!c || !path || !out || !bc_bytes || !bc_off || !bc_group) return fail(NATAC_E_ARG, "null argument");
    if (on_device) *on_device = 0;
    natac_fragio::SplitTableHost table;
    if (const int rc = frag_split_table(n_barcodes, bc_bytes, bc_off, bc_group, n_groups, out, table)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (path_is_bgzf(path) && n_barcodes <= natac_fragdev::SPLIT_DEV_MAX_BARCODES) {      // other containers and larger tables are the host path's
        natac_fragio::SplitBuilder sb(n_groups);
        natac_fragdev::SplitJob job;
        job.table = &table;
        job.sb = &sb;
        if (natac_fragdev::decode_device(path, c->stream, frag_dev_window(), job).empty()) {
            std::vector<natac_bamio::Bam *> impl((size_t)n_groups, nullptr);
            sb.finish(impl.data());
            for (int g = 0; g < n_groups; ++g) {
                out[g] = new natac_bam();
                out[g]->impl = impl[(size_t)g];
            }
            if (bc_count) std::copy(job.bc_count.begin(), job.bc_count.end(), bc_count);
            if (n_unassigned) *n_unassigned = sb.n_records - sb.n_assigned;
            if (on_device) *on_device = 1;
            return NATAC_OK;
        }
    }
    // everything natac_frag_open_device hands over, a line without a barcode field, too many groups x runs in a window: the host path answers
    return frag_split_host(path, 0, table, out, bc_count, n_unassigned);
}

/* ---------------- the cells of a fragment file ---------------- */

static int frag_cells_host(const char *path, int n_threads, int32_t nfr_upper, int32_t mono_upper, natac_cells **out) {
    std::unique_ptr<natac_cells> h(new natac_cells());
    std::string err;
    if (!natac_fragio::decode_cells(path, n_threads, nfr_upper, mono_upper, NATAC_SPLIT_MAX_BARCODES, &h->table, err, host_window()))
        return fail(NATAC_E_ARG, "%s: %s", path, err.c_str());
    *out = h.release();
    return NATAC_OK;
}

int natac_frag_cells(const char *path, int n_threads, int32_t nfr_upper, int32_t mono_upper, natac_cells **out) {
    if (!path || !out) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    if (!(0 < nfr_upper && nfr_upper < mono_upper)) return fail(NATAC_E_ARG, "0 < nfr_upper < mono_upper does not hold (got %d and %d)", nfr_upper, mono_upper);
    return frag_cells_host(path, n_threads, nfr_upper, mono_upper, out);
}

int natac_frag_cells_device(natac_ctx *c, const char *path, int32_t nfr_upper, int32_t mono_upper, natac_cells **out, int *on_device) {
    if (!c || !path || !out) return fail(NATAC_E_ARG, "null argument");
    *out = nullptr;
    if (on_device) *on_device = 0;
    if (!(0 < nfr_upper && nfr_upper < mono_upper)) return fail(NATAC_E_ARG, "0 < nfr_upper < mono_upper does not hold (got %d and %d)", nfr_upper, mono_upper);
    HIPCHK(hipSetDevice(c->device));
    if (path_is_bgzf(path)) {                         // other containers are the host path's
        std::unique_ptr<natac_cells> h(new natac_cells());
        natac_fragdev::CellsJob job;
        job.nfr_upper = nfr_upper;
        job.mono_upper = mono_upper;
        job.out = &h->table;
        if (natac_fragdev::decode_device(path, c->stream, frag_dev_window(), job).empty()) {
            *out = h.release();
            if (on_device) *on_device = 1;
            return NATAC_OK;
        }
    }
    // everything natac_frag_open_device hands over, a line without a barcode field, a full table, a HIP failure: the host path answers
    return frag_cells_host(path, 0, nfr_upper, mono_upper, out);
}

int natac_cells_counts(natac_cells *cells, int64_t *n_cells, int64_t *n_bytes, int64_t *n_data, int64_t *n_unassigned) {
    if (!cells) return fail(NATAC_E_ARG, "cells is NULL");
    if (n_cells) *n_cells = (int64_t)cells->table.n_frag.size();
    if (n_bytes) *n_bytes = (int64_t)cells->table.bytes.size();
    if (n_data) *n_data = cells->table.n_data;
    if (n_unassigned) *n_unassigned = cells->table.n_unassigned;
    return NATAC_OK;
}

int natac_cells_read(natac_cells *cells, int64_t n_cells, int64_t n_bytes, void *bc_bytes, int64_t *bc_off, int64_t *n_frag, int64_t *n_nfr,
                     int64_t *n_mono) {
    if (!cells) return fail(NATAC_E_ARG, "cells is NULL");
    const natac_fragio::Cells &t = cells->table;
    if (n_cells != (int64_t)t.n_frag.size() || n_bytes != (int64_t)t.bytes.size())
        return fail(NATAC_E_ARG, "the handle holds %zu cells of %zu bytes, buffers are for %lld of %lld", t.n_frag.size(), t.bytes.size(), (long long)n_cells,
                    (long long)n_bytes);
    if (bc_bytes && n_bytes) std::memcpy(bc_bytes, t.bytes.data(), (size_t)n_bytes);
    if (bc_off) std::memcpy(bc_off, t.off.data(), ((size_t)n_cells + 1) * sizeof(int64_t));
    if (n_frag && n_cells) std::memcpy(n_frag, t.n_frag.data(), (size_t)n_cells * sizeof(int64_t));
    if (n_nfr && n_cells) std::memcpy(n_nfr, t.n_nfr.data(), (size_t)n_cells * sizeof(int64_t));
    if (n_mono && n_cells) std::memcpy(n_mono, t.n_mono.data(), (size_t)n_cells * sizeof(int64_t));
    return NATAC_OK;
}

void natac_cells_close(natac_cells *cells) { delete cells; }

int natac_inflate_raw_host(const void *src, size_t csize, void *out, size_t isize) {
    if ((!src && csize) || (!out && isize) || csize > 0xffffffffull || isize > 0xffffffffull) return -1;
    std::vector<unsigned char> padded(csize + 32, 0);        // the bit reader takes whole words: 32 readable bytes behind the payload
    if (csize) std::memcpy(padded.data(), src, csize);
    return natac_bgzfdev::inflate_member_host(padded.data(), (unsigned int)csize, (unsigned char *)out, (unsigned int)isize);
}

void natac_bam_close(natac_bam *bam) {
    if (!bam) return;
    delete bam->impl;
    delete bam;
}

int natac_bam_counts(natac_bam *bam, int32_t *n_refs, int64_t *n_records, int64_t *n_kept) {
    if (!bam) return fail(NATAC_E_ARG, "bam is NULL");
    if (n_refs) *n_refs = (int32_t)bam->impl->refs.size();
    if (n_records) *n_records = bam->impl->n_records;
    if (n_kept) *n_kept = bam->impl->n_kept;
    return NATAC_OK;
}

int natac_bam_ref_info(natac_bam *bam, int32_t ref, char *name, size_t name_len, int64_t *length, int64_t *n_reads) {
    if (!bam || ref < 0 || ref >= (int32_t)bam->impl->refs.size()) return fail(NATAC_E_ARG, "bad reference index");
    const natac_bamio::Ref &r = bam->impl->refs[ref];
    if (name && name_len) snprintf(name, name_len, "%s", r.name.c_str());
    if (length) *length = r.length;
    if (n_reads) *n_reads = (int64_t)r.pos.size();
    return NATAC_OK;
}

int natac_bam_ref_reads(natac_bam *bam, int32_t ref, int64_t *pos, int64_t *tlen, int64_t n) {
    if (!bam || ref < 0 || ref >= (int32_t)bam->impl->refs.size()) return fail(NATAC_E_ARG, "bad reference index");
    const natac_bamio::Ref &r = bam->impl->refs[ref];
    if (n != (int64_t)r.pos.size()) return fail(NATAC_E_ARG, "reference holds %zu reads, buffers are for %lld", r.pos.size(), (long long)n);
    if (n && (!pos || !tlen)) return fail(NATAC_E_ARG, "null argument");
    if (n) {
        std::memcpy(pos, r.pos.data(), (size_t)n * sizeof(int64_t));
        std::memcpy(tlen, r.tlen.data(), (size_t)n * sizeof(int64_t));
    }
    return NATAC_OK;
}

int natac_bam_ref_cells(natac_bam *bam, int32_t ref, int32_t *cell) {
    if (!bam || ref < 0 || ref >= (int32_t)bam->impl->refs.size()) return fail(NATAC_E_ARG, "bad reference index");
    if (!bam->impl->tagged) return fail(NATAC_E_ARG, "the handle holds no cell indices (natac_frag_open_cells gives them)");
    const natac_bamio::Ref &r = bam->impl->refs[ref];
    if (!r.cell.empty() && !cell) return fail(NATAC_E_ARG, "null argument");
    if (!r.cell.empty()) std::memcpy(cell, r.cell.data(), r.cell.size() * sizeof(int32_t));
    return NATAC_OK;
}

}  // extern "C"
