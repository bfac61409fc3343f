// natac_fragfile.hpp -- fragment file (fragments.tsv.gz of Cell Ranger ATAC, ENCODE, chromap, sinto, ArchR ...) -> fragment arrays, host C++17.
//
// A fragment file is tab-separated text, one fragment per line (chrom start end [barcode [count]]), usually BGZF-compressed.  The
// store keeps (pos, |tlen|) of the forward proper-pair reads of a BAM (natac_bam.hpp), which is what such a line carries: the format
// rule of include/natac.h (natac_frag_open) maps [start, end) to pos = start - 4, tlen = end - start + 8, the inverse of the reference's
// ATAC offsets (pyatac/fragments.pyx:26-31).  parse_line below IS that rule; it is __host__ __device__ so that the device decoder
// (natac_fragfile_dev.hpp) classifies every line with the same code.
// Container by magic bytes: BGZF (the window reader of natac_bam.hpp), any other gzip (zlib, several members allowed), plain text.
// Splitting by cell barcode (natac_frag_split): split_line below IS the rule of include/natac.h -- parse_line, then the fourth field looked
// up in a SplitTable -- and is __host__ __device__ for the same reason.
// The cell-tagged read (natac_frag_open_cells) is the one-group split that keeps, per kept record, the index of its barcode in the table.
// Discovering the cells (natac_frag_cells): the cells rule of include/natac.h is barcode_line below, split_line's own line without a table: the
// barcodes are numbered as the file's data lines bring them up, each with its three fragment counters.
#pragma once
#include "natac_bam.hpp"

#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#ifdef __HIPCC__
#define NATAC_FRAG_HD __host__ __device__
#else
#define NATAC_FRAG_HD
#endif

namespace natac_fragio {

using natac_bamio::Bam;
using natac_bamio::Ref;

// what a line is: LINE_SKIP (empty or '#'), LINE_DATA, or a malformed data line (one value per fixed reason string)
enum { LINE_SKIP = 0, LINE_DATA = 1, BAD_FIELDS = 2, BAD_NAME_EMPTY = 3, BAD_NAME_LONG = 4, BAD_NUMBER = 5, BAD_RANGE = 6, BAD_ORDER = 7,
       BAD_NO_BARCODE = 8 };        // (only when splitting by barcode: split_line)

inline const char *reason_text(int kind) {
    switch (kind) {
        case BAD_FIELDS: return "fewer than three tab-separated fields";
        case BAD_NAME_EMPTY: return "empty chromosome name";
        case BAD_NAME_LONG: return "chromosome name longer than 255 bytes";
        case BAD_NUMBER: return "start / end is not a number";
        case BAD_RANGE: return "start / end out of range (more than 2147483647)";
        case BAD_ORDER: return "end before start";
        case BAD_NO_BARCODE: return "no barcode field";
    }
    return "";
}

// 1-10 ASCII digits, value <= 2^31 - 1.  LINE_DATA, BAD_NUMBER or BAD_RANGE.
NATAC_FRAG_HD inline int parse_coord(const unsigned char *p, size_t len, int32_t *out) {
    if (len == 0) return BAD_NUMBER;
    unsigned long long v = 0;
    for (size_t i = 0; i < len; ++i) {
        const unsigned d = (unsigned)p[i] - (unsigned)'0';
        if (d > 9u) return BAD_NUMBER;
        if (i < 11) v = v * 10ull + d;                  // (eleven digits of nines fit 64 bits; more digits are out of range anyway)
    }
    if (len > 10 || v > 2147483647ull) return BAD_RANGE;
    *out = (int32_t)v;
    return LINE_DATA;
}

// One line p[0, len) without its '\n' (and without the '\r' before it).  Checks in this order: fields, name, start, end, end >= start.
NATAC_FRAG_HD inline int parse_line(const unsigned char *p, size_t len, uint32_t *name_len, int32_t *start, int32_t *end) {
    if (len == 0 || p[0] == '#') return LINE_SKIP;
    size_t t1 = 0;
    while (t1 < len && p[t1] != '\t') ++t1;
    size_t t2 = t1 + 1;
    while (t2 < len && p[t2] != '\t') ++t2;
    if (t1 >= len || t2 >= len) return BAD_FIELDS;
    size_t t3 = t2 + 1;
    while (t3 < len && p[t3] != '\t') ++t3;
    if (t1 == 0) return BAD_NAME_EMPTY;
    if (t1 > 255) return BAD_NAME_LONG;
    int rc = parse_coord(p + t1 + 1, t2 - t1 - 1, start);
    if (rc != LINE_DATA) return rc;
    rc = parse_coord(p + t2 + 1, t3 - t2 - 1, end);
    if (rc != LINE_DATA) return rc;
    if (*end < *start) return BAD_ORDER;
    *name_len = (uint32_t)t1;
    return LINE_DATA;
}

// ---- splitting by cell barcode: the lookup table and the rule ----
// Open addressing, linear probing: slot[h & (n_slots - 1)] holds 1 + the index of a barcode, 0 = empty.  n_slots is a power of two of at
// least twice n_barcodes, so an empty slot always exists; the probe loop is bounded by n_slots all the same.  A slot only matches after
// its bytes compared equal.  hash_mask keeps the low bits of the hash (all of them unless NATAC_SPLIT_HASH_BITS says otherwise: tests).
struct SplitTable {
    const unsigned char *bytes;     // the barcodes, concatenated
    const uint32_t *off;            // [n_barcodes + 1] into bytes
    const int32_t *group;           // [n_barcodes]
    const uint32_t *slot;           // [n_slots]
    uint32_t n_barcodes, n_slots, hash_mask;
};

NATAC_FRAG_HD inline uint32_t barcode_hash(const unsigned char *p, size_t len) {      // FNV-1a and a final mix of the high bits into the low
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < len; ++i) h = (h ^ (uint32_t)p[i]) * 16777619u;
    h ^= h >> 15;
    h *= 0x2c1b3c6du;
    h ^= h >> 12;
    return h;
}

// index of the barcode p[0, len) in the table, or -1 (an empty barcode and one longer than 255 bytes are never listed)
NATAC_FRAG_HD inline int32_t barcode_lookup(const SplitTable &tb, const unsigned char *p, size_t len) {
    if (len == 0 || len > 255) return -1;
    uint32_t s = (barcode_hash(p, len) & tb.hash_mask) & (tb.n_slots - 1u);
    for (uint32_t probe = 0; probe < tb.n_slots; ++probe, s = (s + 1u) & (tb.n_slots - 1u)) {
        const uint32_t v = tb.slot[s];
        if (v == 0) return -1;
        const uint32_t k = v - 1u;
        if (k >= tb.n_barcodes) continue;
        const uint32_t a = tb.off[k], b = tb.off[k + 1];
        if ((size_t)(b - a) != len) continue;
        bool same = true;
        for (size_t i = 0; i < len && same; ++i) same = tb.bytes[a + i] == p[i];
        if (same) return (int32_t)k;
    }
    return -1;
}

// A data line and its barcode, for THE SPLIT RULE and THE CELLS RULE alike.  The line is classified by parse_line (same checks, same order); a
// data line without a fourth field is BAD_NO_BARCODE, checked last.  The barcode is p[*bc_at, *bc_at + *bc_len): the bytes between the
// third TAB and the fourth (or the line's end), whatever their number.
NATAC_FRAG_HD inline int barcode_line(const unsigned char *p, size_t len, uint32_t *name_len, int32_t *start, int32_t *end, size_t *bc_at, size_t *bc_len) {
    const int kind = parse_line(p, len, name_len, start, end);
    if (kind != LINE_DATA) return kind;
    size_t t = 0;
    for (int k = 0; k < 3; ++k, ++t) {                  // behind the third TAB
        while (t < len && p[t] != '\t') ++t;
        if (t >= len) return BAD_NO_BARCODE;
    }
    size_t e = t;
    while (e < len && p[e] != '\t') ++e;
    *bc_at = t;
    *bc_len = e - t;
    return LINE_DATA;
}

// THE SPLIT RULE.  barcode_line, and the barcode compared byte for byte: *bc = its index in the table, or -1: unassigned (empty, longer than
// 255 bytes or not listed), which is no error.
NATAC_FRAG_HD inline int split_line(const unsigned char *p, size_t len, const SplitTable &tb, uint32_t *name_len, int32_t *start, int32_t *end,
                                    int32_t *bc) {
    size_t at = 0, bc_len = 0;
    const int kind = barcode_line(p, len, name_len, start, end, &at, &bc_len);
    if (kind != LINE_DATA) return kind;
    *bc = barcode_lookup(tb, p + at, bc_len);
    return LINE_DATA;
}

// chromosomes in order of first appearance; a chromosome that comes back gets its old id and its records go behind the earlier ones
struct Builder {
    Bam *bam;
    std::unordered_map<std::string, int> ids;
    explicit Builder(Bam *b) : bam(b) {}
    Ref &ref_of(const std::string &name) {
        auto it = ids.find(name);
        if (it == ids.end()) {
            it = ids.emplace(name, (int)bam->refs.size()).first;
            bam->refs.emplace_back();
            bam->refs.back().name = name;
        }
        return bam->refs[(size_t)it->second];
    }
};

struct Run {                        // consecutive data lines of one chromosome
    std::string name;
    std::vector<int64_t> pos, tlen;
    int64_t max_end = 0;
};
struct SliceOut {
    std::vector<Run> runs;
    size_t n_lines = 0;             // lines seen (up to and including a malformed one)
    int bad = 0;                    // reason of the first malformed line (it is line n_lines of the slice)
};

// the complete lines of p[a, b) (b is behind a '\n', or `open_end`: the last line of the file has no '\n')
inline void parse_slice(const unsigned char *p, size_t a, size_t b, bool open_end, SliceOut *out) {
    Run *run = nullptr;
    while (a < b) {
        const unsigned char *nl = (const unsigned char *)std::memchr(p + a, '\n', b - a);
        size_t e = nl ? (size_t)(nl - p) : b;
        const size_t next = nl ? e + 1 : b;
        if (!nl && !open_end) break;
        if (nl && e > a && p[e - 1] == '\r') --e;
        ++out->n_lines;
        uint32_t nlen = 0;
        int32_t s = 0, t = 0;
        const int kind = parse_line(p + a, e - a, &nlen, &s, &t);
        if (kind > LINE_DATA) { out->bad = kind; return; }
        if (kind == LINE_DATA) {
            if (!run || run->name.size() != nlen || std::memcmp(run->name.data(), p + a, nlen) != 0) {
                out->runs.emplace_back();
                run = &out->runs.back();
                run->name.assign((const char *)p + a, nlen);
            }
            run->pos.push_back((int64_t)s - 4);
            run->tlen.push_back((int64_t)t - (int64_t)s + 8);
            if (t > run->max_end) run->max_end = t;
        }
        a = next;
    }
}

inline void append_run(Builder &bd, const std::string &name, const int64_t *pos, const int64_t *tlen, size_t n, int64_t max_end) {
    Ref &r = bd.ref_of(name);
    r.pos.insert(r.pos.end(), pos, pos + n);
    r.tlen.insert(r.tlen.end(), tlen, tlen + n);
    if (max_end > r.length) r.length = max_end;
    bd.bam->n_records += (int64_t)n;
    bd.bam->n_kept += (int64_t)n;
}

// Lines of p[0, n) in line-aligned slices, one per thread; the slices are merged in file order, so the result (and the first error) does
// not depend on n_threads.  *lines counts every line of the file so far.  false + err on a malformed line.
inline bool parse_text(const unsigned char *p, size_t n, bool open_end, int n_threads, Builder &bd, unsigned long long *lines, std::string &err) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_threads), n / 256));
    std::vector<size_t> cut((size_t)T + 1, n);
    cut[0] = 0;
    for (int t = 1; t < T; ++t) {
        const size_t at = std::max(cut[(size_t)t - 1], n * (size_t)t / (size_t)T);
        const unsigned char *nl = at < n ? (const unsigned char *)std::memchr(p + at, '\n', n - at) : nullptr;
        cut[(size_t)t] = nl ? (size_t)(nl - p) + 1 : n;
    }
    std::vector<SliceOut> out((size_t)T);
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(parse_slice, p, cut[(size_t)t], cut[(size_t)t + 1], open_end, &out[(size_t)t]);
    parse_slice(p, cut[0], cut[1], open_end, &out[0]);
    for (auto &x : th) x.join();
    for (auto &so : out) {
        *lines += so.n_lines;
        if (so.bad) { err = "line " + std::to_string(*lines) + ": " + reason_text(so.bad); return false; }
        for (auto &r : so.runs) append_run(bd, r.name, r.pos.data(), r.tlen.data(), r.pos.size(), r.max_end);
    }
    return true;
}

// BGZF: a gzip member whose extra field holds the BC subfield (SAM spec 4.1)
inline bool is_bgzf(const unsigned char *h, size_t have) {
    if (have < 18 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return false;
    const size_t xlen = natac_bamio::rd16(h + 10);
    for (size_t x = 12; x + 4 <= 12 + xlen && x + 4 <= have;) {
        const unsigned slen = natac_bamio::rd16(h + x + 2);
        if (h[x] == 'B' && h[x + 1] == 'C' && slen == 2) return true;
        x += 4 + slen;
    }
    return false;
}

// Streaming decode, bounded memory like natac_bamio::decode: ~window bytes of (compressed) input at a time, the bytes behind a window's
// last '\n' carried to the front of the next.  returns false + error text ("line N: reason" for a malformed line).
// parse(p, n, open_end, n_threads, &lines, err) takes every window's complete lines (parse_text, or parse_text_split below).
template <class Parse>
inline bool stream_text(const char *path, int n_threads, std::string &err, size_t window, Parse &&parse) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { err = std::string("cannot open ") + path; return false; }
    if (n_threads <= 0) n_threads = natac_cores::default_threads(64);
    window = std::max<size_t>(window, (size_t)4096);
    unsigned char magic[1040];
    const size_t have = std::fread(magic, 1, sizeof magic, f);
    std::rewind(f);
    const bool gz = have >= 2 && magic[0] == 0x1f && magic[1] == 0x8b, bgzf = is_bgzf(magic, have);
    std::vector<unsigned char> data, in;
    std::unique_ptr<natac_bamio::BgzfWindows> z(bgzf ? new natac_bamio::BgzfWindows(f, n_threads, window) : nullptr);
    z_stream zs;
    std::memset(&zs, 0, sizeof zs);
    bool zs_open = false, in_member = false, file_end = false;
    auto fail = [&](const std::string &msg) -> bool {
        err = msg;
        if (zs_open) inflateEnd(&zs);
        std::fclose(f);
        return false;
    };
    if (gz && !bgzf) {
        if (inflateInit2(&zs, 15 + 16) != Z_OK) return fail("zlib: inflateInit2 failed");
        zs_open = true;
        in.resize(std::min<size_t>(window, (size_t)4 << 20));
    }
    // the next window of text behind data[0, pend): 1 a window, 0 the file is done, -1 error (in msg)
    std::string msg;
    auto next = [&](size_t pend, size_t *n) -> int {
        if (bgzf) { const int rc = z->next(data, pend, n); if (rc < 0) msg = z->error; return rc; }
        if (data.size() < pend + window) data.resize(pend + window);
        if (!gz) {
            const size_t got = std::fread(data.data() + pend, 1, window, f);
            *n = pend + got;
            return got ? 1 : 0;
        }
        size_t o = pend;
        while (o < pend + window) {
            if (zs.avail_in == 0) {
                if (file_end) break;
                zs.avail_in = (uInt)std::fread(in.data(), 1, in.size(), f);
                zs.next_in = in.data();
                if (zs.avail_in == 0) { file_end = true; break; }
            }
            if (!in_member) {            // between members: zero padding is skipped (as gzip does), anything else must be a member
                while (zs.avail_in && *zs.next_in == 0) { ++zs.next_in; --zs.avail_in; }
                if (!zs.avail_in) continue;
                in_member = true;
            }
            zs.next_out = data.data() + o;
            zs.avail_out = (uInt)std::min<size_t>(pend + window - o, (size_t)1 << 30);
            const size_t before = zs.avail_out;
            const int rc = inflate(&zs, Z_NO_FLUSH);
            o += before - zs.avail_out;
            if (rc == Z_STREAM_END) { in_member = false; inflateReset(&zs); }
            else if (rc != Z_OK && rc != Z_BUF_ERROR) { msg = "inflate failed (corrupt gzip stream)"; return -1; }
        }
        if (file_end && zs.avail_in == 0 && in_member && o < pend + window) { msg = "truncated gzip stream"; return -1; }
        *n = o;
        return o > pend || !file_end ? 1 : 0;
    };
    size_t pend = 0;
    unsigned long long lines = 0;
    for (;;) {
        size_t n = 0;
        const int got = next(pend, &n);
        if (got < 0) return fail(msg);
        if (got == 0) break;
        size_t last = n;                                   // behind the last '\n' of the window
        while (last > pend && data[last - 1] != '\n') --last;
        if (last == pend) { pend = n; continue; }           // no line ends in this window: a line longer than it
        if (!parse(data.data(), last, false, n_threads, &lines, err)) return fail(err);
        pend = n - last;
        std::memmove(data.data(), data.data() + last, pend);
    }
    if (pend && !parse(data.data(), pend, true, 1, &lines, err)) return fail(err);                // a last line without '\n' is a line
    if (zs_open) inflateEnd(&zs);
    std::fclose(f);
    return true;
}

inline Bam *decode(const char *path, int n_threads, std::string &err, size_t window = (size_t)48 << 20) {
    Bam *bam = new Bam();
    Builder bd(bam);
    const bool ok = stream_text(path, n_threads, err, window, [&](const unsigned char *p, size_t n, bool open_end, int threads, unsigned long long *lines,
                                                                  std::string &e) { return parse_text(p, n, open_end, threads, bd, lines, e); });
    if (!ok) { delete bam; return nullptr; }
    return bam;
}

// ---- the split by barcode on the host ----
// The table as the host owns it.  build() checks the caller's arrays and that the barcodes are distinct (false + err names both entries).
struct SplitTableHost {
    std::vector<unsigned char> bytes;
    std::vector<uint32_t> off, slot;
    std::vector<int32_t> group;
    uint32_t hash_mask = 0xffffffffu;
    int n_groups = 0;
    SplitTable view() const { return SplitTable{bytes.data(), off.data(), group.data(), slot.data(), (uint32_t)group.size(), (uint32_t)slot.size(), hash_mask}; }
    bool build(int64_t n_barcodes, const unsigned char *bc_bytes, const int64_t *bc_off, const int32_t *bc_group, int groups, int max_groups,
               int64_t max_barcodes, std::string &err) {
        if (n_barcodes < 1 || n_barcodes > max_barcodes) { err = "n_barcodes must be in [1, " + std::to_string(max_barcodes) + "]"; return false; }
        if (groups < 1 || groups > max_groups) { err = "n_groups must be in [1, " + std::to_string(max_groups) + "]"; return false; }
        if (bc_off[0] != 0) { err = "bc_off[0] must be 0"; return false; }
        for (int64_t k = 0; k < n_barcodes; ++k) {
            const int64_t len = bc_off[k + 1] - bc_off[k];
            if (len < 1 || len > 255) { err = "barcode " + std::to_string(k) + " is not 1-255 bytes long"; return false; }
            if (bc_group[k] < 0 || bc_group[k] >= groups) { err = "barcode " + std::to_string(k) + ": group out of range"; return false; }
        }
        n_groups = groups;
        bytes.assign(bc_bytes, bc_bytes + bc_off[n_barcodes]);
        off.resize((size_t)n_barcodes + 1);
        for (int64_t k = 0; k <= n_barcodes; ++k) off[(size_t)k] = (uint32_t)bc_off[k];
        group.assign(bc_group, bc_group + n_barcodes);
        if (const char *e = getenv("NATAC_SPLIT_HASH_BITS")) { const int b = atoi(e); if (b >= 0 && b < 32) hash_mask = (1u << b) - 1u; }
        uint32_t ns = 16;
        while ((uint64_t)ns < 2ull * (uint64_t)n_barcodes) ns <<= 1;
        slot.assign(ns, 0u);
        for (int64_t k = 0; k < n_barcodes; ++k) {
            const unsigned char *p = bytes.data() + off[(size_t)k];
            const size_t len = off[(size_t)k + 1] - off[(size_t)k];
            const int32_t seen = barcode_lookup(view(), p, len);
            if (seen >= 0) { err = "barcodes " + std::to_string(seen) + " and " + std::to_string(k) + " are the same"; return false; }
            uint32_t s = (barcode_hash(p, len) & hash_mask) & (ns - 1u);
            while (slot[s] != 0) s = (s + 1u) & (ns - 1u);
            slot[s] = (uint32_t)k + 1u;
        }
        return true;
    }
};

// What both paths append to: ONE chromosome list (first appearance over all data lines, assigned or not) and one length per chromosome
// (the largest end over all of its data lines) for every group; per group and chromosome the group's records in file order.
// With `cells` (one group only) a third array per chromosome holds the table index of every kept record's barcode.
struct SplitBuilder {
    int G;
    bool cells;
    std::vector<std::vector<int32_t>> cell;                          // [chromosome]
    std::unordered_map<std::string, int> ids;
    std::vector<std::string> names;
    std::vector<int64_t> length, kept;
    std::vector<std::vector<std::vector<int64_t>>> pos, tlen;        // [group][chromosome]
    int64_t n_records = 0, n_assigned = 0;
    explicit SplitBuilder(int groups, bool keep_cells = false)
        : G(groups), cells(keep_cells), kept((size_t)groups, 0), pos((size_t)groups), tlen((size_t)groups) {}
    int chrom(const std::string &name, int64_t max_end, int64_t n_lines) {      // a run of n_lines data lines on `name`
        auto it = ids.find(name);
        if (it == ids.end()) {
            it = ids.emplace(name, (int)names.size()).first;
            names.push_back(name);
            length.push_back(0);
        }
        if (max_end > length[(size_t)it->second]) length[(size_t)it->second] = max_end;
        n_records += n_lines;
        return it->second;
    }
    void append(int g, int c, int64_t start, int64_t end, int32_t bc = 0) {
        auto &p = pos[(size_t)g], &t = tlen[(size_t)g];
        if (p.size() <= (size_t)c) { p.resize((size_t)c + 1); t.resize((size_t)c + 1); }
        p[(size_t)c].push_back(start - 4);
        t[(size_t)c].push_back(end - start + 8);
        if (cells) {
            if (cell.size() <= (size_t)c) cell.resize((size_t)c + 1);
            cell[(size_t)c].push_back(bc);
        }
        ++kept[(size_t)g];
        ++n_assigned;
    }
    void finish(Bam **out) {                             // out[G]; the arrays move
        for (int g = 0; g < G; ++g) {
            Bam *b = new Bam();
            b->refs.resize(names.size());
            for (size_t c = 0; c < names.size(); ++c) {
                b->refs[c].name = names[c];
                b->refs[c].length = length[c];
                if (c < pos[(size_t)g].size()) { b->refs[c].pos = std::move(pos[(size_t)g][c]); b->refs[c].tlen = std::move(tlen[(size_t)g][c]); }
                if (cells && c < cell.size()) b->refs[c].cell = std::move(cell[c]);
            }
            b->n_records = n_records;
            b->n_kept = kept[(size_t)g];
            out[g] = b;
        }
    }
};

struct SplitRun {                   // consecutive data lines of one chromosome: all of them counted, the assigned ones kept
    std::string name;
    std::vector<int32_t> start, end, group;      // group: the record's group, or (a cell-tagged read) the index of its barcode
    int64_t max_end = 0, n_data = 0;
};
struct SplitSliceOut {
    std::vector<SplitRun> runs;
    size_t n_lines = 0;
    int bad = 0;
};

// parse_slice with split_line.  bc_count (may be null) is shared by the slices: relaxed atomic adds, the sum does not depend on the order.
// keep_bc: a run keeps the barcode's index where it keeps the barcode's group otherwise.
inline void parse_slice_split(const unsigned char *p, size_t a, size_t b, bool open_end, const SplitTable *tb, int64_t *bc_count, bool keep_bc,
                              SplitSliceOut *out) {
    SplitRun *run = nullptr;
    while (a < b) {
        const unsigned char *nl = (const unsigned char *)std::memchr(p + a, '\n', b - a);
        size_t e = nl ? (size_t)(nl - p) : b;
        const size_t next = nl ? e + 1 : b;
        if (!nl && !open_end) break;
        if (nl && e > a && p[e - 1] == '\r') --e;
        ++out->n_lines;
        uint32_t nlen = 0;
        int32_t s = 0, t = 0, bc = -1;
        const int kind = split_line(p + a, e - a, *tb, &nlen, &s, &t, &bc);
        if (kind > LINE_DATA) { out->bad = kind; return; }
        if (kind == LINE_DATA) {
            if (!run || run->name.size() != nlen || std::memcmp(run->name.data(), p + a, nlen) != 0) {
                out->runs.emplace_back();
                run = &out->runs.back();
                run->name.assign((const char *)p + a, nlen);
            }
            ++run->n_data;
            if (t > run->max_end) run->max_end = t;
            if (bc >= 0) {
                run->start.push_back(s);
                run->end.push_back(t);
                run->group.push_back(keep_bc ? bc : tb->group[bc]);
                if (bc_count) __atomic_fetch_add(&bc_count[bc], (int64_t)1, __ATOMIC_RELAXED);
            }
        }
        a = next;
    }
}

// parse_text with split_line: the same slices, merged in file order
inline bool parse_text_split(const unsigned char *p, size_t n, bool open_end, int n_threads, const SplitTable &tb, int64_t *bc_count, SplitBuilder &sb,
                             unsigned long long *lines, std::string &err) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_threads), n / 256));
    std::vector<size_t> cut((size_t)T + 1, n);
    cut[0] = 0;
    for (int t = 1; t < T; ++t) {
        const size_t at = std::max(cut[(size_t)t - 1], n * (size_t)t / (size_t)T);
        const unsigned char *nl = at < n ? (const unsigned char *)std::memchr(p + at, '\n', n - at) : nullptr;
        cut[(size_t)t] = nl ? (size_t)(nl - p) + 1 : n;
    }
    std::vector<SplitSliceOut> out((size_t)T);
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t)
        th.emplace_back(parse_slice_split, p, cut[(size_t)t], cut[(size_t)t + 1], open_end, &tb, bc_count, sb.cells, &out[(size_t)t]);
    parse_slice_split(p, cut[0], cut[1], open_end, &tb, bc_count, sb.cells, &out[0]);
    for (auto &x : th) x.join();
    for (auto &so : out) {
        *lines += so.n_lines;
        if (so.bad) { err = "line " + std::to_string(*lines) + ": " + reason_text(so.bad); return false; }
        for (auto &r : so.runs) {
            const int c = sb.chrom(r.name, r.max_end, r.n_data);
            if (sb.cells) for (size_t k = 0; k < r.start.size(); ++k) sb.append(0, c, r.start[k], r.end[k], r.group[k]);
            else for (size_t k = 0; k < r.start.size(); ++k) sb.append(r.group[k], c, r.start[k], r.end[k]);
        }
    }
    return true;
}

// natac_frag_split's host path: out[n_groups] handles, or false + err and nothing.  cells: natac_frag_open_cells (a table of one group)
inline bool decode_split(const char *path, int n_threads, const SplitTableHost &th, Bam **out, int64_t *bc_count, int64_t *n_unassigned, std::string &err,
                         size_t window = (size_t)48 << 20, bool cells = false) {
    SplitBuilder sb(th.n_groups, cells);
    const SplitTable tb = th.view();
    if (bc_count) std::fill(bc_count, bc_count + tb.n_barcodes, (int64_t)0);
    const bool ok = stream_text(path, n_threads, err, window, [&](const unsigned char *p, size_t n, bool open_end, int threads, unsigned long long *lines,
                                                                  std::string &e) { return parse_text_split(p, n, open_end, threads, tb, bc_count, sb, lines, e); });
    if (!ok) return false;
    sb.finish(out);
    if (n_unassigned) *n_unassigned = sb.n_records - sb.n_assigned;
    return true;
}

// ---- discovering the cells of a fragment file (natac_frag_cells) ----
// THE CELLS RULE's line is barcode_line: a data line whose barcode is 1-255 bytes long belongs to the cell of that barcode, any other data
// line is unassigned (the callers' business: parse_slice_cells here, cells_parse on the device).
// the size class of a data line: 0 ilen < nfr_upper, 1 nfr_upper <= ilen < mono_upper, 2 neither
NATAC_FRAG_HD inline int cells_size_class(int32_t start, int32_t end, int32_t nfr_upper, int32_t mono_upper) {
    const int32_t ilen = end - start;                   // (0 <= start <= end <= 2^31 - 1: no overflow)
    return ilen < nfr_upper ? 0 : ilen < mono_upper ? 1 : 2;
}

// the result of both paths: the cells in order of first appearance over the file's data lines
struct Cells {
    std::vector<unsigned char> bytes;                   // the barcodes, concatenated
    std::vector<int64_t> off{0};                        // [n_cells + 1] into bytes
    std::vector<int64_t> n_frag, n_nfr, n_mono;         // [n_cells]
    int64_t n_data = 0, n_unassigned = 0;
};

struct CellsSliceOut {                                  // the cells of one slice in order of first appearance IN THE SLICE
    std::unordered_map<std::string_view, uint32_t> ids; // (views into the window's text: the slice outputs do not outlive parse_text_cells)
    std::vector<std::string_view> bc;
    std::vector<size_t> first_line;                     // the slice's line (1-based) on which the cell first appears
    std::vector<int64_t> cnt;                           // [3 * cells]: n_frag, n_nfr, n_mono
    int64_t n_data = 0, n_unassigned = 0;
    size_t n_lines = 0;
    int bad = 0;
};

inline void parse_slice_cells(const unsigned char *p, size_t a, size_t b, bool open_end, int32_t nfr_upper, int32_t mono_upper, CellsSliceOut *out) {
    while (a < b) {
        const unsigned char *nl = (const unsigned char *)std::memchr(p + a, '\n', b - a);
        size_t e = nl ? (size_t)(nl - p) : b;
        const size_t next = nl ? e + 1 : b;
        if (!nl && !open_end) break;
        if (nl && e > a && p[e - 1] == '\r') --e;
        ++out->n_lines;
        int32_t s = 0, t = 0;
        size_t at = 0, len = 0;
        uint32_t nlen = 0;
        const int kind = barcode_line(p + a, e - a, &nlen, &s, &t, &at, &len);
        if (kind > LINE_DATA) { out->bad = kind; return; }
        if (kind == LINE_DATA) {
            ++out->n_data;
            if (len < 1 || len > 255) ++out->n_unassigned;
            else {
                const std::string_view key((const char *)p + a + at, len);
                auto it = out->ids.find(key);
                if (it == out->ids.end()) {
                    it = out->ids.emplace(key, (uint32_t)out->bc.size()).first;
                    out->bc.push_back(key);
                    out->first_line.push_back(out->n_lines);
                    out->cnt.insert(out->cnt.end(), 3, (int64_t)0);
                }
                int64_t *c = out->cnt.data() + 3 * (size_t)it->second;
                ++c[0];
                const int cls = cells_size_class(s, t, nfr_upper, mono_upper);
                if (cls < 2) ++c[1 + cls];
            }
        }
        a = next;
    }
}

// What the slices merge into.  The slices discover in parallel; merged in file order, a cell new to the file is first met in the earliest slice
// that holds it, and within that slice in the slice's own order of first appearance: the file's order of first appearance.
struct CellsBuilder {
    Cells *out;
    int64_t max_cells;
    std::unordered_map<std::string, int64_t> ids;
    CellsBuilder(Cells *o, int64_t limit) : out(o), max_cells(limit) {}
};

// parse_text with barcode_line: the same slices.  An error is the first in file order: the line that passes the limit of distinct barcodes, or
// a malformed line.
inline bool parse_text_cells(const unsigned char *p, size_t n, bool open_end, int n_threads, int32_t nfr_upper, int32_t mono_upper, CellsBuilder &cb,
                             unsigned long long *lines, std::string &err) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_threads), n / 256));
    std::vector<size_t> cut((size_t)T + 1, n);
    cut[0] = 0;
    for (int t = 1; t < T; ++t) {
        const size_t at = std::max(cut[(size_t)t - 1], n * (size_t)t / (size_t)T);
        const unsigned char *nl = at < n ? (const unsigned char *)std::memchr(p + at, '\n', n - at) : nullptr;
        cut[(size_t)t] = nl ? (size_t)(nl - p) + 1 : n;
    }
    std::vector<CellsSliceOut> out((size_t)T);
    std::vector<std::thread> th;
    for (int t = 1; t < T; ++t) th.emplace_back(parse_slice_cells, p, cut[(size_t)t], cut[(size_t)t + 1], open_end, nfr_upper, mono_upper, &out[(size_t)t]);
    parse_slice_cells(p, cut[0], cut[1], open_end, nfr_upper, mono_upper, &out[0]);
    for (auto &x : th) x.join();
    Cells &res = *cb.out;
    for (auto &so : out) {
        const unsigned long long before = *lines;
        *lines += so.n_lines;
        for (size_t k = 0; k < so.bc.size(); ++k) {
            auto it = cb.ids.find(std::string(so.bc[k]));
            if (it == cb.ids.end()) {
                if ((int64_t)res.n_frag.size() >= cb.max_cells) {
                    err = "line " + std::to_string(before + so.first_line[k]) + ": more than " + std::to_string(cb.max_cells) + " distinct barcodes";
                    return false;
                }
                it = cb.ids.emplace(std::string(so.bc[k]), (int64_t)res.n_frag.size()).first;
                res.bytes.insert(res.bytes.end(), so.bc[k].begin(), so.bc[k].end());
                res.off.push_back((int64_t)res.bytes.size());
                res.n_frag.push_back(0);
                res.n_nfr.push_back(0);
                res.n_mono.push_back(0);
            }
            const size_t c = (size_t)it->second;
            res.n_frag[c] += so.cnt[3 * k];
            res.n_nfr[c] += so.cnt[3 * k + 1];
            res.n_mono[c] += so.cnt[3 * k + 2];
        }
        if (so.bad) { err = "line " + std::to_string(*lines) + ": " + reason_text(so.bad); return false; }
        res.n_data += so.n_data;
        res.n_unassigned += so.n_unassigned;
    }
    return true;
}

// natac_frag_cells' host path: containers, windows, slices and the first error as decode_split
inline bool decode_cells(const char *path, int n_threads, int32_t nfr_upper, int32_t mono_upper, int64_t max_cells, Cells *out, std::string &err,
                         size_t window = (size_t)48 << 20) {
    CellsBuilder cb(out, max_cells);
    return stream_text(path, n_threads, err, window, [&](const unsigned char *p, size_t n, bool open_end, int threads, unsigned long long *lines,
                                                         std::string &e) { return parse_text_cells(p, n, open_end, threads, nfr_upper, mono_upper, cb, lines, e); });
}

}  // namespace natac_fragio
