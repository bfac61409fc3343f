// natac_bam_dev.hpp -- BAM -> fragment arrays on the GPU: BGZF members inflated by the device, records walked by the device.
//
// The host extractor (natac_bam.hpp) spends its time in zlib: ~180 MB/s of inflated data per core, 9-18 s for the 100 M
// records behind configs[2] -- several times the whole `occ` run on the accelerated path.  Here the file comes through
// natac_bgzf_dev.hpp's DevWindows: windows of members, staged, inflated one member per lane and CRC-checked on the device.
// This file holds what is a BAM's own: the header, the record walk and the per-reference append.
//
// Records chain through their block_size fields and may start anywhere in a member.  Each lane of the walk kernel finds the
// first record start of ITS member by validation (a chain of plausible records: reference ids, name length and terminator,
// field sizes against block_size), walks to the end of the member and reports where it stopped.  The host then follows
// first/exit through the member table from the one start that is known (the end of the header / of the previous window's
// carry): where a member's guess is not where the chain arrives, that member is walked again from the chain's offset (a
// single-lane launch; more than a few thousand of those per window send the file to the host decoder).  The result is exact
// by induction, not heuristic: a walk that starts at a true record start only visits true record starts.
// Kept reads (proper pair, forward strand: pyatac/fragments.pyx:24-38) are written in file order after a scan of the counts.
#pragma once
#include <memory>
#include "natac_bgzf_dev.hpp"

namespace natac_bamdev {

using natac_bgzfdev::DevWindows;
using natac_bgzfdev::DevBuf;
using natac_bgzfdev::Member;
struct WalkOut { unsigned long long first, exit; unsigned int n_rec, n_kept; };

// ---- kernels -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int ld32(const unsigned char *p) {
    return (unsigned int)p[0] | ((unsigned int)p[1] << 8) | ((unsigned int)p[2] << 16) | ((unsigned int)p[3] << 24);
}

// is [o, ...) a plausible alignment record (SAM spec 4.2)?  n: valid bytes of data.  *next = start of the following record.
__device__ __forceinline__ bool plausible(const unsigned char *data, unsigned long long o, unsigned long long n, int n_ref, unsigned long long *next) {
    if (o + 36 > n) return false;
    const unsigned char *r = data + o;
    const int bs = (int)ld32(r);
    if (bs < 32 || bs > (1 << 28)) return false;
    const int ref = (int)ld32(r + 4), pos = (int)ld32(r + 8);
    const int lname = r[12];
    const int ncig = r[16] | (r[17] << 8);
    const int lseq = (int)ld32(r + 20);
    const int nref = (int)ld32(r + 24), npos = (int)ld32(r + 28);
    if (ref < -1 || ref >= n_ref || nref < -1 || nref >= n_ref || pos < -1 || npos < -1 || lname < 1 || lseq < 0) return false;
    const long long fixed = 32ll + lname + 4ll * ncig + ((long long)lseq + 1) / 2 + lseq;
    if (fixed > bs) return false;
    const unsigned long long nul = o + 36 + (unsigned long long)lname - 1;
    if (nul < n && data[nul] != 0) return false;
    *next = o + 4 + (unsigned long long)bs;
    return true;
}

// pass 0 (write == 0): first record start of every member (member 0: q0, the others by validation), walk to the member's end:
// counts and the exit offset.  pass 1 (write == 1): the same walk from wo[m].first, kept reads written at kept_base[m] + i.
// write == 2: pass 0 for the single member `only` from the given start q0 (the host found the guess of that member wrong).
// A member the host marked void (first == ~0) owns no record.  The walk stops at the first record that is not complete
// inside [0, n): that offset is the carry into the next window.
__global__ void __launch_bounds__(64) bamdev_walk(const unsigned char *__restrict__ data, unsigned long long n, const Member *__restrict__ mem,
                                                  int n_members, unsigned long long q0, int n_ref, int write, int only,
                                                  const unsigned long long *__restrict__ kept_base, WalkOut *__restrict__ wo, int *__restrict__ o_ref,
                                                  int *__restrict__ o_pos, int *__restrict__ o_tlen) {
    int m = blockIdx.x * 64 + threadIdx.x;
    if (write == 2) {
        if (m != 0) return;
        m = only;
        write = 0;
    } else only = 0;
    if (m >= n_members) return;
    const Member mb = mem[m];
    const unsigned long long ustart = mb.uoff, uend = mb.uoff + mb.isize;
    unsigned long long q;
    if (write) {
        q = wo[m].first;
        if (q == ~0ull) return;
    } else {
        WalkOut w;
        w.first = w.exit = ~0ull;
        w.n_rec = w.n_kept = 0;
        if (m == only) q = q0;
        else {
            // the first offset in the member from which CHAIN records validate, or validate exactly up to the end of the data.
            // (A chain that jumps past the end after fewer records is what a misaligned block_size looks like; the rare true
            // start of that kind -- the window's last, incomplete record -- is settled by the host with a write == 2 launch.)
            const int CHAIN = 8;
            q = ~0ull;
            for (unsigned long long o = ustart; o < uend && q == ~0ull; ++o) {
                unsigned long long c = o, nx = 0;
                int ok = 0;
                while (ok < CHAIN && plausible(data, c, n, n_ref, &nx)) { c = nx; ++ok; }
                if (ok == CHAIN || (ok > 0 && c <= n && c + 36 > n)) q = o;
            }
        }
        w.first = w.exit = q;                                   // no start found: ~0 (the host decides whether that matters)
        wo[m] = w;
        if (q == ~0ull) return;
    }
    unsigned int n_rec = 0, n_kept = 0;
    const unsigned long long base = write ? kept_base[m] : 0ull;
    while (q < uend) {
        if (q + 4 > n) break;
        const int bs = (int)ld32(data + q);
        if (bs < 32) { q = ~0ull - 1; break; }                  // malformed: reported through exit, the host rejects the file
        if (q + 4 + (unsigned long long)bs > n) break;          // incomplete inside this window: the carry starts here
        const unsigned char *r = data + q + 4;
        const int ref = (int)ld32(r);
        const unsigned int flag = r[14] | ((unsigned int)r[15] << 8);
        ++n_rec;
        if (ref >= 0 && ref < n_ref && (flag & 0x2u) && !(flag & 0x10u)) {
            if (write) {
                const int tl = (int)ld32(r + 28);
                o_ref[base + n_kept] = ref;
                o_pos[base + n_kept] = (int)ld32(r + 4);
                o_tlen[base + n_kept] = tl < 0 ? -tl : tl;
            }
            ++n_kept;
        }
        q += 4 + (unsigned long long)bs;
    }
    if (!write) {
        wo[m].exit = q;
        wo[m].n_rec = n_rec;
        wo[m].n_kept = n_kept;
    }
}

// ---- host driver ---------------------------------------------------------------------------------------------------------
// What is not a complete record at the end of a window's inflated bytes is carried to the front of the next window's.
// Returns the same object as natac_bamio::decode.  nullptr + err: the file is damaged (same messages as the host decoder);
// nullptr + *undecided = true: the record chain could not be confirmed, the header outgrew a window or a HIP call failed (no
// memory for a window on a shared GPU): the caller uses the host decoder.
inline natac_bamio::Bam *decode_device(const char *path, hipStream_t stream, std::string &err, bool *undecided,
                                       size_t window_bytes = (size_t)8 << 30) {
    using natac_bamio::rdi32;
    *undecided = false;
    std::unique_ptr<natac_bamio::Bam> bam(new natac_bamio::Bam());
    DevBuf d_wo, d_base, d_ref, d_pos, d_tlen;
    std::vector<WalkOut> wo;
    std::vector<unsigned long long> base;
    std::vector<int> h_ref, h_pos, h_tlen;
    std::vector<unsigned char> head;
    DevWindows win;                   // (declared last: it waits for the device before any buffer above is freed)
    auto fail = [&](const std::string &msg) -> natac_bamio::Bam * { err = msg; return nullptr; };
    auto give_up = [&]() -> natac_bamio::Bam * { *undecided = true; return nullptr; };
    // the stream has stopped: a damaged file is reported, a HIP failure is not the file's fault
    auto stopped = [&](const std::string &stop) -> natac_bamio::Bam * { *undecided = !win.file_error; return fail(stop); };
// a HIP failure (typically: no memory left for a window on a shared GPU) is not the file's fault: the host decoder answers
#define BAMDEV_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipGetLastError(); *undecided = true; return fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
    std::string stop = win.open(path, stream, window_bytes, (size_t)512 << 20);
    if (!stop.empty()) return stopped(stop);
    const bool timing = getenv("NATAC_BAM_DEV_TIMING") != nullptr;
    double t_walk = 0, t_chain = 0, t_out = 0;
    bool header_done = false;
    int32_t n_ref = 0;
    const DevWindows::Window &w = win.w;
    for (;;) {
        stop = win.next();
        if (!stop.empty()) return stopped(stop);
        if (w.M == 0) break;                                            // the whole chain is done
        const unsigned char *data = w.data;
        const unsigned long long n = w.n;
        const int M = w.M;
        // ---- header (first window): parsed on the host from the front of the inflated bytes
        unsigned long long q0 = 0;
        if (!header_done) {
            size_t have = (size_t)std::min<unsigned long long>(n, (unsigned long long)8 << 20);
            bool complete = false;
            for (;;) {
                head.resize(have);
                BAMDEV_HIP(hipMemcpy(head.data(), data, have, hipMemcpyDeviceToHost));
                const unsigned char *p = head.data();
                do {
                    if (have < 12) break;
                    if (std::memcmp(p, "BAM\1", 4) != 0) return fail("not a BAM file (bad magic)");
                    size_t hq = 8 + (size_t)(uint32_t)rdi32(p + 4);
                    if (hq + 4 > have) break;
                    n_ref = rdi32(p + hq);
                    hq += 4;
                    if (n_ref < 0) return fail("truncated reference list");
                    std::vector<natac_bamio::Ref> refs((size_t)n_ref);
                    bool ok = true;
                    for (int32_t r = 0; r < n_ref; ++r) {
                        if (hq + 4 > have) { ok = false; break; }
                        const int32_t ln = rdi32(p + hq);
                        if (ln < 1) return fail("truncated reference list");
                        if (hq + 8 + (size_t)ln > have) { ok = false; break; }
                        refs[r].name.assign((const char *)p + hq + 4, (size_t)ln - 1);
                        refs[r].length = rdi32(p + hq + 4 + ln);
                        hq += 8 + (size_t)ln;
                    }
                    if (!ok) break;
                    bam->refs.swap(refs);
                    q0 = hq;
                    complete = true;
                } while (false);
                if (complete || have == n) break;
                have = (size_t)n;
            }
            if (!complete) {
                if (w.eof) return fail(n < 12 ? "not a BAM file (bad magic)" : "truncated BAM header");
                return give_up();          // a header larger than a window: the host decoder streams it
            }
            header_done = true;
        }
        // ---- record walk, pass 0: first / exit / counts per member
        BAMDEV_HIP(d_wo.reserve((size_t)M * sizeof(WalkOut)));
        hipLaunchKernelGGL(bamdev_walk, dim3((M + 63) / 64), dim3(64), 0, stream, data, n, w.d_mem, M, q0, (int)n_ref, 0, 0,
                           (const unsigned long long *)nullptr, (WalkOut *)d_wo.p, (int *)nullptr, (int *)nullptr, (int *)nullptr);
        wo.resize((size_t)M);
        BAMDEV_HIP(hipMemcpyAsync(wo.data(), d_wo.p, (size_t)M * sizeof(WalkOut), hipMemcpyDeviceToHost, stream));
        BAMDEV_HIP(hipStreamSynchronize(stream));
        win.laps.lap(t_walk);
        // ---- the chain from the one known start: every member's guess must be where the previous walk stopped
        base.assign((size_t)M, 0);
        unsigned long long cur = q0, kept = 0, nrec = 0;
        bool stop_walk = false;
        int fixups = 0;
        const int MAX_FIXUPS = 4096;       // per window; beyond that the guesses are systematically off: host decoder
        for (int m = 0; m < M; ++m) {
            const unsigned long long uend = w.mem[m].uoff + w.mem[m].isize;
            if (stop_walk || cur >= uend) { wo[m].first = ~0ull; continue; }                // owns no record
            if (cur + 36 > n && wo[m].first != cur) { wo[m].first = ~0ull; stop_walk = true; continue; }   // an incomplete record header: the carry
            if (wo[m].first != cur) {
                // the guess of this member is not where the chain arrives (a chance pattern before it, or the window's last,
                // incomplete record): `cur` IS a record start, so the member is walked again from there
                if (++fixups > MAX_FIXUPS) return give_up();
                hipLaunchKernelGGL(bamdev_walk, dim3(1), dim3(64), 0, stream, data, n, w.d_mem, M, cur, (int)n_ref, 2, m,
                                   (const unsigned long long *)nullptr, (WalkOut *)d_wo.p, (int *)nullptr, (int *)nullptr, (int *)nullptr);
                BAMDEV_HIP(hipMemcpyAsync(&wo[m], (const WalkOut *)d_wo.p + m, sizeof(WalkOut), hipMemcpyDeviceToHost, stream));
                BAMDEV_HIP(hipStreamSynchronize(stream));
                if (wo[m].first != cur) return give_up();
            }
            if (wo[m].exit == ~0ull - 1) return fail("truncated alignment record");
            base[m] = kept;
            kept += wo[m].n_kept;
            nrec += wo[m].n_rec;
            cur = wo[m].exit;
        }
        bam->n_records += (int64_t)nrec;
        win.laps.lap(t_chain);
        // ---- pass 1: the kept reads in file order
        if (kept) {
            BAMDEV_HIP(d_base.reserve((size_t)M * sizeof(unsigned long long)));
            BAMDEV_HIP(d_ref.reserve(kept * sizeof(int)));
            BAMDEV_HIP(d_pos.reserve(kept * sizeof(int)));
            BAMDEV_HIP(d_tlen.reserve(kept * sizeof(int)));
            BAMDEV_HIP(hipMemcpyAsync(d_wo.p, wo.data(), (size_t)M * sizeof(WalkOut), hipMemcpyHostToDevice, stream));
            BAMDEV_HIP(hipMemcpyAsync(d_base.p, base.data(), (size_t)M * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(bamdev_walk, dim3((M + 63) / 64), dim3(64), 0, stream, data, n, w.d_mem, M, q0, (int)n_ref, 1, 0,
                               (const unsigned long long *)d_base.p, (WalkOut *)d_wo.p, (int *)d_ref.p, (int *)d_pos.p, (int *)d_tlen.p);
            h_ref.resize(kept); h_pos.resize(kept); h_tlen.resize(kept);
            BAMDEV_HIP(hipMemcpyAsync(h_ref.data(), d_ref.p, kept * sizeof(int), hipMemcpyDeviceToHost, stream));
            BAMDEV_HIP(hipMemcpyAsync(h_pos.data(), d_pos.p, kept * sizeof(int), hipMemcpyDeviceToHost, stream));
            BAMDEV_HIP(hipMemcpyAsync(h_tlen.data(), d_tlen.p, kept * sizeof(int), hipMemcpyDeviceToHost, stream));
            BAMDEV_HIP(hipStreamSynchronize(stream));
            for (size_t a = 0; a < kept;) {                   // runs of one reference (a sorted file has one per reference)
                size_t b = a + 1;
                while (b < kept && h_ref[b] == h_ref[a]) ++b;
                natac_bamio::Ref &r = bam->refs[(size_t)h_ref[a]];
                const size_t at = r.pos.size();
                r.pos.resize(at + (b - a));
                r.tlen.resize(at + (b - a));
                for (size_t i = a; i < b; ++i) { r.pos[at + i - a] = h_pos[i]; r.tlen[at + i - a] = h_tlen[i]; }
                a = b;
            }
            bam->n_kept += (int64_t)kept;
        }
        // ---- carry the incomplete tail to the front of the other buffer
        stop = win.carry(cur);
        if (!stop.empty()) return stopped(stop);
        win.laps.lap(t_out);
        if (w.eof) break;
    }
#undef BAMDEV_HIP
    if (timing)
        std::fprintf(stderr, "[natac_bam_dev] read + upload %.3f s, waiting for the member chain %.3f, inflate %.3f, walk %.3f, chain %.3f, kept reads + carry %.3f\n",
                     win.t_read, win.t_chain, win.t_inflate, t_walk, t_chain, t_out);
    if (!header_done) return fail("truncated BAM header");
    if (win.pend != 0) return fail("truncated alignment record");
    return bam.release();
}

}  // namespace natac_bamdev
