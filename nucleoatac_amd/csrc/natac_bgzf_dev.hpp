// natac_bgzf_dev.hpp -- a BGZF file through the GPU, window by window: what the device decoders of a BAM (natac_bam_dev.hpp) and of a
// fragment file (natac_fragfile_dev.hpp) share.
//
// A BGZF file is a sequence of INDEPENDENT raw-deflate members of <= 64 KiB (SAM spec 4.1), tens of thousands per gigabyte.  Here:
//   inflate_member / bamdev_inflate: one LANE inflates one member (RFC 1951: stored, fixed and dynamic blocks, canonical Huffman decode
//     without tables larger than the code itself) and checks its CRC-32, so a window of the file keeps every SIMD of the chip busy with
//     serial decoders.  The decoder is __host__ __device__: the CPU test suite runs the same code.
//   Chain / walk_chain: where every member starts, its payload and inflated sizes, walked on a thread of its own with the host decoder's
//     checks and messages.
//   DevWindows: the file in windows of ~window_bytes of compressed data, one window of inflated bytes after the other; what a decoder
//     does not use up at a window's end (an incomplete record, an unfinished line) is carried to the front of the next one on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "natac_bam.hpp"

namespace natac_bgzfdev {

struct Member { unsigned long long coff; unsigned int csize, isize; unsigned long long uoff; };   // payload offset / sizes / output offset

// ---- raw deflate (RFC 1951), one stream, serial; the same code runs on the host in the CPU test suite ----------------------
// Table storage is a template parameter: on the device the symbol tables of the 64 lanes of a workgroup sit lane-interleaved in
// LDS (element i of a lane at index i * 64 + lane), on the host they are plain arrays.
template <class T, int STRIDE>
struct Strided {
    T *base;
    __host__ __device__ T &operator[](int i) const { return base[i * STRIDE]; }
};

struct BitIn {
    const unsigned char *p;      // readable bytes behind p[n - 1]: see inflate_member
    unsigned int n, pos;
    unsigned long long buf;
    int cnt;
    __host__ __device__ void init(const unsigned char *src, unsigned int len) { p = src; n = len; pos = 0; buf = 0; cnt = 0; }
    __host__ __device__ void refill() {              // >= 32 valid bits afterwards (bytes past the end are never legitimately used:
        if (cnt <= 32) {                             // consumed() exposes a stream that runs over)
            unsigned int w;
            __builtin_memcpy(&w, p + pos, 4);
            buf |= (unsigned long long)w << cnt;
            pos += 4;
            cnt += 32;
        }
    }
    __host__ __device__ unsigned int peek(int k) { refill(); return (unsigned int)(buf & ((1ull << k) - 1ull)); }
    __host__ __device__ void skip(int k) { buf >>= k; cnt -= k; }
    __host__ __device__ unsigned int bits(int k) { const unsigned int v = peek(k); skip(k); return v; }
    __host__ __device__ unsigned int consumed() const { return pos - (unsigned int)(cnt >> 3); }    // whole bytes taken from the input
};

// Canonical Huffman code in the form the decoder wants: for the next 15 stream bits read as a number X with the first bit on top,
// the code has length l = the smallest l with X < lim[l] (lim is non-decreasing), and the symbol is sym[(X >> (15 - l)) + delta[l]].
// lim lives in registers (static indices only), delta / sym / work in the caller's table storage.
// Returns the number of unused code points (0: complete, > 0: incomplete, < 0: over-subscribed).
template <class L8, class T16>
__host__ __device__ inline int build_code(const L8 &length, int first_sym, int n, unsigned int (&lim)[16], const T16 &delta, const T16 &sym,
                                          const T16 &work) {
#pragma unroll
    for (int l = 0; l < 16; ++l) { work[l] = 0; lim[l] = 0; }
    for (int s = 0; s < n; ++s) work[length[first_sym + s]] = (unsigned short)(work[length[first_sym + s]] + 1);
    if (work[0] == n) return 0;                        // no codes at all: every lim stays 0, decoding any symbol fails
    int left = 1;
    unsigned int code = 0, off = 0;
#pragma unroll
    for (int l = 1; l <= 15; ++l) {
        const unsigned int c = work[l];
        left = (left << 1) - (int)c;
        lim[l] = (code + c) << (15 - l);
        delta[l] = (unsigned short)(off - code);        // modulo 2^16: the index sum below is taken modulo 2^16 too
        work[l] = (unsigned short)off;                  // next free slot of this length
        off += c;
        code = (code + c) << 1;
    }
    if (left < 0) return left;
    for (int s = 0; s < n; ++s) {
        const int l = length[first_sym + s];
        if (l != 0) { const unsigned short at = work[l]; sym[at] = (unsigned short)s; work[l] = (unsigned short)(at + 1); }
    }
    return left;
}

// next symbol; -1: the bits are no code
template <class T16>
__host__ __device__ inline int decode_symbol(BitIn &in, const unsigned int (&lim)[16], const T16 &delta, const T16 &sym) {
    const unsigned int x = __builtin_bitreverse32(in.peek(15)) >> 17;
    int l = 1;
#pragma unroll
    for (int k = 1; k <= 14; ++k) l += x >= lim[k] ? 1 : 0;
    if (x >= lim[15]) return -1;
    in.skip(l);
    return sym[(unsigned short)((x >> (15 - l)) + delta[l])];
}

// inflate one member's payload into out[0, isize); 0 ok, otherwise an error code (1 bad block type, 2 stored length, 3 code
// lengths, 4 bad symbol, 5 distance too far, 6 output overrun / short, 7 input overrun).  src needs 32 readable bytes of slack: a valid
// stream reads at most 8 bytes behind its end, a stream that runs over is caught within one symbol (a dynamic header's fixed part and
// first symbol: 11 bytes, plus the reader's 8).
template <class L8, class T16>
__host__ __device__ inline int inflate_member(const unsigned char *src, unsigned int csize, unsigned char *out, unsigned int isize, const L8 &lengths,
                                              const T16 &lsym, const T16 &ldelta, const T16 &lwork, const T16 &dsym, const T16 &ddelta, const T16 &dwork) {
    const unsigned short LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const unsigned char LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const unsigned short DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                      8193, 12289, 16385, 24577};
    const unsigned char DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    const unsigned char ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    unsigned int llim[16], dlim[16];
    BitIn in;
    in.init(src, csize);
    unsigned int o = 0;
    for (;;) {
        const unsigned int last = in.bits(1), type = in.bits(2);
        if (type == 0) {
            in.skip(in.cnt & 7);                                  // to the byte boundary
            const unsigned int len = in.bits(16), nlen = in.bits(16);
            if ((len ^ 0xffffu) != nlen) return 2;
            const unsigned int q = in.consumed();
            if (q + len > csize) return 7;
            if (o + len > isize) return 6;
            for (unsigned int i = 0; i < len; ++i) out[o + i] = src[q + i];
            o += len;
            in.pos = q + len;
            in.buf = 0;
            in.cnt = 0;
        } else if (type == 1 || type == 2) {
            if (type == 1) {
                for (int s = 0; s < 144; ++s) lengths[s] = 8;
                for (int s = 144; s < 256; ++s) lengths[s] = 9;
                for (int s = 256; s < 280; ++s) lengths[s] = 7;
                for (int s = 280; s < 288; ++s) lengths[s] = 8;
                for (int s = 288; s < 318; ++s) lengths[s] = 5;
                build_code(lengths, 0, 288, llim, ldelta, lsym, lwork);
                build_code(lengths, 288, 30, dlim, ddelta, dsym, dwork);
            } else {
                const int nlen = (int)in.bits(5) + 257, ndist = (int)in.bits(5) + 1, ncode = (int)in.bits(4) + 4;
                if (nlen > 286 || ndist > 30) return 3;
                for (int i = 0; i < 19; ++i) lengths[i] = 0;
                for (int i = 0; i < ncode; ++i) lengths[ORDER[i]] = (unsigned char)in.bits(3);
                if (build_code(lengths, 0, 19, llim, ldelta, lsym, lwork) != 0) return 3;      // the code-length code must be complete
                int idx = 0;
                while (idx < nlen + ndist) {
                    const int sym = decode_symbol(in, llim, ldelta, lsym);
                    if (sym < 0) return 4;
                    if (sym < 16) lengths[idx++] = (unsigned char)sym;
                    else {
                        int rep, val = 0;
                        if (sym == 16) {
                            if (idx == 0) return 3;
                            val = lengths[idx - 1];
                            rep = 3 + (int)in.bits(2);
                        } else if (sym == 17) rep = 3 + (int)in.bits(3);
                        else rep = 11 + (int)in.bits(7);
                        if (idx + rep > nlen + ndist) return 3;
                        while (rep--) lengths[idx++] = (unsigned char)val;
                    }
                    if (in.consumed() > csize) return 7;          // a header that runs over must not be read to its end: the slack is 32 bytes
                }
                if (lengths[256] == 0) return 3;                  // no end-of-block code
                // An incomplete set passes only under zlib's rule (inflate_table: its longest code has ONE bit, i.e. it is a single 1-bit
                // code): the host decoder inflates with zlib, and both must refuse the same members.
                int left = build_code(lengths, 0, nlen, llim, ldelta, lsym, lwork);
                int longer = 0;
                for (int s = 0; s < nlen; ++s) longer += lengths[s] > 1;
                if (left < 0 || (left > 0 && longer != 0)) return 3;
                left = build_code(lengths, nlen, ndist, dlim, ddelta, dsym, dwork);
                longer = 0;
                for (int s = 0; s < ndist; ++s) longer += lengths[nlen + s] > 1;
                if (left < 0 || (left > 0 && longer != 0)) return 3;
            }
            for (;;) {
                int sym = decode_symbol(in, llim, ldelta, lsym);
                if (sym < 0) return 4;
                if (sym < 256) {
                    if (o >= isize) return 6;
                    out[o++] = (unsigned char)sym;
                } else if (sym == 256) break;
                else {
                    sym -= 257;
                    if (sym >= 29) return 4;
                    const unsigned int len = LBASE[sym] + in.bits(LEXT[sym]);
                    const int ds = decode_symbol(in, dlim, ddelta, dsym);
                    if (ds < 0 || ds >= 30) return 4;
                    const unsigned int dist = DBASE[ds] + in.bits(DEXT[ds]);
                    if (dist > o) return 5;
                    if (o + len > isize) return 6;
                    unsigned int i = 0;
                    if (dist >= 4)                                // whole words while source and destination do not overlap within one
                        for (; i + 4 <= len; i += 4) {
                            unsigned int w;
                            __builtin_memcpy(&w, out + o + i - dist, 4);
                            __builtin_memcpy(out + o + i, &w, 4);
                        }
                    for (; i < len; ++i) out[o + i] = out[o + i - dist];
                    o += len;
                }
                if (in.consumed() > csize) return 7;
            }
        } else return 1;
        if (in.consumed() > csize) return 7;
        if (last) break;
    }
    return o == isize ? 0 : 6;
}

// the decoder with plain arrays (host test entry)
inline int inflate_member_host(const unsigned char *src, unsigned int csize, unsigned char *out, unsigned int isize) {
    unsigned char lengths[320];
    unsigned short lsym[288], ldelta[16], lwork[16], dsym[32], ddelta[16], dwork[16];
    typedef Strided<unsigned char, 1> L8;
    typedef Strided<unsigned short, 1> T16;
    return inflate_member(src, csize, out, isize, L8{lengths}, T16{lsym}, T16{ldelta}, T16{lwork}, T16{dsym}, T16{ddelta}, T16{dwork});
}

// ---- kernels -------------------------------------------------------------------------------------------------------------
// one lane per member, 64 lanes per workgroup; the symbol tables of a lane are lane-interleaved in LDS (48 KiB per workgroup), the
// code lengths of a block header -- touched only while a block's tables are built -- stay in private memory.
// status[0] = first error code (0 = none), status[1] = its member
constexpr int INFLATE_LDS_U16 = (288 + 32 + 4 * 16) * 64;
// A launch covers the members [m_begin, n_members) whose bytes have arrived; it fills the chip at most once (3 workgroups per CU: the
// LDS tables) and every lane takes members from the launch's queue until it is empty: a serial decoder needs ~85 ms per 64-KiB member, so with one member per lane a launch of 55 k members took two rounds
// of 49 k lanes, the second nearly empty.
// CRC-32 (IEEE, reflected) of p[0, n) with the slicing-by-8 tables t8[8][256] (t8[0] = the byte table): eight independent lookups
// per 8 bytes, so the dependent chain is one load per 8 bytes -- ~0.5 ms for a 64-KiB member next to the ~85 ms its inflate takes
__device__ __forceinline__ unsigned int crc32_slice8(const unsigned int *__restrict__ t8, const unsigned char *p, unsigned int n) {
    unsigned int c = 0xffffffffu;
    while (n && ((uintptr_t)p & 7)) { c = t8[(c ^ *p++) & 0xff] ^ (c >> 8); --n; }
    for (; n >= 8; n -= 8, p += 8) {
        const unsigned long long w = *(const unsigned long long *)p;
        const unsigned int lo = (unsigned int)w ^ c, hi = (unsigned int)(w >> 32);
        c = t8[7 * 256 + (lo & 0xff)] ^ t8[6 * 256 + ((lo >> 8) & 0xff)] ^ t8[5 * 256 + ((lo >> 16) & 0xff)] ^ t8[4 * 256 + (lo >> 24)] ^
            t8[3 * 256 + (hi & 0xff)] ^ t8[2 * 256 + ((hi >> 8) & 0xff)] ^ t8[1 * 256 + ((hi >> 16) & 0xff)] ^ t8[hi >> 24];
    }
    while (n) { c = t8[(c ^ *p++) & 0xff] ^ (c >> 8); --n; }
    return c ^ 0xffffffffu;
}
inline void crc32_slice8_tables(unsigned int *t8) {       // host: the tables above
    for (unsigned int i = 0; i < 256; ++i) {
        unsigned int c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xedb88320u : c >> 1;
        t8[i] = c;
    }
    for (int s = 1; s < 8; ++s)
        for (unsigned int i = 0; i < 256; ++i) t8[s * 256 + i] = t8[(s - 1) * 256 + i] >> 8 ^ t8[t8[(s - 1) * 256 + i] & 0xff];
}

// error code 8 (inflate_member's own end at 7, input overrun): the member inflated to ISIZE bytes but its CRC-32 (the four bytes behind
// the payload, RFC 1952) does not match
__global__ void __launch_bounds__(64) bamdev_inflate(const unsigned char *__restrict__ raw, const Member *__restrict__ mem, int m_begin, int n_members,
                                                     unsigned char *__restrict__ data, int *__restrict__ status, int *__restrict__ queue,
                                                     const unsigned int *__restrict__ crc_t8) {
    __shared__ unsigned short tab[INFLATE_LDS_U16];
    unsigned char lengths[320];
    typedef Strided<unsigned char, 1> L8;
    typedef Strided<unsigned short, 64> T16;
    unsigned short *t = tab + threadIdx.x;
    for (;;) {
        const int m = m_begin + atomicAdd(queue, 1);
        if (m >= n_members) break;
        const Member mb = mem[m];
        const unsigned char *tr = raw + mb.coff + mb.csize;              // trailer: CRC-32, ISIZE
        const unsigned int want = (unsigned int)tr[0] | ((unsigned int)tr[1] << 8) | ((unsigned int)tr[2] << 16) | ((unsigned int)tr[3] << 24);
        int rc = 0;
        if (mb.isize == 0) rc = want == 0 ? 0 : 8;
        else {
            rc = inflate_member(raw + mb.coff, mb.csize, data + mb.uoff, mb.isize, L8{lengths}, T16{t}, T16{t + 288 * 64}, T16{t + 304 * 64},
                                T16{t + 320 * 64}, T16{t + 352 * 64}, T16{t + 368 * 64});
            if (rc == 0 && crc32_slice8(crc_t8, data + mb.uoff, mb.isize) != want) rc = 8;
        }
        if (rc != 0 && atomicCAS(&status[0], 0, rc) == 0) status[1] = m;
    }
}

// ---- device memory, and the chain of members ------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    // at least n bytes; the first `keep` bytes survive a reallocation
    hipError_t reserve(size_t n, size_t keep = 0, hipStream_t stream = nullptr) {
        if (n <= cap) return hipSuccess;
        const size_t want = n + n / 8 + 4096;
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, want);
        if (e != hipSuccess) return e;
        if (p && keep) {
            e = hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) { (void)hipFree(q); return e; }
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = want;
        return hipSuccess;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

// The BGZF chain of a file (where every member starts, its payload and inflated sizes), walked with one small pread per member on a
// thread of its own while the bulk of the file goes to the device; the same checks and messages as the host decoder's window scan.
struct Chain {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Member> members;          // coff = ABSOLUTE file offset of the deflate payload; uoff unused here
    std::vector<unsigned long long> ends;  // absolute end offset of every member
    bool done = false;
    std::string error;
};

inline void walk_chain(int fd, unsigned long long fsize, Chain *ch) {
    using natac_bamio::rd16;
    using natac_bamio::rd32;
    std::vector<Member> part;
    std::vector<unsigned long long> part_end;
    auto publish = [&](bool done, const std::string &error) {
        std::lock_guard<std::mutex> lk(ch->mu);
        ch->members.insert(ch->members.end(), part.begin(), part.end());
        ch->ends.insert(ch->ends.end(), part_end.begin(), part_end.end());
        part.clear(); part_end.clear();
        if (done) { ch->done = true; ch->error = error; }
        ch->cv.notify_all();
    };
    unsigned long long off = 0;
    bool any = false;
    unsigned char h[4 + 1024];
    while (off < fsize) {
        if (off + 18 > fsize) return publish(true, any ? "trailing bytes after the last BGZF block" : "not a BGZF file (bad block header)");
        // the last four bytes of the previous member (its ISIZE) and this member's header in one read
        const unsigned long long from = off >= 4 ? off - 4 : 0;
        const size_t want = (size_t)std::min<unsigned long long>(sizeof h, fsize - from);
        if (pread(fd, h, want, (off_t)from) != (ssize_t)want) return publish(true, "read error");
        const unsigned char *g = h + (off - from);
        const size_t have = want - (size_t)(off - from);
        if (any) {
            const uint32_t isize = rd32(g - 4);
            if (isize > 65536) return publish(true, "corrupt BGZF block (ISIZE > 65536)");
            part.back().isize = isize;
        }
        if (g[0] != 0x1f || g[1] != 0x8b || g[2] != 8 || !(g[3] & 4)) return publish(true, "not a BGZF file (bad block header)");
        const unsigned xlen = rd16(g + 10);
        if (12 + (size_t)xlen > have) {
            if (off + 12 + xlen > fsize) return publish(true, any ? "trailing bytes after the last BGZF block" : "not a BGZF file (bad block header)");
            return publish(true, "BGZF extra field longer than 1 KiB");      // never written by samtools / htslib / this writer
        }
        size_t bsize = 0;
        for (size_t x = 12; x + 4 <= 12 + (size_t)xlen;) {
            const unsigned slen = rd16(g + x + 2);
            if (g[x] == 'B' && g[x + 1] == 'C' && slen == 2) bsize = (size_t)rd16(g + x + 4) + 1;
            x += 4 + slen;
        }
        if (!bsize || bsize < 12 + (size_t)xlen + 8) return publish(true, "truncated BGZF block");
        if (off + bsize > fsize) return publish(true, any ? "trailing bytes after the last BGZF block" : "not a BGZF file (bad block header)");
        if (part.size() >= 4096) publish(false, "");
        part.push_back({off + 12 + xlen, (unsigned int)(bsize - 12 - xlen - 8), 0u, 0ull});
        part_end.push_back(off + bsize);
        off += bsize;
        any = true;
    }
    if (any) {
        unsigned char t[4];
        if (pread(fd, t, 4, (off_t)(fsize - 4)) != 4) return publish(true, "read error");
        const uint32_t isize = rd32(t);
        if (isize > 65536) return publish(true, "corrupt BGZF block (ISIZE > 65536)");
        part.back().isize = isize;
    }
    publish(true, any ? "" : "not a BGZF file (bad block header)");
}

// ---- the file in windows --------------------------------------------------------------------------------------------------
// for code that returns "" or the reason it stops: expr is a HIP call (a failed one is the reason) or another such piece of code
inline std::string stop_reason(hipError_t e, const char *expr) {
    if (e == hipSuccess) return std::string();
    (void)hipGetLastError();
    return std::string(expr) + ": " + hipGetErrorString(e);
}
inline std::string stop_reason(const std::string &reason, const char *) { return reason; }
#define NATAC_DEV_TRY(expr) do { const std::string s_ = natac_bgzfdev::stop_reason((expr), #expr); if (!s_.empty()) return s_; } while (0)

// wall-clock phases of a decode (NATAC_BAM_DEV_TIMING, NATAC_FRAG_DEV_TIMING): lap(acc) adds the time since the last lap to acc
struct Laps {
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    double t0 = now();
    void lap(double &acc) { const double t = now(); acc += t - t0; t0 = t; }
};

// The file goes through the device in windows of ~window_bytes of compressed data: as many members as end inside
// win_start + window_bytes (at least one), once the chain walk has got that far.  A window's bytes are read into two small pinned
// staging buffers (pinning memory costs ~0.25 s per GiB: a window-sized pinned buffer took longer to allocate than the whole decode),
// the read of one overlapping the upload of the other; the members of every subwin_bytes that have arrived are inflated on a side
// stream while the rest of the window is still being read.
// open / next / carry return "" or what ends the stream; `file_error` then tells a damaged or unreadable file (the chain's error, "read
// error", a member that does not inflate or fails its CRC-32: the host decoders' messages) from a failed HIP call (typically: no memory
// left for a window on a shared GPU), which is not the file's fault.
struct DevWindows {
    struct Window {
        unsigned char *data = nullptr;      // device: the carry of the window before at the front, then the members' inflated bytes
        unsigned long long n = 0;           // bytes of data
        const Member *mem = nullptr;        // host: the members, coff relative to the window's start, uoff into data
        const Member *d_mem = nullptr;      // the same on the device
        int M = 0;                          // members; 0: the chain is done, there is no window
        size_t m0 = 0;                      // the first member's index in the chain
        bool eof = false;                   // the window ends the file
    } w;                                    // the last window next() yielded

    bool file_error = false;
    unsigned long long pend = 0;            // carried bytes at the front of the next window's data
    Laps laps;
    double t_read = 0, t_chain = 0, t_inflate = 0;      // read + upload, waiting for the member chain, inflate

    // safe after any partial open: nothing is freed before the walker has stopped reading the file and the device has finished with the buffers
    ~DevWindows() {
        if (walker.joinable()) walker.join();
        for (int i = 0; i < 3; ++i) if (aux[i]) (void)hipStreamSynchronize(aux[i]);
        if (fd >= 0) (void)hipStreamSynchronize(stream);
        for (int i = 0; i < 2; ++i) { if (stage[i]) (void)hipHostFree(stage[i]); if (staged[i]) (void)hipEventDestroy(staged[i]); }
        for (int i = 0; i < 3; ++i) if (aux[i]) (void)hipStreamDestroy(aux[i]);
        if (fd >= 0) close(fd);
    }

    std::string open(const char *path, hipStream_t caller, size_t window, size_t subwin) {
        stream = caller;
        window_bytes = std::max<size_t>(window, (size_t)4096);
        subwin_bytes = subwin;
        fd = ::open(path, O_RDONLY);
        if (fd < 0) return bad_file(std::string("cannot open ") + path);
        struct stat sb;
        if (fstat(fd, &sb) != 0) return bad_file("cannot size the file");
        fsize = (unsigned long long)sb.st_size;
        stage_bytes = (size_t)std::min<unsigned long long>((unsigned long long)32 << 20, std::max<unsigned long long>(fsize, 4096));
        walker = std::thread(walk_chain, fd, fsize, &chain);
        for (int i = 0; i < 2; ++i) {
            NATAC_DEV_TRY(hipHostMalloc((void **)&stage[i], stage_bytes, hipHostMallocDefault));
            NATAC_DEV_TRY(hipEventCreateWithFlags(&staged[i], hipEventDisableTiming));
        }
        for (int i = 0; i < 3; ++i) NATAC_DEV_TRY(hipStreamCreateWithFlags(&aux[i], hipStreamNonBlocking));
        NATAC_DEV_TRY(d_status.reserve(4 * sizeof(int)));
        {
            std::vector<unsigned int> t8(8 * 256);
            crc32_slice8_tables(t8.data());
            NATAC_DEV_TRY(d_crc.reserve(t8.size() * sizeof(unsigned int)));
            NATAC_DEV_TRY(hipMemcpyAsync(d_crc.p, t8.data(), t8.size() * sizeof(unsigned int), hipMemcpyHostToDevice, stream));
            NATAC_DEV_TRY(hipStreamSynchronize(stream));      // t8 is a local
        }
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
        laps.t0 = Laps::now();
        return std::string();
    }

    // the next window into w, inflated and CRC-checked
    std::string next() {
        // ---- the members of this window: as many as fit window_bytes (at least one), once the chain walk has got that far
        // (every member the walker has published carries its ISIZE)
        size_t m1 = m0;
        unsigned long long win_end = win_start;
        {
            std::unique_lock<std::mutex> lk(chain.mu);
            chain.cv.wait(lk, [&]() { return chain.done || (!chain.ends.empty() && chain.ends.back() >= win_start + window_bytes); });
            if (!chain.error.empty()) return bad_file(chain.error);
            while (m1 < chain.ends.size() && (m1 == m0 || chain.ends[m1] <= win_start + window_bytes)) ++m1;
            mem.assign(chain.members.begin() + (long)m0, chain.members.begin() + (long)m1);
            if (m1 > m0) win_end = chain.ends[m1 - 1];
        }
        const int M = w.M = (int)mem.size();
        if (M == 0) return std::string();                               // the whole chain is done
        unsigned long long n = pend;
        for (auto &mb : mem) { mb.coff -= win_start; mb.uoff = n; n += mb.isize; }
        const size_t o = (size_t)(win_end - win_start);
        laps.lap(t_chain);
        // ---- upload (read of one staging buffer next to the copy of the other) + inflate: the members of every subwin_bytes that
        // have arrived are launched on a side stream while the rest of the window is still being read
        NATAC_DEV_TRY(d_raw.reserve(o + 64));
        NATAC_DEV_TRY(d_mem.reserve(mem.size() * sizeof(Member)));
        NATAC_DEV_TRY(d_data[cur_buf].reserve((size_t)n + 64, (size_t)pend, stream));      // the carry at the front stays
        unsigned char *data = (unsigned char *)d_data[cur_buf].p;
        const int max_launches = (int)(o / subwin_bytes) + 2;
        NATAC_DEV_TRY(d_queue.reserve((size_t)max_launches * sizeof(int)));
        NATAC_DEV_TRY(hipMemcpyAsync(d_mem.p, mem.data(), mem.size() * sizeof(Member), hipMemcpyHostToDevice, stream));
        NATAC_DEV_TRY(hipMemsetAsync(d_status.p, 0, 4 * sizeof(int), stream));
        NATAC_DEV_TRY(hipMemsetAsync(d_queue.p, 0, (size_t)max_launches * sizeof(int), stream));
        {
            int which = 0, launched = 0, n_launch = 0;
            size_t since = 0;
            for (size_t at = 0; at < o; which ^= 1) {
                const size_t len = std::min(stage_bytes, o - at);
                NATAC_DEV_TRY(hipEventSynchronize(staged[which]));      // the copy that used this buffer last has finished
                {   // four concurrent preads fill the staging buffer (one thread copies out of the page cache at ~5 GB/s)
                    const int RT = len >= ((size_t)4 << 20) ? 4 : 1;
                    bool bad[4] = {false, false, false, false};
                    auto fill = [&](int t) {
                        size_t a = len * (size_t)t / (size_t)RT;
                        const size_t b = len * ((size_t)t + 1) / (size_t)RT;
                        while (a < b) {
                            const ssize_t r = pread(fd, stage[which] + a, b - a, (off_t)(win_start + at + a));
                            if (r <= 0) { bad[t] = true; return; }
                            a += (size_t)r;
                        }
                    };
                    std::thread th[3];
                    for (int t = 1; t < RT; ++t) th[t - 1] = std::thread(fill, t);
                    fill(0);
                    for (int t = 1; t < RT; ++t) th[t - 1].join();
                    if (bad[0] || bad[1] || bad[2] || bad[3]) return bad_file("read error");
                }
                NATAC_DEV_TRY(hipMemcpyAsync((unsigned char *)d_raw.p + at, stage[which], len, hipMemcpyHostToDevice, stream));
                NATAC_DEV_TRY(hipEventRecord(staged[which], stream));
                at += len;
                since += len;
                if (since >= subwin_bytes || at == o) {
                    int upto = launched;                                // members that lie completely inside the uploaded bytes
                    while (upto < M && mem[(size_t)upto].coff + mem[(size_t)upto].csize + 8 <= at) ++upto;
                    if (at == o) upto = M;
                    if (upto > launched) {
                        hipStream_t side = aux[n_launch % 3];
                        NATAC_DEV_TRY(hipStreamWaitEvent(side, staged[which], 0));
                        const int cnt = upto - launched;
                        hipLaunchKernelGGL(bamdev_inflate, dim3((unsigned)std::min<long long>((cnt + 63) / 64, 3ll * n_cu)), dim3(64), 0, side,
                                           (const unsigned char *)d_raw.p, (const Member *)d_mem.p, launched, upto, data, (int *)d_status.p,
                                           (int *)d_queue.p + n_launch, (const unsigned int *)d_crc.p);
                        launched = upto;
                        ++n_launch;
                        since = 0;
                    }
                }
            }
        }
        laps.lap(t_read);
        for (int i = 0; i < 3; ++i) NATAC_DEV_TRY(hipStreamSynchronize(aux[i]));
        int st[2] = {0, 0};
        NATAC_DEV_TRY(hipMemcpyAsync(st, d_status.p, sizeof st, hipMemcpyDeviceToHost, stream));
        NATAC_DEV_TRY(hipStreamSynchronize(stream));
        if (st[0] == 8) {      // the member's file offset: where the previous member of the chain ends
            unsigned long long at = 0;
            { std::lock_guard<std::mutex> lk(chain.mu); if (m0 + (size_t)st[1] > 0) at = chain.ends[m0 + (size_t)st[1] - 1]; }
            return bad_file("CRC-32 mismatch in the BGZF member at file offset " + std::to_string(at) + " (corrupt file)");
        }
        if (st[0] != 0) return bad_file("inflate failed (corrupt BGZF block)");
        w.data = data;
        w.n = n;
        w.mem = mem.data();
        w.d_mem = (const Member *)d_mem.p;
        w.m0 = m0;
        w.eof = win_end == fsize;
        win_start = win_end;
        m0 = m1;
        laps.lap(t_inflate);
        return std::string();
    }

    // what the decoder has not used up -- w's bytes from `cur` on -- goes to the front of the other buffer: the next window's
    std::string carry(unsigned long long cur) {
        pend = w.n - cur;
        NATAC_DEV_TRY(d_data[cur_buf ^ 1].reserve((size_t)pend + 64));
        if (pend) NATAC_DEV_TRY(hipMemcpyAsync(d_data[cur_buf ^ 1].p, w.data + cur, (size_t)pend, hipMemcpyDeviceToDevice, stream));
        NATAC_DEV_TRY(hipStreamSynchronize(stream));
        cur_buf ^= 1;
        return std::string();
    }

  private:
    std::string bad_file(const std::string &msg) { file_error = true; return msg; }

    int fd = -1;
    unsigned long long fsize = 0;
    hipStream_t stream = nullptr;
    size_t window_bytes = 0, subwin_bytes = 0, stage_bytes = 0;
    Chain chain;
    std::thread walker;
    unsigned char *stage[2] = {nullptr, nullptr};
    hipEvent_t staged[2] = {nullptr, nullptr};
    hipStream_t aux[3] = {nullptr, nullptr, nullptr};
    DevBuf d_raw, d_mem, d_data[2], d_queue, d_crc, d_status;      // d_status: bamdev_inflate's status words, zeroed for every window
    std::vector<Member> mem;
    int cur_buf = 0, n_cu = 256;
    unsigned long long win_start = 0;       // file offset of the next window = start of its first member
    size_t m0 = 0;                          // its first member in the chain
};

}  // namespace natac_bgzfdev
