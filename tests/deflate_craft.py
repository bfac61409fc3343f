"""Raw-deflate streams written from explicit instructions (RFC 1951), and BGZF members around them (RFC 1952 + SAM spec 4.1), for
the tests of the device BAM decoder.  A compressor chooses what it emits; here the test does: block types and their order, the code
lengths of the three alphabets of a dynamic block, how those lengths are run-length coded, and every literal / match token.  The bytes
a stream must inflate to are computed from the tokens, never by inflating.  Plain Python; all tables come from the RFC's arithmetic."""
import struct
import zlib          # crc32 of a BGZF member only

# length symbols 257..285 and distance symbols 0..29: (symbol, base, extra bits).  RFC 1951 3.2.5: after the first eight (four) symbols the
# number of extra bits grows by one every four (two) symbols; 285 is length 258 on its own.
LEN_SYMS = []
_b = 3
for _i in range(28):
    _e = max(0, (_i - 4) // 4)
    LEN_SYMS.append((257 + _i, _b, _e))
    _b += 1 << _e
LEN_SYMS.append((285, 258, 0))
DIST_SYMS = []
_b = 1
for _i in range(30):
    _e = max(0, (_i - 2) // 2)
    DIST_SYMS.append((_i, _b, _e))
    _b += 1 << _e
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32           # 30 and 31 have codes and no meaning


def len_symbol(length, sym=None):
    """(symbol, base, extra bits) of a match length; 258 is symbol 285 unless sym=284 asks for 227 + 31"""
    if length == 258 and sym != 284:
        return LEN_SYMS[28]
    for s, b, e in LEN_SYMS[:28]:
        if b <= length < b + (1 << e):
            return s, b, e
    raise ValueError(length)


def dist_symbol(dist):
    for s, b, e in DIST_SYMS:
        if b <= dist < b + (1 << e):
            return s, b, e
    raise ValueError(dist)


def canon(lengths):
    """canonical codes of RFC 1951 3.2.2, each already bit-reversed for an LSB-first writer; None where the length is 0.
    An over-subscribed set still gets (overflowing) codes: such a block is rejected at its header"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 17):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
            continue
        c, r = nxt[l] & ((1 << l) - 1), 0
        nxt[l] += 1
        for _ in range(l):
            r, c = (r << 1) | (c & 1), c >> 1
        out.append(r)
    return out


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, k):
        self.acc |= v << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def nbits(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def rle_plain(lengths):
    return [(l,) for l in lengths]


def rle_greedy(lengths):
    """the longest repeat at every position: 18 / 17 for zeros, 16 for a repeated nonzero length"""
    ops, i, n = [], 0, len(lengths)
    while i < n:
        j = i
        while j < n and lengths[j] == lengths[i]:
            j += 1
        run = j - i
        if lengths[i] == 0 and run >= 3:
            r = min(run, 138)
            ops.append((18, r) if r >= 11 else (17, r))
            i += r
        elif lengths[i] != 0 and run >= 4:
            ops.append((lengths[i],))
            r = min(run - 1, 6)
            ops.append((16, r))
            i += 1 + r
        else:
            ops.append((lengths[i],))
            i += 1
    return ops


def balanced(k):
    """k >= 2 code lengths of a complete code, as equal as possible"""
    b = k.bit_length() - 1
    return [b] * ((2 << b) - k) + [b + 1] * (2 * (k - (1 << b)))


def random_code(rng, k, maxbits, deep=False):
    """k code lengths of a random complete prefix code (k = 1: the one incomplete set deflate allows, a single 1-bit code): random Kraft
    splits of a leaf into two one level down.  deep: split the deepest leaf first until a code of maxbits bits exists"""
    if k == 1:
        return [1]
    d = [1, 1]
    while len(d) < k:
        can = [i for i, x in enumerate(d) if x < maxbits]
        i = max(can, key=lambda j: d[j]) if deep and max(d) < maxbits else can[int(rng.integers(len(can)))]
        d[i] += 1
        d.append(d[i])
    return d


def code_over(rng, symbols, maxbits=15, deep=False):
    """code lengths (a list up to the highest symbol) of a random complete code over exactly `symbols`"""
    symbols = sorted(symbols)
    d = random_code(rng, len(symbols), maxbits, deep)
    d = [d[i] for i in rng.permutation(len(d))]
    out = [0] * (symbols[-1] + 1)
    for s, l in zip(symbols, d):
        out[s] = l
    return out


def used_symbols(tokens):
    ls, ds = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        else:
            ls.add(len_symbol(t[0], t[2] if len(t) > 2 else None)[0])
            ds.add(dist_symbol(t[1])[0])
    return ls, ds


def alphabets(rng, tokens, maxbits=15, deep=False, spare=0):
    """(literal/length lengths, distance lengths) of random complete codes that cover the tokens and `spare` unused symbols"""
    ls, ds = used_symbols(tokens)
    for _ in range(spare):
        ls.add(int(rng.integers(0, 286)))
        ds.add(int(rng.integers(0, 30)))
    ll = code_over(rng, ls, maxbits, deep)
    ll += [0] * (257 - len(ll))
    dl = code_over(rng, ds, maxbits, deep) if ds else [0]
    return ll, dl


def tokenize(data, policy="greedy", rng=None):
    """bytes -> tokens.  none: literals only; greedy: the most recent earlier occurrence of the next three bytes, extended as far as it
    goes; far: the earliest occurrence inside the 32 KiB history instead; dist1: only runs of one byte, as distance-1 copies"""
    data = bytes(data)
    n, i, toks = len(data), 0, []
    if policy == "none":
        return list(data)
    seen = {}
    while i < n:
        m = None
        if policy == "dist1":
            if i > 0 and data[i] == data[i - 1]:
                m = i - 1
        elif i + 3 <= n:
            cand = seen.get(data[i:i + 3])
            if policy == "far" and cand:
                while cand and i - cand[0] > 32768:
                    cand.pop(0)
                m = cand[0] if cand else None
            elif cand and i - cand[-1] <= 32768:
                m = cand[-1]
        ln = 0
        if m is not None:
            while ln < 258 and i + ln < n and data[m + ln] == data[i + ln]:
                ln += 1
        if ln >= 3 and rng is not None and ln > 3 and rng.integers(4) == 0:
            ln = int(rng.integers(3, ln + 1))                    # a shorter copy than possible, now and then
        step = ln if ln >= 3 else 1
        toks.append((ln, i - m) if ln >= 3 else data[i])
        if policy != "dist1":
            for j in range(i, min(i + step, n - 2)):
                seen.setdefault(data[j:j + 3], []).append(j)
        i += step
    return toks


class Stream:
    """one raw-deflate stream under construction: .w the bits, .out what they must inflate to (None once a token says something no
    decoder can follow: a distance past the start of the output, a raw symbol)"""

    def __init__(self):
        self.w, self.out, self.headers = BitWriter(), bytearray(), []       # headers: [first bit, end bit) of every block header

    def header(self, final, btype):
        self.headers.append([self.w.nbits(), self.w.nbits() + 3])
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, length=None, nlen=None):
        """LEN and NLEN are written as given (default: len(data) and its complement), then the data bytes"""
        self.header(final, 0)
        self.w.align()
        length = len(data) if length is None else length
        self.w.bits(length, 16)
        self.w.bits((length ^ 0xffff) if nlen is None else nlen, 16)
        self.headers[-1][1] = self.w.nbits()
        self.w.out += data
        if self.out is not None:
            self.out += data
        return self

    def _body(self, tokens, ll, dl, eob):
        lc, dc, w = canon(ll), canon(dl), self.w
        for t in tokens:
            if isinstance(t, int):
                w.bits(lc[t], ll[t])
                if self.out is not None:
                    self.out.append(t)
            elif t[0] == "L":                        # a bare literal/length symbol, ("D", s) a bare distance symbol, ("X", v, k) k raw bits
                w.bits(lc[t[1]], ll[t[1]])
                self.out = None
            elif t[0] == "D":
                w.bits(dc[t[1]], dl[t[1]])
                self.out = None
            elif t[0] == "X":
                w.bits(t[1], t[2])
            else:
                s, b, e = len_symbol(t[0], t[2] if len(t) > 2 else None)
                w.bits(lc[s], ll[s])
                w.bits(t[0] - b, e)
                s, b, e = dist_symbol(t[1])
                w.bits(dc[s], dl[s])
                w.bits(t[1] - b, e)
                if self.out is not None and t[1] > len(self.out):
                    self.out = None
                if self.out is not None:
                    for _ in range(t[0]):
                        self.out.append(self.out[-t[1]])
        if eob:
            w.bits(lc[256], ll[256])

    def fixed(self, tokens, final=False, eob=True):
        self.header(final, 1)
        self._body(tokens, FIXED_LL, FIXED_DL, eob)
        return self

    def dynamic(self, ll, dl, tokens, final=False, rle=None, cl=None, hclen=None, hlit=None, hdist=None, eob=True):
        """ll / dl: the code lengths of the literal/length and the distance alphabet (HLIT / HDIST = their sizes unless given);
        rle: the code-length symbols for ll + dl, [(length,) | (16, 3..6) | (17, 3..10) | (18, 11..138)] (default: rle_greedy);
        cl: the 19 lengths of the code-length code (default: a balanced complete code over the symbols rle uses);
        hclen: how many of them are sent (default: up to the last nonzero one in transmission order)"""
        rle = rle_greedy(list(ll) + list(dl)) if rle is None else rle
        if cl is None:
            used = sorted({op[0] for op in rle} | ({0, 18} if len({op[0] for op in rle}) < 2 else set()))
            cl = [0] * 19
            for s, l in zip(used, balanced(max(2, len(used)))):
                cl[s] = l
        if hclen is None:
            hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl[s]))
        self.header(final, 2)
        w = self.w
        w.bits((len(ll) if hlit is None else hlit) - 257, 5)
        w.bits((len(dl) if hdist is None else hdist) - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl[s], 3)
        cc = canon(cl)
        for op in rle:
            w.bits(cc[op[0]], cl[op[0]])
            if op[0] == 16:
                w.bits(op[1] - 3, 2)
            elif op[0] == 17:
                w.bits(op[1] - 3, 3)
            elif op[0] == 18:
                w.bits(op[1] - 11, 7)
        self.headers[-1][1] = w.nbits()
        self._body(tokens, list(ll) + [0] * (288 - len(ll)), list(dl) + [0] * (32 - len(dl)), eob)
        return self

    def finish(self):
        """(stream, the bytes it inflates to or None)"""
        return self.w.bytes(), None if self.out is None else bytes(self.out)


def bgzf_member(payload, data=b"", crc=None, isize=None, pre=(), post=(), mtime=0, xfl=0, os_=0xff):
    """a BGZF member around any payload; pre / post: extra subfields (two id bytes, content) before / after BC; the CRC and ISIZE fields
    are those of `data` unless given"""
    sub = lambda f: bytes(f[0]) + struct.pack("<H", len(f[1])) + f[1]
    before, after = b"".join(sub(f) for f in pre), b"".join(sub(f) for f in post)
    xlen = len(before) + 6 + len(after)
    bsize = 12 + xlen + len(payload) + 8
    assert bsize <= 65536, bsize
    head = bytes([0x1f, 0x8b, 8, 4]) + struct.pack("<IBBH", mtime, xfl, os_, xlen) + before + b"BC" + struct.pack("<HH", 2, bsize - 1) + after
    return head + payload + struct.pack("<II", (zlib.crc32(data) & 0xffffffff) if crc is None else crc, len(data) if isize is None else isize)


BGZF_EOF = bgzf_member(bytes([3, 0]))


# ---- member encoders: one way each of writing given bytes as one valid stream (the strategies of the heterogeneous-workgroup test and of
# tests/fuzz/fuzz_bam.py).  Every one returns a payload whose Stream.out was checked against the input.
def _split(rng, data, k):
    cuts = sorted(int(c) for c in rng.integers(0, len(data) + 1, k - 1))
    return [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]


def enc_stored(rng, data):
    s = Stream()
    parts = [q for p in _split(rng, data, 1 + int(rng.integers(3))) for q in (p[:32768], p[32768:]) if q or len(p) == 0]
    for i, p in enumerate(parts):
        s.stored(p, final=i == len(parts) - 1)
    return s


def enc_fixed(rng, data):
    return Stream().fixed(tokenize(data, "greedy", rng), final=True)


def enc_dynamic_short(rng, data):
    t = tokenize(data, "greedy", rng)
    return Stream().dynamic(*alphabets(rng, t, maxbits=9), t, final=True)


def enc_dynamic_deep(rng, data):
    t = tokenize(data, "greedy", rng)
    return Stream().dynamic(*alphabets(rng, t, maxbits=15, deep=True, spare=12), t, final=True)


def enc_single_distance(rng, data):
    """matches of one distance symbol only: the distance set is a single 1-bit code"""
    t = tokenize(data, "dist1")
    ll, _ = alphabets(rng, t)
    return Stream().dynamic(ll, [1], t, final=True)


def enc_literal_only(rng, data):
    t = tokenize(data, "none")
    ll, _ = alphabets(rng, t)
    return Stream().dynamic(ll, [0], t, final=True)


def enc_far(rng, data):
    t = tokenize(data, "far")
    return Stream().dynamic(*alphabets(rng, t, spare=3), t, final=True)


def enc_many_blocks(rng, data):
    """up to 12 blocks of all three types with empty stored blocks between them"""
    s = Stream()
    parts = _split(rng, data, 2 + int(rng.integers(11)))
    for i, p in enumerate(parts):
        kind = int(rng.integers(4))
        if kind == 0:
            s.stored(p)
        elif kind == 1:
            s.fixed(tokenize(p, "none"))                   # a block's matches may not reach into a stored block's bytes here: the
        elif kind == 2:                                    # tokenizer sees one part at a time, which keeps every distance inside it
            t = tokenize(p, "greedy", rng)
            s.dynamic(*alphabets(rng, t), t)
        else:
            s.stored(b"").fixed(tokenize(p, "dist1"))
    return s.stored(b"", final=True)


ENCODERS = [enc_stored, enc_fixed, enc_dynamic_short, enc_dynamic_deep, enc_single_distance, enc_literal_only, enc_far, enc_many_blocks]


def encode_member(rng, data, k):
    """payload of `data` by encoder k; falls back to stored blocks when the crafted codes do not fit a 64-KiB member"""
    if len(data) == 0:
        return bytes([3, 0])
    payload, out = ENCODERS[k % len(ENCODERS)](rng, data).finish()
    assert out == data, ENCODERS[k % len(ENCODERS)].__name__
    if len(payload) + 26 > 65536:
        payload, out = Stream().stored(data[:len(data) // 2]).stored(data[len(data) // 2:], final=True).finish()
    return payload
