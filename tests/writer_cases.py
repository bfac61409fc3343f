"""Crafted inputs and plain references for the device track writer (tests/test_gpu_writer_edges.py, tests/test_deflate_host.py):
batches without fragments whose per-base values go in through DeviceBatch.set_track, built so that the text lands where the
kernels of csrc/natac_textz.hpp take their rare arms -- members that must be `stored`, member borders at chosen columns, texts of
chosen lengths -- and the values whose twelve-digit rounding sits on an edge of natac_text::round12.  Pure numpy / CPython: the
references here never call the library."""
import math
import string

import numpy as np

from nucleoatac_amd.packing import PackedChunks
from nucleoatac_amd.pyatac.tracks import _py2_float_str as f2s

BLK = 0xff00                      # input bytes per BGZF member
# characters no plain line ("1", digits, '.', tab, newline) and no value text ('e', '+', '-') contains
ODD_ALPHABET = [c for c in string.ascii_letters + "!$%&()*,/:;<=>?@[]^_{|}~" if c not in "e"]


def packed(starts, lens):
    """a batch of chunks without fragments or bias: all the writer needs"""
    n = len(lens)
    return PackedChunks(np.asarray(starts, np.int64), np.asarray(lens, np.int64), np.zeros(n + 1, np.int64), np.zeros(0, np.int32),
                        np.zeros(0, np.int32), None, None)


def line(name, a, b, v):
    return "%s\t%d\t%d\t%s\n" % (name, a, b, f2s(float(v)))


def plain_values(rng, n):
    """n distinct values in (0.1, 1) whose text is always 14 characters ("0." + twelve digits, the last one not 0)"""
    k = np.zeros(0, np.int64)
    while len(k) < n:
        d = rng.integers(0, 10, size=(n + 16, 12))
        d[:, 0] = np.maximum(d[:, 0], 1)
        d[:, 11] = np.maximum(d[:, 11], 1)
        k = np.unique(np.concatenate((k, d @ 10 ** np.arange(11, -1, -1, dtype=np.int64))))
    k = rng.permutation(k)[:n]
    vals = k / 1e12                                        # two exact operands: the double nearest to 0.dddddddddddd
    assert all(f2s(float(x)) == "0.%012d" % i for x, i in zip(vals[:20], k[:20]))
    return vals


def members(z):
    """(offset, size, first deflate byte, crc, isize) of every BGZF member of z"""
    import struct
    out, o = [], 0
    while o < len(z):
        assert z[o:o + 4] == b"\x1f\x8b\x08\x04" and z[o + 12:o + 16] == b"BC\x02\x00", o
        size = struct.unpack_from("<H", z, o + 16)[0] + 1
        crc, isz = struct.unpack_from("<II", z, o + size - 8)
        out.append((o, size, z[o + 18], crc, isz))
        o += size
    assert o == len(z)
    return out


# ---- B: members that must be stored ---------------------------------------------------------------------------------------
def stored_member_case(indexable=False, n_members=73, seed=3):
    """(PackedChunks, chroms, values): the text fills `n_members` members.  Members 0, 8, 16, ... -- the ones the Huffman code of a text
    of >= 64 members is built from (natac_deflate.hpp: sample_stride) -- hold plain lines "1\\t<pos>\\t<pos+1>\\t0.dddddddddddd\\n"
    (chunks with a distinct value per base), every other member one-line chunks (121 equal values) whose 64-character names are
    drawn from 256 names over characters the sample never sees and differ between consecutive chunks: the unseen literals get
    the longest codes, the Huffman payload passes 64 KiB and the member must be stored.
    indexable: a tabix index needs every chromosome's records in one contiguous stretch, so here every one-line chunk has a name
    of its own, every plain stretch its own number as a name, and only a few members (INDEXABLE_ODD) hold one-line chunks -- the
    index of tens of thousands of chromosomes is slow to build."""
    rng = np.random.default_rng(seed)
    table = ["".join(rng.choice(ODD_ALPHABET, size=64)) for _ in range(256)]
    assert len(set(table)) == 256
    chroms, starts, lens, vals = [], [], [], []
    n_text, coord, prev, stretch, was_odd = 0, 1000000, -1, 1, False
    target = n_members * BLK - BLK // 2
    while n_text < target:
        m = n_text // BLK
        odd_member = m in INDEXABLE_ODD if indexable else m % 8 != 0
        name = str(stretch) if indexable else "1"
        plain_len = len(name) + len(str(coord)) + len(str(coord + 1)) + 14 + 4
        n = 0 if odd_member else min(1500, ((m + 1) * BLK - n_text) // plain_len)
        if n > 0:                                          # plain chunk: ends before the member does
            assert len(str(coord + n)) == len(str(coord))
            v = plain_values(rng, n)
            n_text += n * plain_len
            was_odd = False
        else:                                              # one line with an odd name
            n = 121
            if indexable:
                name = "".join(rng.choice(ODD_ALPHABET, size=64))
                stretch += 0 if was_odd else 1
            else:
                j = int(rng.integers(0, 256))
                j = (j + 1) % 256 if j == prev else j
                name, prev = table[j], j
            x = float(rng.normal(0, 1) * 10.0 ** int(rng.integers(-30, 11)))
            v = np.full(n, x if x != 0 else 1.5)
            n_text += len(line(name, coord, coord + n, v[0]))
            was_odd = True
        chroms.append(name)
        starts.append(coord)
        lens.append(n)
        vals.append(v)
        coord += n
    if indexable:
        odd = [c for c in chroms if len(c) == 64]
        assert len(set(odd)) == len(odd)
    return packed(starts, lens), chroms, np.concatenate(vals)


INDEXABLE_ODD = (1, 2, 11, 36, 71)


# ---- C: borders and lengths -------------------------------------------------------------------------------------------------
def border_sweep_case(long_line, seed=11):
    """(PackedChunks, values, chroms_of, line_len, n_steps): a text a little over one member.  chroms_of(step) gives the chromosome names of
    step 0 .. n_steps - 1: only the names of the one-line chunks in front grow, one character per step, so the first member
    border (byte 0xff00) moves back through the line it cuts one column per step.  Every line around the border is `line_len`
    characters long: 33 (plain lines), or 96 with long_line (a 64-character name: the border passes the 64 columns matches are
    searched in)."""
    rng = np.random.default_rng(seed)
    lead = 2 if long_line else 1
    coord = 1000000
    starts, lens, vals, names = [], [], [], []
    n_text = 0
    for i in range(lead):                                  # one line each; its name is what the steps vary
        starts.append(coord); lens.append(121); vals.append(np.full(121, 0.5)); names.append(None)
        n_text += len(line("x", coord, coord + 121, 0.5))
        coord += 121
    plain_len = len(line("1", coord, coord + 1, 0.123456789012))
    long_name = "L" * 64
    long_len = len(line(long_name, coord, coord + 1, 0.123456789012))
    stop = BLK - 300 if long_line else BLK + 200
    n = (stop - n_text) // plain_len
    starts.append(coord); lens.append(n); vals.append(plain_values(rng, n)); names.append("1")
    n_text += n * plain_len
    coord += n
    if long_line:
        starts.append(coord); lens.append(6); vals.append(plain_values(rng, 6)); names.append(long_name)
        coord += 6
    # the tail: a zero, a run lost before a NaN, a NaN run -- the modes of the writer differ here, behind the border
    tail = np.concatenate((plain_values(rng, 3), [0.0, 0.0], plain_values(rng, 2), [0.25, 0.25, np.nan, np.nan], plain_values(rng, 110)))
    starts.append(coord); lens.append(len(tail)); vals.append(tail); names.append("2")
    n_steps = long_len if long_line else 64

    def chroms_of(step):
        grow = [1 + min(step, 63), 1 + max(0, step - 63)]
        return [("a" if i == 0 else "b") * grow[i] if nm is None else nm for i, nm in enumerate(names)]

    return packed(starts, lens), np.concatenate(vals), chroms_of, (long_len if long_line else plain_len), n_steps


def first_border_offset(text):
    """(offset of byte 0xff00 inside its line, length of that line)"""
    ls = text.rfind(b"\n", 0, BLK) + 1
    le = text.index(b"\n", BLK) + 1
    return BLK - ls, le - ls


def text_length_case(target, seed=5):
    """(PackedChunks, chroms, values) whose default-mode text is exactly `target` bytes: plain lines of 33 characters in ragged chunks, then
    one line whose name takes what is left"""
    rng = np.random.default_rng(seed)
    coord = 1000000
    plain_len = len(line("1", coord, coord + 1, 0.123456789012))
    fixed = len(line("", coord, coord + 121, 0.5))
    n = (target - fixed - 1) // plain_len
    while not 1 <= target - n * plain_len - fixed <= 64:
        n -= 1
    starts, lens, chroms, v = [], [], [], plain_values(rng, n)
    cuts = [0] + [c for c in (700, 1033, 1034, 2955) if c < n] + [n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        starts.append(coord + a); lens.append(b - a); chroms.append("1")
    starts.append(coord + n); lens.append(121); chroms.append("q" * (target - n * plain_len - fixed))
    return packed(starts, lens), chroms, np.concatenate((v, np.full(121, 0.5)))


# ---- A: what a reader of the file gets ------------------------------------------------------------------------------------
NAMED_TIES = (1234567890125.0, 875485468971500.0)         # exact ties beyond the exact range of the power-of-ten table


def exp12(v):
    """decimal exponent of v rounded to twelve significant digits (CPython's correctly rounded '%e')"""
    return int(("%.11e" % abs(v)).split("e")[1])


def is_hard(v):
    """the verdict natac_store_adopt must reach for a written value: not adoptable iff the twelve-digit decimal lies outside
    [1e-11, 1e34) -- its power of ten is then no exact double, one IEEE operation does not give the correctly rounded parse --
    or the value is one of the two named ties"""
    if v == 0 or v != v or math.isinf(v):
        return False
    return not -11 <= exp12(v) <= 33 or abs(v) in NAMED_TIES


def _tie_from_1e12(v):
    """exact: |v| >= 1e12 lies half way between two twelve-digit decimals (the device cannot decide those: `hard`)"""
    v = abs(v)
    if v < 1e12 or v != math.floor(v):
        return False
    n = int(v)
    d = len(str(n)) - 12
    return d >= 1 and n % 10 ** d == 5 * 10 ** (d - 1)


def exact_ties(rng, per_scale=200):
    """(values, twelfth digits): doubles exactly half way between two twelve-digit decimals below 1e12, v = (D + 1/2) / 10^s:
    representable iff 5^s divides 2 D + 1"""
    from fractions import Fraction
    vals, digs = [], []
    for s in range(0, 18):
        f = 5 ** s
        lo, hi = -(-(2 * 10 ** 11 + 1) // f), (2 * 10 ** 12 - 1) // f
        ks = set(int(k) | 1 for k in rng.integers(lo, hi + 1, size=per_scale)) | set(k for k in range(lo, min(hi, lo + 8) + 1) if k & 1)
        for k in sorted(ks):
            q = k * f
            if not 2 * 10 ** 11 < q < 2 * 10 ** 12:
                continue
            v = math.ldexp(k, -(s + 1))                    # q / (2 10^s) = k / 2^(s + 1), exact
            D = (q - 1) // 2
            assert Fraction(v) * 10 ** s == Fraction(2 * D + 1, 2)
            vals.append(v)
            digs.append(D % 10)
    return vals, digs


def in_range_values(seed=1):
    """about 190,000 doubles whose twelve-digit decimal exponent lies in [-11, 33]: the edges listed in the test's docstring"""
    rng = np.random.default_rng(seed)
    inf = math.inf
    out = [9.99999999999e33, 2.0 ** 53, 2.0 ** 53 - 1, 999999999999.5, 99999999999.95, 9.999999999995e-12]
    for j in range(-11, 34):
        for k in range(1, 10):
            x = float("%de%d" % (k, j))
            out += [x, math.nextafter(x, 0.0), math.nextafter(x, inf)]
        out += [float("9.999999999995e%d" % (j - 1)), float("9.99999999999e%d" % j), float("9.9999999999949e%d" % j)]
    ties, digs = exact_ties(rng)
    assert sum(d & 1 for d in digs) > 100 and sum(1 - (d & 1) for d in digs) > 100
    out += ties
    bits = rng.integers(1, 54, size=20000)
    out += [float(int(rng.integers(1 << (b - 1), 1 << b))) for b in bits]
    out += list(np.ldexp(1.0 + rng.random(75000), rng.integers(-37, 114, size=75000)))
    out = [v for v in out if -11 <= exp12(v) <= 33 and not _tie_from_1e12(v)]
    v = np.array(out)
    v = np.concatenate((v, -v))
    rng.shuffle(v)
    return v


def as_written_case(seed=2):
    """(PackedChunks, chroms, values, meta): in_range_values in ragged chunks, between them NaN runs of 1..60 bases (inside chunks, at
    chunk starts, at chunk ends, whole chunks), runs of equal values directly before a NaN, runs that mix +0.0 and -0.0, single
    zeros of either sign, +-inf"""
    rng = np.random.default_rng(seed)
    stream = in_range_values(seed + 1)
    nan = lambda n: np.full(n, np.nan)
    chunks, heads, tails = [], set(), set()
    i = 0
    while i < len(stream):
        k = len(chunks)
        if k % 10 == 9:
            chunks.append(nan(121 + k))                    # a whole chunk of NaN
            continue
        h, t = k % 61, (7 * k + 3) % 61
        heads.add(h); tails.add(t)
        body, want = [nan(h)], int(rng.integers(121, 3000))
        while sum(map(len, body)) < want and i < len(stream):
            n = int(rng.integers(1, 400))
            body.append(stream[i:i + n])
            i += n
            kind = int(rng.integers(0, 6))
            x = stream[int(rng.integers(0, len(stream)))]
            if kind == 0:
                body.append(nan(int(rng.integers(1, 61))))
            elif kind == 1:                                # a run of equal values directly before a NaN
                body += [np.full(int(rng.integers(2, 10)), x), nan(int(rng.integers(1, 61)))]
            elif kind == 2:                                # +0.0 and -0.0 compare equal: one run, written with its first sign
                body.append(np.where(rng.random(int(rng.integers(2, 9))) < 0.5, 0.0, -0.0))
            elif kind == 3:                                # a zero that starts a run of its own, either sign; sometimes before a NaN
                body.append(np.array([-0.0 if rng.random() < 0.5 else 0.0]))
                if rng.random() < 0.3:
                    body.append(nan(int(rng.integers(1, 5))))
            elif kind == 4:
                body.append(np.array([math.inf, x, -math.inf]))
            else:
                body.append(np.full(int(rng.integers(2, 6)), x))
        body.append(nan(t))
        chunks.append(np.concatenate(body))
    lens = [len(c) for c in chunks]
    starts = np.cumsum([5000] + [l + 77 for l in lens[:-1]])
    names = ["c", "chrA", "scaffold_" + "0123456789" * 4]
    chroms = [names[min(2, 3 * k // len(chunks))] for k in range(len(chunks))]
    return packed(starts, lens), chroms, np.concatenate(chunks), dict(heads=heads, tails=tails)


def text_round_trip(v):
    """float('%.12g' % x) of every value: CPython formats and parses correctly rounded"""
    return np.array([float("%.12g" % x) for x in v])


def as_written_expected(pk, v, rounded, write_zero, keep_runs_before_nan):
    """per base, what a reader of Track.write_track's file gets (pyatac/tracks.py:37-74, restated): a run = equal consecutive values of
    one chunk (NaNs together; +0.0 == -0.0); it is written with the text of its FIRST value unless it is NaN, is zero without
    write_zero, or is directly followed by a NaN (without keep_runs_before_nan); bases without a line read as NaN"""
    n = len(v)
    start = np.ones(n, bool)
    start[1:] = ~((v[1:] == v[:-1]) | (np.isnan(v[1:]) & np.isnan(v[:-1])))
    start[pk.out_off[:-1]] = True
    rs = np.flatnonzero(start)
    re = np.append(rs[1:], n)
    rv = v[rs]
    chunk_end = pk.out_off[np.searchsorted(pk.out_off, rs, "right")]
    nan_follows = (re < chunk_end) & np.isnan(v[np.minimum(re, n - 1)])
    emitted = ~np.isnan(rv) & ((rv != 0) | write_zero) & (keep_runs_before_nan | ~nan_follows)
    return np.repeat(np.where(emitted, rounded[rs], np.nan), re - rs)


def as_read_back(text, pk, chroms):
    """per-base values a reader of this bedGraph text gets (Track.read_track with empty = nan), every value parsed by float()"""
    out = np.full(int(pk.out_off[-1]), np.nan)
    toks = text.split()
    if not toks:
        return out
    name = np.array(toks[0::4])
    a = np.array(toks[1::4]).astype(np.int64)
    b = np.array(toks[2::4]).astype(np.int64)
    val = np.array([float(t) for t in toks[3::4]])
    chroms = np.array([c.encode() for c in chroms])
    seen = 0
    for c in np.unique(chroms):
        ck = np.flatnonzero(chroms == c)
        ck = ck[np.argsort(pk.chunk_start[ck])]
        m = name == c
        k = ck[np.searchsorted(pk.chunk_start[ck], a[m], "right") - 1]
        assert (a[m] >= pk.chunk_start[k]).all() and (b[m] <= pk.chunk_start[k] + pk.chunk_len[k]).all() and (b[m] > a[m]).all()
        ln = b[m] - a[m]
        first = pk.out_off[k] + a[m] - pk.chunk_start[k]
        idx = np.repeat(first - (np.cumsum(ln) - ln), ln) + np.arange(int(ln.sum()))
        out[idx] = np.repeat(val[m], ln)
        seen += int(m.sum())
    assert seen == len(name)
    return out


def same_bits(got, want):
    """bit-for-bit: -0.0 is not +0.0; a NaN must sit where a NaN is expected (its payload is not part of the contract)"""
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got[~gn].view(np.int64), want[~wn].view(np.int64)))
