"""CPU: the raw-deflate decoder of the device BAM path (natac_bam_dev.hpp: inflate_member, build_code, decode_symbol -- __host__ __device__,
here through natac_inflate_raw_host) against zlib.decompressobj(-15), an independent and complete inflater, on streams that no compressor
writes (tests/deflate_craft.py builds them from explicit instructions).

zlib ACCEPTS a payload s for a length isize iff decompressing s raises nothing, eof is true and the output has isize bytes.  The property:
natac_inflate_raw_host(s, isize) returns 0 iff zlib accepts, and then the bytes are equal.  The host BAM decoder inflates with zlib, so this
is also "the device path takes exactly the members the host path takes".

CASES is the named table (shared with tests/test_gpu_bam_device.py, which sends the identical bytes through the GPU kernel); the verdict of
every case is written down by hand, so a mistake of the builder cannot make both decoders agree by accident."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import deflate_craft as D
from deflate_craft import Stream

A = 97


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def noise(n, seed=1):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def fin(s, isize=None, cut=0, tail=b""):
    """(payload, isize, bytes the builder expects): cut drops bytes from the end of the payload, tail adds some"""
    payload, out = s.finish()
    payload = payload[:len(payload) - cut] + tail
    return payload, (len(out) if out is not None else 0) if isize is None else isize, out


def dyn(name, tokens, final=True, **kw):
    ll, dl = D.alphabets(rng_of(name), tokens, **kw)
    return Stream().dynamic(ll, dl, tokens, final=final)


LL_A = [0] * A + [2] + [0] * 158 + [2, 1]                 # 'a' and end-of-block: 2 bits, length symbol 257 (length 3): 1 bit -- complete
EOB1 = [0] * 256 + [1]                                     # the end-of-block code alone, one bit


def _stored_at_bit(k):
    s = Stream().fixed([200] * ((k + 6) % 8))              # 3 + 9 m + 7 bits: the next block starts k bits into a byte
    assert s.w.nbits() % 8 == k
    return fin(s.stored(b"xyz", final=True))


def _ends_on_bit7():
    s = Stream().fixed([200] * 6, final=True)              # 3 + 54 + 7 = 64 bits
    assert s.w.nbits() % 8 == 0
    return fin(s)


def _deep(which):
    name = "deep15_" + which
    if which == "literal":
        tokens = list(range(40))
        s = dyn(name, tokens, deep=True)
    else:
        tokens = [(3, b) for _, b, _ in D.DIST_SYMS[:18]]
        ll, dl = D.alphabets(rng_of(name), tokens, deep=True)
        assert max(dl) == 15
        s = Stream().stored(noise(600)).dynamic(ll, dl, tokens, final=True)
    return fin(s)


def _cl_7bit():
    ll = [1, 2, 3, 4, 5, 6, 7] + [0] * 249 + [7]           # complete; its lengths 0..7 are the eight symbols of a code-length code 1..7,7
    s = Stream().dynamic(ll, [0], list(range(7)), final=True, rle=D.rle_plain(ll + [0]), cl=[1, 2, 3, 4, 5, 6, 7, 7] + [0] * 11)
    return fin(s)


def _full_alphabets():
    r = rng_of("full")
    ll, dl = D.code_over(r, range(286)), D.code_over(r, range(30))
    assert len(ll) == 286 and len(dl) == 30
    toks = [int(x) for x in r.integers(0, 256, 300)] + [(258, 300), (3, 1), (100, 7)] + [(l, 200) for _, l, _ in D.LEN_SYMS]
    return fin(Stream().dynamic(ll, dl, toks, final=True))


def _hclen19():
    toks = list(range(40))
    ll, dl = D.alphabets(rng_of("hclen19"), toks, deep=True)
    assert ll.count(15) > 0                                # length 15 is the last of the 19 in transmission order
    return fin(Stream().dynamic(ll, dl, toks, final=True, rle=D.rle_plain(ll + dl)))


def _hclen(n):
    """lengths 0 and 8 only: 256 codes of 8 bits on symbols 1..256.  8 is the fifth entry in transmission order.  (With HCLEN = 4 only
    16, 17, 18 and 0 can be sent, every length is 0 and there is no end-of-block code: no dynamic block with HCLEN = 4 is valid, _hclen4.)"""
    ll = [0] + [8] * 256
    cl = [0] * 19
    cl[0], cl[8], cl[16] = 2, 2, 1
    return fin(Stream().dynamic(ll, [0], [1, 2, 255], final=True, cl=cl, hclen=n))


def _hclen4():
    cl = [0] * 19
    cl[0], cl[18] = 1, 1
    return fin(one().dynamic([0] * 257, [0], [("X", 0, 8)], final=True, rle=[(18, 138), (18, 120)], cl=cl, hclen=4, eob=False), isize=1)


def _repeat_cases(which):
    if which == "16_after_17_and_18":
        ll = [0] * A + [1] + [0] * 158 + [1]
        rle = [(18, 94), (16, 3), (1,), (17, 10), (16, 6), (18, 138), (16, 4), (1,), (0,)]
        return fin(Stream().dynamic(ll, [0], [A, A], final=True, rle=rle))
    if which == "16_across_the_border":                    # 16 with count 3 + 0: the last literal/length length and two distance lengths
        ll = LL_A + [0, 0]
        rle = D.rle_plain(ll[:259]) + [(16, 3), (1,)]
        return fin(Stream().dynamic(ll, [0, 0, 1], [A, A, A, (3, 3)], final=True, rle=rle))
    ll = [0] * A + [1] + [0] * 158 + [1] + [0] * 23        # 18 runs over 23 literal/length and 5 distance lengths
    rle = D.rle_plain(ll[:257]) + [(18, 28), (1,)]
    return fin(Stream().dynamic(ll, [0] * 5 + [1], [A], final=True, rle=rle))


def _mixed_blocks(n):
    r = rng_of("mixed%d" % n)
    s = Stream()
    for i in range(n):
        p = noise(int(r.integers(0, 40)), seed=i) + b"abcabcabcabc" * int(r.integers(0, 4))
        kind = (i + n) % 4
        if kind == 0:
            s.stored(p, final=i == n - 1)
        elif kind == 1:
            s.fixed(D.tokenize(p), final=i == n - 1)
        else:
            t = D.tokenize(p, "greedy" if kind == 2 else "none")
            s.dynamic(*D.alphabets(r, t), t, final=i == n - 1)
    return fin(s)


def _max_member_far():
    """65,536 bytes: 32,768 stored, then 127 copies of 258 bytes from 32,768 back and two literals"""
    h = noise(32768, 7)
    return fin(Stream().stored(h).fixed([(258, 32768)] * 127 + [1, 2], final=True))


def _truncated(bits_needed):
    """a fixed block of 9-bit literals cut one byte short: the decoder needs `bits_needed` (1..8) more bits than the payload holds"""
    m = (bits_needed + 6) % 8                              # 3 + 9 m + 7 = bits_needed mod 8
    s = Stream().fixed([200] * (m + 8), final=True)
    assert s.w.nbits() % 8 == bits_needed % 8
    return fin(s, isize=m + 8, cut=1)


def one():
    """a leading block of one literal: the invalid cases keep ISIZE > 0, since neither BAM decoder inflates a member whose ISIZE is 0"""
    return Stream().fixed([A])


def single(which, k, used=True):
    """the literal/length or the distance set is ONE code of k bits.  zlib's inflate_table takes an incomplete set only when its longest
    code has one bit"""
    if which == "lit":
        return fin(one().dynamic([0] * 256 + [k], [0], [], final=True), isize=1)
    s = Stream().dynamic(LL_A, [k], [A, (3, 1)] if used else [A], final=True)
    return fin(s, isize=4 if used else 1)


def hexcase(h, isize):
    return bytes.fromhex(h), isize, None


def _case_list():
    c = []
    ok = lambda name, fn: c.append((name, "ok", fn))
    bad = lambda name, fn: c.append((name, "bad", fn))
    # ---- valid ----------------------------------------------------------------------------------------------------------------------
    for s, b, e in D.LEN_SYMS:
        ok("length_sym_%d_least_extra_fixed" % s, lambda b=b: fin(Stream().fixed([A, (b, 1)], final=True)))
        ok("length_sym_%d_most_extra_dynamic" % s, lambda s=s, b=b, e=e: fin(dyn("len%d" % s, [A, 5, (b + (1 << e) - 1, 2, s)])))
    ok("length_258_as_symbol_285", lambda: fin(Stream().fixed([A, (258, 1, 285)], final=True)))
    ok("length_258_as_symbol_284_extra_31", lambda: fin(Stream().fixed([A, (258, 1, 284)], final=True)))
    for s, b, e in D.DIST_SYMS:
        ok("distance_sym_%d_least_extra_fixed" % s, lambda b=b: fin(Stream().stored(noise(b)).fixed([(3, b)], final=True)))
        ok("distance_sym_%d_most_extra_dynamic" % s,
           lambda s=s, b=b, e=e: fin(Stream().stored(noise(b + (1 << e) - 1)).dynamic(*D.alphabets(rng_of("d%d" % s), [(4, b + (1 << e) - 1)]),
                                                                                        [(4, b + (1 << e) - 1)], final=True)))
    ok("distance_32768_in_a_65536_byte_member", _max_member_far)
    for d in (1, 2, 3, 4, 5):
        for ln in (3, 4, 5, 7, 258):
            ok("copy_distance_%d_length_%d" % (d, ln), lambda d=d, ln=ln: fin(Stream().fixed(list(b"abcde") + [(ln, d)], final=True)))
    ok("literal_codes_of_15_bits", lambda: _deep("literal"))
    ok("distance_codes_of_15_bits", lambda: _deep("distance"))
    ok("code_length_codes_of_7_bits", _cl_7bit)
    ok("only_the_end_of_block_code_1_bit", lambda: single("lit", 1))
    ok("one_distance_code_of_1_bit", lambda: single("dist", 1))
    ok("one_distance_code_of_1_bit_unused", lambda: single("dist", 1, used=False))
    ok("one_distance_code_of_1_bit_hand_written", lambda: hexcase("0dc0010900000080a0adfe3f516201", 6))
    ok("one_distance_code_on_symbol_3", lambda: fin(Stream().dynamic(LL_A, [0, 0, 0, 1], list(b"aaaa") + [(3, 4)], final=True)))
    ok("no_distance_code_literal_only_body", lambda: fin(Stream().dynamic(LL_A, [0], [A, A, A], final=True)))
    ok("hlit_286_hdist_30_in_full", _full_alphabets)
    ok("hclen_19", _hclen19)
    ok("hclen_5_the_least_that_can_be_valid", lambda: _hclen(5))
    ok("repeat_16_after_17_and_after_18", lambda: _repeat_cases("16_after_17_and_18"))
    ok("repeat_16_across_the_literal_distance_border", lambda: _repeat_cases("16_across_the_border"))
    ok("repeat_18_across_the_literal_distance_border", lambda: _repeat_cases("18_across_the_border"))
    ok("empty_stored_block_first", lambda: fin(Stream().stored(b"").fixed([A, A], final=True)))
    ok("empty_stored_block_between_huffman_blocks", lambda: fin(dyn("esb", [A, (5, 1)], final=False).stored(b"").fixed([(4, 2)], final=True)))
    ok("empty_stored_block_last", lambda: fin(Stream().fixed([A, A]).stored(b"", final=True)))
    for k in range(8):
        ok("stored_block_begins_%d_bits_into_a_byte" % k, lambda k=k: _stored_at_bit(k))
    for n in (1, 2, 40):
        ok("%d_blocks_of_mixed_types" % n, lambda n=n: _mixed_blocks(n))
    ok("final_block_ends_on_bit_7_of_the_last_byte", _ends_on_bit7)
    ok("bytes_behind_the_final_block_are_not_looked_at", lambda: fin(Stream().fixed([A], final=True), tail=b"\xff\x00\xa5" * 5))
    ok("isize_0_stored", lambda: fin(Stream().stored(b"", final=True)))
    ok("isize_0_fixed", lambda: fin(Stream().fixed([], final=True)))
    ok("isize_1", lambda: fin(Stream().fixed([0], final=True)))
    ok("isize_65280_one_stored_block", lambda: fin(Stream().stored(noise(65280, 3), final=True)))
    ok("isize_65536_two_stored_blocks", lambda: fin(Stream().stored(noise(65535, 4)).stored(b"!", final=True)))
    ok("isize_65536_distance_1_copies", lambda: fin(Stream().fixed([0] + [(258, 1)] * 254 + [(3, 1)], final=True)))
    # ---- invalid: one per return code of inflate_member and per rule inside it -----------------------------------------------------------
    def type3():
        s = one()
        s.header(True, 3)
        return fin(s, isize=1)
    bad("block_type_3", type3)
    bad("stored_len_nlen_mismatch", lambda: fin(Stream().stored(b"abc", final=True, nlen=0x1234), isize=3))
    bad("stored_len_past_the_payload", lambda: fin(Stream().stored(b"abc", final=True, length=10), isize=10))
    bad("stored_len_past_isize", lambda: fin(Stream().stored(b"abcdef", final=True), isize=5))
    bad("hlit_287", lambda: fin(Stream().dynamic(LL_A + [0] * 29, [1], [A], final=True), isize=1))
    bad("hlit_288", lambda: fin(Stream().dynamic(LL_A + [0] * 30, [1], [A], final=True), isize=1))
    bad("hdist_31", lambda: fin(Stream().dynamic(LL_A, [1] + [0] * 30, [A], final=True), isize=1))
    bad("hdist_32", lambda: fin(Stream().dynamic(LL_A, [1] + [0] * 31, [A], final=True), isize=1))
    cl3 = lambda a, b, c_: [a, b, c_] + [0] * 16
    bad("code_length_code_over_subscribed", lambda: fin(one().dynamic(EOB1, [0], [], final=True, rle=D.rle_plain(EOB1 + [0]), cl=cl3(1, 1, 1)), isize=1))
    bad("code_length_code_incomplete", lambda: fin(one().dynamic(EOB1, [0], [], final=True, rle=D.rle_plain(EOB1 + [0]), cl=cl3(1, 2, 0)), isize=1))
    bad("code_length_code_single_code", lambda: fin(one().dynamic([0] * 257, [0], [("X", 0, 1)], final=True, rle=D.rle_plain([0] * 258), cl=cl3(1, 0, 0), eob=False), isize=1))
    bad("code_length_code_empty", lambda: fin(one().dynamic([0] * 257, [0], [("X", 0, 16)], final=True, rle=[], cl=[0] * 19, hclen=4, eob=False), isize=1))
    bad("hclen_4_cannot_be_valid", _hclen4)
    bad("repeat_16_as_the_first_length_symbol", lambda: fin(one().dynamic(EOB1, [0], [], final=True, rle=[(16, 3)] + D.rle_plain(EOB1[3:] + [0])), isize=1))
    bad("repeat_runs_past_hlit_plus_hdist", lambda: fin(one().dynamic(EOB1, [0], [], final=True, rle=D.rle_plain(EOB1) + [(18, 11)]), isize=1))
    bad("repeat_16_runs_past_hlit_plus_hdist", lambda: fin(Stream().dynamic(LL_A, [1], [A], final=True, rle=D.rle_plain(LL_A) + [(16, 3)]), isize=1))
    bad("no_end_of_block_code", lambda: fin(Stream().dynamic([1, 1] + [0] * 255, [0], [0, 1], final=True, eob=False), isize=2))
    bad("literal_set_over_subscribed", lambda: fin(Stream().dynamic([1, 1] + [0] * 254 + [1], [0], [0], final=True), isize=1))
    bad("literal_set_incomplete_two_codes", lambda: fin(Stream().dynamic([0] * A + [2] + [0] * 158 + [2], [0], [A], final=True), isize=1))
    bad("literal_set_incomplete_three_codes", lambda: fin(Stream().dynamic([0] * A + [1] + [0] * 158 + [3, 3], [0], [A], final=True), isize=1))
    bad("distance_set_over_subscribed", lambda: fin(Stream().dynamic(LL_A, [1, 1, 1], [A, (3, 1)], final=True), isize=4))
    bad("distance_set_incomplete_two_codes", lambda: fin(Stream().dynamic(LL_A, [2, 2], [A, (3, 1)], final=True), isize=4))
    for k in range(2, 16):
        bad("only_the_end_of_block_code_%d_bits" % k, lambda k=k: single("lit", k))
        bad("one_distance_code_of_%d_bits" % k, lambda k=k: single("dist", k))
    bad("one_distance_code_of_2_bits_unused", lambda: single("dist", 2, used=False))
    bad("one_distance_code_of_2_bits_hand_written", lambda: hexcase("0dc0010900000080a0adfe3f516102", 6))
    bad("only_the_end_of_block_code_1_bit_then_the_other_bit", lambda: fin(one().dynamic(EOB1, [0], [("X", 1, 1)], final=True), isize=1))
    bad("one_distance_code_of_1_bit_then_the_other_bit", lambda: fin(Stream().dynamic(LL_A, [1], [A, ("L", 257), ("X", 1, 1)], final=True), isize=4))
    bad("fixed_block_symbol_286", lambda: fin(Stream().fixed([A, ("L", 286), ("D", 0)], final=True), isize=4))
    bad("fixed_block_symbol_287", lambda: fin(Stream().fixed([A, ("L", 287), ("D", 0)], final=True), isize=4))
    bad("fixed_block_distance_symbol_30", lambda: fin(Stream().fixed([A, ("L", 257), ("D", 30)], final=True), isize=4))
    bad("fixed_block_distance_symbol_31", lambda: fin(Stream().fixed([A, ("L", 257), ("D", 31)], final=True), isize=4))
    bad("length_code_when_no_distance_code_exists", lambda: fin(Stream().dynamic(LL_A, [0], [A, ("L", 257), ("X", 0, 1)], final=True), isize=4))
    bad("distance_one_past_the_start_of_the_output", lambda: fin(Stream().fixed([A, (3, 2)], final=True), isize=4))
    bad("distance_one_past_the_start_after_a_stored_block", lambda: fin(Stream().stored(b"abc").fixed([(3, 4)], final=True), isize=6))
    bad("output_one_byte_longer_than_isize", lambda: fin(Stream().fixed([A, (5, 1)], final=True), isize=5))
    bad("output_one_byte_longer_than_isize_literal", lambda: fin(Stream().fixed([A, A], final=True), isize=1))
    bad("output_one_byte_shorter_than_isize", lambda: fin(Stream().fixed([A, (5, 1)], final=True), isize=7))
    bad("stream_needs_1_bit_more", lambda: _truncated(1))
    bad("stream_needs_1_byte_more", lambda: _truncated(8))
    bad("stream_needs_9_bytes_more", lambda: fin(Stream().fixed([200] * 20, final=True), isize=20, cut=9))
    bad("stream_ends_inside_a_dynamic_header", lambda: (_full_alphabets()[0][:20], 500, None))
    bad("stream_ends_inside_a_stored_header", lambda: fin(Stream().fixed([A]).stored(b"abc", final=True), isize=4, cut=5))
    bad("empty_payload", lambda: (b"", 0, None))
    bad("no_final_block", lambda: fin(Stream().fixed([A, A]), isize=2))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, "ok" | "bad", payload, isize, expected bytes or None)]"""
    out = []
    for name, verdict, fn in _case_list():
        payload, isize, exp = fn()
        out.append((name, verdict, payload, isize, exp))
    assert len({c[0] for c in out}) == len(out)
    return out


CASE_NAMES = [c[0] for c in _case_list()]


def zlib_accepts(s, isize):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(s, isize + 1)          # one byte more than wanted is enough to see a stream that runs long
    except zlib.error:
        return False, b""
    return d.eof and len(out) == isize, out


@functools.lru_cache(maxsize=None)
def _lib():
    from nucleoatac_amd import _lib as L
    return L.load()


def inflate(s, isize):
    out = C.create_string_buffer(max(1, isize))
    return _lib().natac_inflate_raw_host(s, len(s), out, isize), out.raw[:isize]


def conforms(s, isize, what=""):
    """the property; returns zlib's verdict"""
    rc, got = inflate(s, isize)
    acc, ref = zlib_accepts(s, isize)
    assert (rc == 0) == acc, "%s: inflate_member returns %d, zlib %s (%d payload bytes, isize %d)" % (what, rc, "accepts" if acc else "rejects", len(s), isize)
    if acc:
        assert got == ref, "%s: accepted by both, bytes differ" % what
    return acc


@pytest.mark.parametrize("name", CASE_NAMES)
def test_named_case(name):
    _, verdict, payload, isize, exp = next(c for c in cases() if c[0] == name)
    acc, ref = zlib_accepts(payload, isize)
    assert acc == (verdict == "ok"), "the table says %s, zlib says otherwise: the case is not what its name says" % verdict
    if verdict == "ok" and exp is not None:
        assert ref == exp and len(exp) == isize, "the builder's own bytes differ from zlib's"
    assert conforms(payload, isize, name) == acc


def test_the_table_is_what_it_claims():
    """properties the names promise that no verdict shows: code lengths really reach 15 bits, members really reach 65,536 bytes, and
    the two hand-written streams differ in the one length"""
    by = {c[0]: c for c in cases()}
    assert by["isize_65536_two_stored_blocks"][3] == 65536 and by["distance_32768_in_a_65536_byte_member"][3] == 65536
    assert by["isize_65280_one_stored_block"][3] == 65280 and by["isize_0_fixed"][3] == 0 and by["isize_1"][3] == 1
    a, b = by["one_distance_code_of_1_bit_hand_written"][2], by["one_distance_code_of_2_bits_hand_written"][2]
    assert len(a) == len(b) == 15 and sum(x != y for x, y in zip(a, b)) == 2
    assert sum(1 for c in cases() if c[1] == "ok") >= 130 and sum(1 for c in cases() if c[1] == "bad") >= 70


# ---- seeded random sweep ----------------------------------------------------------------------------------------------------------------------
def random_data(rng, n):
    kind = int(rng.integers(5))
    if kind == 0:
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))
    if kind == 1:
        return bytes(rng.integers(0, 4, n, dtype=np.uint8))
    if kind == 2:
        return (b"chr1\t12345\t12346\t0.123456789012\n" * (n // 30 + 1))[:n]
    if kind == 3:
        return bytes(n)
    return bytes(np.repeat(rng.integers(0, 256, n, dtype=np.uint8), rng.integers(1, 14, n))[:n].tolist())        # runs of 1..13 equal bytes


SWEEP_SEED = 20240611
SWEEP_ROUNDS = 160
# what zlib alone says about the mutants of this seed and this many rounds (measured on the CPU: 2,780 accepted, 35,308 rejected);
# the floors leave a quarter of headroom, so the sweep cannot pass by producing nothing of one kind
SWEEP_MIN_ACCEPTED = 2000
SWEEP_MIN_REJECTED = 26000


def test_random_streams_and_their_mutants():
    rng = np.random.default_rng(SWEEP_SEED)
    accepted = rejected = 0
    for r in range(SWEEP_ROUNDS):
        n = int(rng.choice([0, 1, 2, 3, 17, 300, 3000, int(rng.integers(0, 3000)), int(rng.integers(0, 20000))]))
        if r % 40 == 39:
            n = int(rng.choice([65280, 65535, 65536]))
        data = random_data(rng, n)
        k = int(rng.integers(len(D.ENCODERS)))
        s = D.ENCODERS[k](rng, data) if n else Stream().fixed([], final=True)
        payload, out = s.finish()
        what = "round %d (%s, %d bytes)" % (r, D.ENCODERS[k].__name__, n)
        assert out == data, what
        assert conforms(payload, n, what), what + ": a valid stream"
        # every bit of every block header (a sample of 96 when the member is large), a sample of all bits, truncations, wrong lengths
        hdr = [b for a, e in s.headers for b in range(a, e)]
        if len(hdr) > 96 and n > 4000:
            hdr = [hdr[i] for i in sorted(rng.choice(len(hdr), 96, replace=False))]
        nb = 8 * len(payload)
        body = [int(b) for b in rng.integers(0, nb, 48 if n <= 4000 else 12)]
        for b in hdr + body:
            g = bytearray(payload)
            g[b >> 3] ^= 1 << (b & 7)
            if conforms(bytes(g), n, what + " bit %d flipped" % b):
                accepted += 1
            else:
                rejected += 1
        for cut in sorted({1, 2, 9, len(payload) // 2, int(rng.integers(1, len(payload) + 1))}):
            if cut <= len(payload):
                assert not conforms(payload[:len(payload) - cut], n, what + " cut by %d" % cut)
                rejected += 1
        for isz in (n - 1, n + 1):
            if isz >= 0:
                assert not conforms(payload, isz, what + " isize %d" % isz)
    print("sweep: %d accepted, %d rejected mutants" % (accepted, rejected))
    assert accepted >= SWEEP_MIN_ACCEPTED and rejected >= SWEEP_MIN_REJECTED, (accepted, rejected)
