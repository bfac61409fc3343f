"""BAM -> fragment arrays on the device (csrc/natac_bam_dev.hpp: one lane inflates one BGZF member, one lane walks the records
of one member, the host confirms the chain of record starts) against the host decoder (natac_bam.hpp, itself checked against
an independent Python decoder in tests/test_bam.py): the same per-reference arrays for members of every size, windows small
enough that records and the header straddle them, every deflate block type, and the same errors for damaged files."""
import os
import struct
import zlib

import numpy as np
import pytest

from nucleoatac_amd.pyatac.fragments import FragmentStore

pytestmark = pytest.mark.gpu


def _bgzf(data, blk, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    out = bytearray()
    for o in range(0, len(data), blk):
        chunk = data[o:o + blk]
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        comp = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(comp) + 8 - 1)
        out += comp + struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk))
    out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    return bytes(out)


def _random_bam_bytes(rng, n, n_refs=5, long_header=False):
    """uncompressed BAM: records with names, cigars, sequences and aux data of every length, mapped / unmapped, every flag mix"""
    text = b"@HD\tVN:1.0\tSO:coordinate\n"
    if long_header:              # ~300 kB that do not compress
        text += b"@CO\t" + bytes(rng.integers(48, 123, 300000, dtype=np.uint8)) + b"\n"
    parts = [b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_refs)]
    for r in range(n_refs):
        nm = ("chr%d_%s" % (r, "y" * r)).encode() + b"\0"
        parts.append(struct.pack("<i", len(nm)) + nm + struct.pack("<i", 1 << 28))
    ref = np.sort(rng.integers(0, n_refs, n))
    ref[n - n // 50:] = -1                                   # unmapped reads at the end, like a sorted file
    pos = rng.integers(0, 1 << 27, n)
    order = np.lexsort((pos, np.where(ref < 0, n_refs, ref)))
    ref, pos = ref[order], pos[order]
    flags = rng.choice([99, 147, 83, 163, 4, 77, 141, 0, 1, 3, 1187, 2115], n)
    for i in range(n):
        ln, nc, ls, aux = int(rng.integers(2, 40)), int(rng.integers(0, 6)), int(rng.integers(0, 200)), int(rng.integers(0, 50))
        name = bytes(rng.integers(33, 127, ln - 1, dtype=np.uint8)) + b"\0"
        body = name + bytes(rng.integers(0, 256, 4 * nc + (ls + 1) // 2 + ls + aux, dtype=np.uint8))
        tlen = int(rng.integers(-700, 700))
        rec = struct.pack("<iiBBHHHiiii", int(ref[i]), int(pos[i]) if ref[i] >= 0 else -1, ln, 30, 4680, nc, int(flags[i]), ls,
                          int(ref[i]), int(pos[i]) + 40 if ref[i] >= 0 else -1, tlen) + body
        parts.append(struct.pack("<i", len(rec)) + rec)
    return b"".join(parts)


def _same(a, b):
    assert a.references == b.references and list(a.lengths) == list(b.lengths)
    for c in a.references:
        assert np.array_equal(a.pos[c], b.pos[c]) and np.array_equal(a.tlen[c], b.tlen[c]), c


@pytest.mark.parametrize("blk,level,window", [(300, 6, 0), (3000, 1, 0), (65280, 6, 0), (65280, 9, 40000), (5000, 0, 0), (777, 6, 2500),
                                              (65536, 6, 0), (1200, 6, 70000)])
def test_device_decoder_equals_host_decoder(tmp_path, monkeypatch, blk, level, window):
    rng = np.random.default_rng(blk + level)
    raw = _random_bam_bytes(rng, 6000, long_header=(blk == 1200))
    path = str(tmp_path / "a.bam")
    strategy = zlib.Z_FIXED if blk == 777 else zlib.Z_DEFAULT_STRATEGY
    open(path, "wb").write(_bgzf(raw, blk, level, strategy))
    if window:
        monkeypatch.setenv("NATAC_BAM_DEV_WINDOW", str(window))
    host = FragmentStore.from_bam(path, device=False)
    dev = FragmentStore.from_bam(path, device=True)
    if blk == 1200:
        # a header that does not fit the (70,000 + 65,536)-byte window: the device path hands the file to the host decoder
        assert FragmentStore.last_bam_on_device is False
    else:
        assert FragmentStore.last_bam_on_device is True
    _same(host, dev)
    assert sum(len(host.pos[c]) for c in host.references) > 1000


def test_device_decoder_large_file_and_damage(tmp_path):
    """400,000 records through 64-KiB members (several thousand lanes), then the same file truncated / garbled: the device path
    reports what the host decoder reports"""
    from helpers import write_bam
    rng = np.random.default_rng(5)
    n = 400000
    ref = np.sort(rng.integers(0, 3, n))
    pos = rng.integers(0, 5_000_000, n)
    order = np.lexsort((pos, ref))
    flag = rng.choice([99, 147, 83, 163], n)
    tl = rng.integers(30, 900, n) * np.where(flag & 0x10, -1, 1)
    path = str(tmp_path / "big.bam")
    write_bam(path, [("chrI", 6_000_000), ("chrII", 6_000_000), ("chrIII", 6_000_000)],
              zip(ref[order].tolist(), pos[order].tolist(), flag.tolist(), tl.tolist()), blk=65280)
    host = FragmentStore.from_bam(path, device=False)
    dev = FragmentStore.from_bam(path, device=True)
    assert FragmentStore.last_bam_on_device is True
    _same(host, dev)
    assert sum(len(dev.pos[c]) for c in dev.references) == int(((flag & 2) > 0).sum() - ((flag & 0x12) == 0x12).sum())
    b = open(path, "rb").read()
    cut = str(tmp_path / "cut.bam")
    open(cut, "wb").write(b[:len(b) // 2])
    with pytest.raises(Exception, match="truncated|trailing"):
        FragmentStore.from_bam(cut, device=True)
    g = bytearray(b)
    g[len(g) // 3] ^= 0x55
    g[len(g) // 3 + 1] ^= 0xaa
    bad = str(tmp_path / "bad.bam")
    open(bad, "wb").write(bytes(g))
    for device in (False, True):       # a damaged deflate stream either fails to inflate or fails its member's CRC-32
        with pytest.raises(Exception, match="inflate|BGZF|truncated"):
            FragmentStore.from_bam(bad, device=device)


def test_payload_damage_that_still_inflates_fails_the_crc(tmp_path):
    """members written with stored deflate blocks: a flipped bit in the data bytes inflates without complaint to the right length --
    only the member's CRC-32 (which htslib verifies behind every read of the reference, pyatac/fragments.pyx:21) can tell; both
    decoders name the member's file offset"""
    rng = np.random.default_rng(17)
    raw = _random_bam_bytes(rng, 3000)
    blk = 5000
    good = _bgzf(raw, blk, 0)                                   # level 0: one stored block per member
    path = str(tmp_path / "stored.bam")
    open(path, "wb").write(good)
    _same(FragmentStore.from_bam(path, device=False), FragmentStore.from_bam(path, device=True))
    # member k starts at k * (18 + 5 + blk + 8); its data bytes follow the 5-byte stored-block header
    per = 18 + 5 + blk + 8
    for k, byte in ((0, 40), (3, 4999), (len(raw) // blk - 1, 123)):
        g = bytearray(good)
        g[k * per + 18 + 5 + byte] ^= 0x04
        bad = str(tmp_path / ("flip%d.bam" % k))
        open(bad, "wb").write(bytes(g))
        for device in (False, True):
            with pytest.raises(Exception, match=r"CRC-32 mismatch in the BGZF member at file offset %d " % (k * per)):
                FragmentStore.from_bam(bad, device=device)
    # a damaged CRC field itself
    g = bytearray(good)
    g[2 * per + 18 + 5 + blk] ^= 0x80
    bad = str(tmp_path / "crcfield.bam")
    open(bad, "wb").write(bytes(g))
    for device in (False, True):
        with pytest.raises(Exception, match=r"CRC-32 mismatch in the BGZF member at file offset %d " % (2 * per)):
            FragmentStore.from_bam(bad, device=device)


# ---- crafted deflate streams (tests/deflate_craft.py) and decoy records ----------------------------------------------------------------------
# The members above come from zlib's compressor and their records' bodies are random bytes.  Below, the deflate streams are written
# bit by bit (15-bit codes, single-code sets, far and distance-1 copies, empty blocks: what htslib / libdeflate may write and zlib never
# does), the invalid ones are the very bytes tests/test_inflate_conformance.py has checked on the CPU, and records carry believable false
# record chains where a member starts.  Every test asserts last_bam_on_device: a silent hand-over to the host decoder cannot pass.
import functools                                            # noqa: E402

import deflate_craft as D                                   # noqa: E402
from test_inflate_conformance import cases                  # noqa: E402


def _header(n_refs):
    text = b"@HD\tVN:1.0\tSO:unsorted\n"
    parts = [b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", n_refs)]
    for r in range(n_refs):
        nm = ("chr%d" % r).encode() + b"\0"
        parts.append(struct.pack("<i", len(nm)) + nm + struct.pack("<i", 1 << 28))
    return b"".join(parts)


def _rec(ref, pos, flag, tlen, name=b"r\0", ncig=0, lseq=0, aux=b""):
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name), 30, 4680, ncig, flag, lseq, ref, pos + 40 if ref >= 0 else -1, tlen)
    body += name + bytes(4 * ncig + (lseq + 1) // 2 + lseq) + aux
    return struct.pack("<i", len(body)) + body


def _random_rec(rng, n_refs, aux=b""):
    ref = int(rng.integers(0, n_refs)) if n_refs and rng.integers(8) else -1
    flag = int(rng.choice([99, 147, 83, 163, 1187])) if ref >= 0 else int(rng.choice([4, 77, 141]))
    name = bytes(rng.integers(33, 127, int(rng.integers(0, 20)), dtype=np.uint8)) + b"\0"
    return _rec(ref, int(rng.integers(0, 1 << 27)) if ref >= 0 else -1, flag, int(rng.integers(-700, 700)), name, int(rng.integers(0, 4)),
                int(rng.integers(0, 60)), aux)


def _file(raw, cuts, encode=None):
    """BGZF file of `raw` with a member border at every cut (spans over 60,000 bytes are cut further); encode(k, chunk) -> deflate payload
    (default: zlib level 1), or a whole member"""
    out, k = bytearray(), 0
    edges = sorted({0, len(raw)} | {c for c in cuts if 0 < c < len(raw)})
    for a, b in zip(edges, edges[1:]):
        for o in range(a, b, 60000):
            chunk = raw[o:min(b, o + 60000)]
            if encode is None:
                co = zlib.compressobj(1, zlib.DEFLATED, -15)
                m = co.compress(chunk) + co.flush()
            else:
                m = encode(k, chunk)
            out += m if m[:2] == b"\x1f\x8b" else D.bgzf_member(m, chunk)
            k += 1
    return bytes(out + D.BGZF_EOF)


def _same_as_python(dev, path):
    py = FragmentStore.from_bam_python(path)                 # keeps TLEN's sign; the native decoders store |TLEN|
    assert dev.references == py.references
    for c in dev.references:
        assert np.array_equal(dev.pos[c], py.pos[c]) and np.array_equal(dev.tlen[c], np.abs(py.tlen[c])), c


def _both(path, on_device=True, python=True):
    host = FragmentStore.from_bam(path, device=False)
    dev = FragmentStore.from_bam(path, device=True)
    assert FragmentStore.last_bam_on_device is on_device
    _same(host, dev)
    if python:
        _same_as_python(dev, path)
    return dev


def _both_raise(path, match):
    for device in (False, True):
        with pytest.raises(Exception, match=match):
            FragmentStore.from_bam(path, device=device)


def _extreme_bam_bytes(rng, n):
    """_random_bam_bytes plus records of the 37-byte minimum (l_read_name 1, nothing else), with 65,535 CIGAR operations, and with several
    hundred kilobytes of auxiliary data (low-entropy, so that 65,536-byte members of it fit a BGZF member under every encoder)"""
    parts = [_header(4)]
    for i in range(n):
        kind = int(rng.integers(60))
        if kind == 0:
            parts.append(_rec(int(rng.integers(0, 4)), 5, 99, 300, b"\0"))
            assert len(parts[-1]) == 37
        elif kind == 1 and i % 8 == 0:
            parts.append(_random_rec(rng, 4, bytes(rng.integers(0, 3, int(rng.integers(70000, 400000)), dtype=np.uint8))))
        elif kind == 2 and i % 3 == 0:
            parts.append(_rec(1, 7, 99, -250, b"c\0", ncig=65535, lseq=3))
        else:
            parts.append(_random_rec(rng, 4, bytes(rng.integers(0, 256, int(rng.integers(0, 50)), dtype=np.uint8))))
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def _heterogeneous_file():
    """member k is written by encoder k mod 8 of the builder (stored, fixed, dynamic with short codes, with 15-bit codes, a single
    distance code, literals only, far matches, many small blocks), sizes run from 1 byte to 65,536 with empty members between, the
    BGZF headers vary: neighbouring lanes hold Huffman tables of different shapes in their LDS columns and sit in different branches of
    the decoder.  A lane that leaves its column, or state kept from the member it inflated before, changes bytes: the member's CRC-32
    or the arrays tell."""
    rng = np.random.default_rng(77)
    raw = _extreme_bam_bytes(rng, 2000)
    sizes = [1, 2, 3, 37, 64, 300, 700, 1500, 4000, 65536, 0, 9, 20000, 100, 65280, 511, 5, 2000, 33000, 0, 257, 258, 259, 1024]
    cuts, o, i = [], 0, 0
    plan = []
    while o < len(raw):
        want = sizes[(i // 3) % len(sizes)] if i % 3 == 0 else int(rng.integers(1, 1200))
        plan.append(want)
        o += want
        cuts.append(o)
        i += 1
    hdr = [dict(), dict(mtime=1718000000, xfl=2, os_=3), dict(pre=[(b"AB", b"xyz")]), dict(post=[(b"RA", bytes(40))]),
           dict(pre=[(b"BC", b"three")], post=[(b"ZZ", b"")], xfl=4, os_=0)]            # a BC subfield that is not 2 bytes long is not THE BC
    out, o, k, empties = bytearray(), 0, 0, 0
    for want in plan:
        chunk = raw[o:o + want]
        if want == 0:
            out += D.bgzf_member(bytes([3, 0]), b"", **hdr[k % 5])
            empties += 1
            continue
        payload = D.encode_member(rng, chunk, k)
        if len(payload) + 100 > 65536:                       # random record bodies under a crafted code can outgrow a member: two halves
            for half in (chunk[:len(chunk) // 2], chunk[len(chunk) // 2:]):
                out += D.bgzf_member(D.encode_member(rng, half, 0), half, **hdr[k % 5])
        else:
            out += D.bgzf_member(payload, chunk, **hdr[k % 5])
        o += want
        k += 1
    assert k > 1000 and empties > 20, (k, empties, len(raw))
    return bytes(out) + D.BGZF_EOF


@pytest.mark.parametrize("window", [0, 50000])
def test_heterogeneous_workgroups(tmp_path, monkeypatch, window):
    """the file above in one window (one launch, every workgroup mixed) and in windows of 50,000 bytes (many launches, lanes take several
    members from the queue)"""
    path = str(tmp_path / "het.bam")
    open(path, "wb").write(_heterogeneous_file())
    if window:
        monkeypatch.setenv("NATAC_BAM_DEV_WINDOW", str(window))
    dev = _both(path)
    assert sum(len(dev.pos[c]) for c in dev.references) > 500


def test_named_valid_streams_through_the_device(tmp_path):
    """every valid case of the conformance table as a member of its own: the bytes it inflates to are the auxiliary data of a record, the
    member borders lie at the ends of that data, and the member's payload is the case's stream, bit for bit"""
    rng = np.random.default_rng(3)
    parts, cuts, payloads, off = [_header(3)], [], {}, 0
    off = len(parts[0])
    n_ok = 0
    for name, verdict, payload, isize, exp in cases():
        if verdict != "ok" or not isize or isize > 60000:       # (_file cuts longer spans; the 64-KiB cases go through the test above)
            continue
        if exp is None:
            exp = zlib.decompressobj(-15).decompress(payload)
        rec = _random_rec(rng, 3, exp)
        a = off + len(rec) - len(exp)
        cuts += [a, off + len(rec)]
        payloads.setdefault(bytes(exp), []).append(payload)       # several cases inflate to the same bytes: in file order
        parts.append(rec)
        off += len(rec)
        for _ in range(int(rng.integers(0, 3))):
            parts.append(_random_rec(rng, 3))
            off += len(parts[-1])
        n_ok += 1
    raw = b"".join(parts)
    used = []

    def encode(k, chunk):
        p = payloads.get(bytes(chunk))
        if not p:
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            return co.compress(chunk) + co.flush()
        used.append(k)
        return p.pop(0)
    path = str(tmp_path / "named.bam")
    open(path, "wb").write(_file(raw, cuts, encode))
    assert n_ok > 150 and len(used) == n_ok, (n_ok, len(used))
    _both(path, python=False)       # (Python's gzip looks for the trailer behind the final block, not at BSIZE: it cannot read the case with bytes between)


BAD = [c[0] for c in cases() if c[1] == "bad" and c[3] > 0]


@pytest.mark.parametrize("name", BAD)
def test_every_reject_class_on_the_device(tmp_path, name):
    """a valid file with one member in the middle replaced by an invalid case of the conformance table (the bytes that passed the CPU
    test): both decoders raise the inflate error, neither returns arrays.  (A member whose ISIZE is 0 is not inflated by either decoder;
    every invalid case therefore inflates at least one byte first.)"""
    _, _, payload, isize, _ = next(c for c in cases() if c[0] == name)
    rng = np.random.default_rng(11)
    raw = _random_bam_bytes(rng, 600)
    good = _bgzf(raw, 3000, 6)
    offs, o = [], 0
    while o < len(good):
        offs.append(o)
        o += struct.unpack_from("<H", good, o + 16)[0] + 1
    k = len(offs) // 2
    bad = good[:offs[k]] + D.bgzf_member(payload, crc=0x12345678, isize=isize) + good[offs[k + 1]:]
    path = str(tmp_path / "bad.bam")
    open(path, "wb").write(bad)
    _both_raise(path, "inflate failed")


def test_reject_classes_cover_every_error_code():
    assert len(BAD) >= 65 and not [c[0] for c in cases() if c[1] == "bad" and c[3] == 0 and c[0] != "empty_payload"]


def test_empty_member_with_a_nonzero_crc_field(tmp_path):
    rng = np.random.default_rng(12)
    raw = _random_bam_bytes(rng, 600)
    good = _file(raw, range(0, len(raw), 2500))
    path = str(tmp_path / "ok.bam")
    cut = 18 + struct.unpack_from("<H", good, 16)[0] + 1 - 18
    open(path, "wb").write(good[:cut] + D.bgzf_member(bytes([3, 0])) + good[cut:])
    _both(path)
    open(path, "wb").write(good[:cut] + D.bgzf_member(bytes([3, 0]), crc=1) + good[cut:])
    _both_raise(path, "CRC-32 mismatch in the BGZF member at file offset %d " % cut)


def _decoy_raw(rng, units, chain, n_refs=3, inside=False, at_end=False):
    """records whose auxiliary bytes hold `chain` well-formed fake records in a row (valid reference ids, name terminator, sizes that
    add up, flag 99: believing them would add reads), eight bytes of 0xff behind them, and a cut where each chain starts; true records
    follow in the same member.  inside: ONE record holds every chain, so the members lie wholly inside it.  at_end: the last record's
    data ends with a chain, at the end of the file's data"""
    head = _header(n_refs)
    parts, cuts, off = [head], [], len(head)

    def fakes():
        return b"".join(_rec(int(rng.integers(0, n_refs)), int(rng.integers(0, 1 << 20)), 99, 200, b"fk\0", 1, 4) for _ in range(chain))
    if inside:
        aux = bytearray(b"XAZ\0")
        marks = []
        for _ in range(units):
            marks.append(len(aux))
            aux += fakes() + b"\xff" * 8
        rec = _rec(0, 100, 99, 150, b"big\0", aux=bytes(aux))
        cuts = [off + len(rec) - len(aux) + m for m in marks]
        parts += [rec] + [_random_rec(rng, n_refs) for _ in range(20)]
        return b"".join(parts), cuts
    for u in range(units):
        f = fakes()
        rec = _rec(int(rng.integers(0, n_refs)), int(rng.integers(0, 1 << 20)), int(rng.choice([99, 147])), 180, b"t\0", aux=b"XAZ\0" + f + b"\xff" * 8)
        cuts.append(off + len(rec) - 8 - len(f))
        parts.append(rec)
        off += len(rec)
        for _ in range(1 + int(rng.integers(3))):
            parts.append(_random_rec(rng, n_refs))
            off += len(parts[-1])
    if at_end:
        f = fakes()
        rec = _rec(0, 5, 99, 120, b"e\0", aux=b"XAZ\0" + f)
        cuts.append(off + len(rec) - len(f))
        parts.append(rec)
    return b"".join(parts), cuts


def _kept(raw_path_dev):
    return sum(len(raw_path_dev.pos[c]) for c in raw_path_dev.references)


@pytest.mark.parametrize("window", [0, 30000])
def test_decoy_led_members_are_walked_again(tmp_path, monkeypatch, window):
    """(a) a few hundred members that start at a believable false chain of eight records: the device's guess is wrong for each, the host
    walks them again from where the chain really arrives, and the file is still answered by the device"""
    raw, cuts = _decoy_raw(np.random.default_rng(21), 300, 8, at_end=True)
    path = str(tmp_path / "decoy.bam")
    open(path, "wb").write(_file(raw, cuts))
    if window:
        monkeypatch.setenv("NATAC_BAM_DEV_WINDOW", str(window))
    assert _kept(_both(path)) > 200


def test_more_decoy_led_members_than_the_host_walks_again(tmp_path):
    """(b) the same constructor with more than 4,096 such members in one window: the device path hands the file to the host decoder --
    which proves that the decoys of (a) defeat the guess.  With chains of SEVEN the guess is not taken in and the device answers; so it
    does when the same number of decoy-led members lie wholly inside one record (the host skips a member that owns no record)"""
    path = str(tmp_path / "decoy.bam")
    raw, cuts = _decoy_raw(np.random.default_rng(22), 4300, 8)
    open(path, "wb").write(_file(raw, cuts))
    assert _kept(_both(path, on_device=False)) > 3000
    raw, cuts = _decoy_raw(np.random.default_rng(22), 4300, 7)
    open(path, "wb").write(_file(raw, cuts))
    assert _kept(_both(path)) > 3000
    raw, cuts = _decoy_raw(np.random.default_rng(23), 4300, 8, inside=True)
    open(path, "wb").write(_file(raw, cuts))
    _both(path)


def test_unmapped_only_and_zero_references(tmp_path):
    rng = np.random.default_rng(31)
    path = str(tmp_path / "u.bam")
    raw = _header(3) + b"".join(_rec(-1, -1, int(rng.choice([4, 77, 141])), 0, b"u%d\0" % i, lseq=int(rng.integers(0, 90))) for i in range(3000))
    open(path, "wb").write(_file(raw, range(0, len(raw), 1777)))
    assert _kept(_both(path)) == 0
    raw = _header(0) + b"".join(_rec(-1, -1, 77, 0, b"\0", lseq=int(rng.integers(0, 90))) for i in range(3000))
    open(path, "wb").write(_file(raw, range(0, len(raw), 911)))
    dev = _both(path)
    assert dev.references == []
