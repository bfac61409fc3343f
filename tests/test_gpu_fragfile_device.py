"""Fragment file -> fragment arrays on the device (csrc/natac_fragfile_dev.hpp: BGZF members inflated as a BAM's, then the text split into
lines, parsed and compacted by the device) against the host decoder (natac_fragfile.hpp, itself checked against the Python restatement
of the format rule in tests/test_fragfile_host.py): the same arrays for members of every size and deflate block type, windows small
enough that lines and headers straddle them, the hand-over to the host decoder where the device path declines, the host decoder's
errors for damaged files, and byte-identical command outputs from a BAM and from the fragment file made of it."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

from nucleoatac_amd.pyatac.fragments import FragmentStore

pytestmark = pytest.mark.gpu

EOF_MARKER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _bgzf(data, blk, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    out = bytearray()
    for o in range(0, len(data), blk):
        chunk = data[o:o + blk]
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        comp = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(comp) + 8 - 1)
        out += comp + struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk))
    return bytes(out) + EOF_MARKER


def _same(a, b):
    assert a.references == b.references and list(a.lengths) == list(b.lengths)
    for c in a.references:
        assert np.array_equal(a.pos[c], b.pos[c]) and np.array_equal(a.tlen[c], b.tlen[c]), c


def _both(path, on_device=True):
    host = FragmentStore.from_fragments(path, device=False)
    dev = FragmentStore.from_fragments(path, device=True)
    assert FragmentStore.last_frag_on_device is on_device
    _same(host, dev)
    return dev


def _n(st):
    return sum(len(st.pos[c]) for c in st.references)


def _lines(seed, n=6000):
    """~n lines of ~30 bytes over 5 chromosomes, the first coming back at the end; 3 to 5 columns, some CRLF, empty lines, '#' headers of
    ~400 bytes at the top and inside, duplicates, unsorted stretches"""
    rng = np.random.default_rng(seed)
    names = [b"chr1", b"chr2", b"chrX_random", b"c", b"chrUn_KI270442v1", b"chr1"]
    out = [b"# id=sample " + b"h" * 400 + b"\n", b"#\tsecond header line\n"]
    per = n // len(names)
    for k, c in enumerate(names):
        start = np.sort(rng.integers(0, 40_000_000, per))
        if k == 2:
            start = rng.permutation(start)
        end = start + rng.integers(0, 1200, per)
        for i in range(per):
            kind = int(rng.integers(0, 12))
            tail = (b"", b"\tACGTACGTACGTAC-1", b"\tACGTAC#TACGTAC-1\t%d" % int(rng.integers(1, 9)))[kind % 3]
            line = b"%s\t%d\t%d%s%s\n" % (c, start[i], end[i], tail, b"\r" if kind == 7 else b"")
            out.append(line)
            if kind == 11:
                out.append((b"\n", line, b"# note " + b"x" * int(rng.integers(0, 400)) + b"\n")[i % 3])
    return b"".join(out)


def _windows(z, window):
    """the inflated offsets at which the device path's windows end: members are taken while they end inside win_start + window (one at
    least), DevWindows::next of natac_bgzf_dev.hpp"""
    ends, sizes, o = [], [], 0
    while o < len(z):
        bsize = struct.unpack_from("<H", z, o + 16)[0] + 1
        sizes.append(struct.unpack_from("<I", z, o + bsize - 4)[0])
        o += bsize
        ends.append(o)
    cuts, win_start, m, u = [], 0, 0, 0
    while m < len(ends):
        m1 = m
        while m1 < len(ends) and (m1 == m or ends[m1] <= win_start + window):
            u += sizes[m1]
            m1 += 1
        cuts.append(u)
        win_start, m = ends[m1 - 1], m1
    return cuts[:-1]


GRID = [(100, 6, zlib.Z_DEFAULT_STRATEGY, 0), (100, 1, zlib.Z_DEFAULT_STRATEGY, 2500), (300, 9, zlib.Z_DEFAULT_STRATEGY, 0),
        (300, 6, zlib.Z_FIXED, 2500), (3000, 1, zlib.Z_DEFAULT_STRATEGY, 0), (3000, 0, zlib.Z_DEFAULT_STRATEGY, 40000),
        (65280, 6, zlib.Z_DEFAULT_STRATEGY, 0), (65280, 0, zlib.Z_DEFAULT_STRATEGY, 40000), (65536, 6, zlib.Z_DEFAULT_STRATEGY, 0),
        (65536, 9, zlib.Z_FIXED, 40000)]


@pytest.mark.parametrize("blk,level,strategy,window", GRID)
def test_device_decoder_equals_host_decoder(tmp_path, monkeypatch, blk, level, strategy, window):
    text = _lines(blk + level)
    if blk == 100:
        # members of about three lines: their borders fall inside numbers, on a TAB, on the '\n' and right behind it
        cuts = range(blk, len(text), blk)
        assert any(text[o - 1:o].isdigit() and text[o:o + 1].isdigit() for o in cuts)
        assert any(text[o:o + 1] == b"\t" for o in cuts) and any(text[o:o + 1] == b"\n" for o in cuts)
        assert any(text[o - 1:o] == b"\n" for o in cuts)
    z = _bgzf(text, blk, level, strategy)
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(z)
    if window:
        monkeypatch.setenv("NATAC_FRAG_DEV_WINDOW", str(window))
        cuts = _windows(z, window)
        inside = [text.rfind(b"\n", 0, o) + 1 for o in cuts if text[o - 1:o] != b"\n"]      # starts of the lines that straddle a window border
        assert any(text[a:a + 3] == b"chr" for a in inside)
        if window == 2500:
            assert len(cuts) > 30 and any(text[a:a + 1] == b"#" for a in inside)
    dev = _both(path)
    assert _n(dev) > 5500 and dev.references == ["chr1", "chr2", "chrX_random", "c", "chrUn_KI270442v1"]


def test_hand_over_to_the_host_decoder(tmp_path, monkeypatch):
    path = str(tmp_path / "f.tsv.gz")
    # one line with a 100-kB fourth column (random letters: ~75 kB compressed) under a 40,000-byte window: a window without a line end
    rng = np.random.default_rng(1)
    text = b"chr9\t5\t900\t" + bytes(rng.integers(65, 91, 100000, dtype=np.uint8)) + b"\nchr9\t7\t80\n" + _lines(1, 600)
    z = _bgzf(text, 65280, 6)
    assert _windows(z, 40000)[0] == 65280                     # the first window is the first member, all of it inside that line
    open(path, "wb").write(z)
    with monkeypatch.context() as m:
        m.setenv("NATAC_FRAG_DEV_WINDOW", "40000")
        assert _n(_both(path, on_device=False)) > 500
    assert _n(_both(path)) > 500                              # (in one window the device answers)
    # two chromosomes alternating on every line: more than 65,536 runs in one window
    lines = [b"chr%d\t%d\t%d\n" % (i & 1, i, i + 100) for i in range(70000)]
    open(path, "wb").write(_bgzf(b"".join(lines), 65280, 1))
    assert _n(_both(path, on_device=False)) == 70000
    open(path, "wb").write(_bgzf(b"".join(lines[:65536]), 65280, 1))      # at the cap: every line a run of its own
    assert _n(_both(path)) == 65536
    # another container
    open(path, "wb").write(gzip.compress(_lines(2, 600)))
    assert _n(_both(path, on_device=False)) > 500


def test_degenerate_files(tmp_path):
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(_bgzf(b"# only\n#comments\n\n", 10, 6))
    assert _both(path).references == []
    open(path, "wb").write(EOF_MARKER)
    assert _both(path).references == []
    open(path, "wb").write(_bgzf(b"chr7\t12\t99\tno-newline", 7, 6))
    dev = _both(path)
    assert dev.references == ["chr7"] and dev.pos["chr7"].tolist() == [8] and dev.tlen["chr7"].tolist() == [95] and dev.lengths == [99]
    open(path, "wb").write(_bgzf(b"chr7\t12\t99\r", 5, 6))      # a '\r' without '\n' behind it belongs to the field
    for device in (False, True):
        with pytest.raises(Exception, match=r"f\.tsv\.gz: line 1: start / end is not a number"):
            FragmentStore.from_fragments(path, device=device)


def test_large_file_and_damage(tmp_path):
    """400,000 lines through 64-KiB members, then the same file truncated / garbled, and a malformed line in the middle of a file: the
    device path reports what the host decoder reports"""
    rng = np.random.default_rng(5)
    n = 400000
    chrom = np.sort(rng.integers(0, 3, n))
    start = rng.integers(0, 5_000_000, n)
    order = np.lexsort((start, chrom))
    chrom, start = chrom[order], start[order]
    end = start + rng.integers(0, 900, n)
    names = [b"chrI", b"chrII", b"chrIII"]
    text = b"".join([b"%s\t%d\t%d\tBC%d\n" % (names[c], s, e, s & 1023) for c, s, e in zip(chrom.tolist(), start.tolist(), end.tolist())])
    z = _bgzf(text, 65280, 1)
    path = str(tmp_path / "big.tsv.gz")
    open(path, "wb").write(z)
    dev = _both(path)
    assert _n(dev) == n and [len(dev.pos[c.decode()]) for c in names] == np.bincount(chrom).tolist()
    for c in range(3):
        assert np.array_equal(dev.pos[names[c].decode()], start[chrom == c] - 4)
    assert dev.lengths == [int(end[chrom == c].max()) for c in range(3)]

    def errors(data, name):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        msgs = []
        for device in (False, True):
            with pytest.raises(Exception) as e:
                FragmentStore.from_fragments(p, device=device)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1]
        return msgs[0]
    assert "trailing bytes after the last BGZF block" in errors(z[:len(z) // 2], "cut.tsv.gz")
    g = bytearray(z)
    g[len(g) // 3] ^= 0x55
    g[len(g) // 3 + 1] ^= 0xaa
    msg = errors(bytes(g), "bad.tsv.gz")
    assert "inflate failed" in msg or "CRC-32 mismatch" in msg
    lines = _lines(8).split(b"\n")[:6000]
    lines[3000] = b"chr2\t77\t7x"
    assert errors(_bgzf(b"\n".join(lines) + b"\n", 3000, 6), "line.tsv.gz").endswith("line.tsv.gz: line 3001: start / end is not a number")


def test_commands_write_the_same_files_from_a_bam_and_from_its_fragment_file(tmp_path):
    from helpers import GOLDEN, read_bed3, synth_saccer3
    from nucleoatac_amd.nucleoatac.cli import main as nucleoatac_main
    from nucleoatac_amd.pyatac.cli import main as pyatac_main
    from nucleoatac_amd.synth import cli_dataset_as_real_files
    regions = read_bed3(os.path.join(GOLDEN, "ref_example.bed"))[:4]
    bed = str(tmp_path / "regions.bed")
    with open(bed, "w") as f:
        f.write("".join("%s\t%d\t%d\n" % r for r in regions))
    bam_npz, fa = synth_saccer3(str(tmp_path), regions, seed=3)
    bam, _ = cli_dataset_as_real_files(bam_npz, fa, str(tmp_path))
    frag = str(tmp_path / "reads.tsv.gz")
    store = FragmentStore.from_bam(bam)
    store.save_fragments(frag)
    back = FragmentStore.from_fragments(frag)
    assert FragmentStore.last_frag_on_device is True and _n(back) == _n(store) > 10000
    outs = {}
    for tag, src in (("b", bam), ("f", frag)):
        out = str(tmp_path / tag)
        assert pyatac_main(["ins", "--bam", src, "--bed", bed, "--out", out]) == 0
        assert pyatac_main(["sizes", "--bam", src, "--out", out]) == 0
        nucleoatac_main(["occ", "--bed", bed, "--bam", src, "--fasta", fa, "--out", out])
        outs[tag] = {n: open(out + n, "rb").read() for n in (".ins.bedgraph.gz", ".fragmentsizes.txt", ".occ.bedgraph.gz")}
    for n, data in outs["b"].items():
        assert data == outs["f"][n] and len(data) > 100, n
