"""The cells of a fragment file discovered on the device (natac_frag_cells_device, csrc/natac_fragfile_dev.hpp: cells_parse, cells_claim,
cells_verify, cells_number, cells_adopt, cells_count) against the host path (natac_frag_cells, itself checked against two restatements of
the rule in tests/test_cells_host.py): the same barcodes in the same order and the same counters, exactly, with the device answering --
for members and windows that cut barcodes, barcodes that come back in later windows, chains of equal hashes, first appearances on the
kernels' line counts, duplicate lines and long runs of one cell, a table in which probing certainly occurs; the documented hand-over of a
full table and of malformed lines to the host path; and `pyatac cells` feeding `pyatac cellcounts`."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from cells_ref import assert_same_table, assert_table_equals_ref, cells_ref, crafted
from nucleoatac_amd.pyatac.fragments import FragmentStore

pytestmark = pytest.mark.gpu

EOF_MARKER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
WORKGROUP, WAVE, PART_LINES = 256, 64, 8192            # TILE_T, a wave and the largest line count of csrc/natac_fragfile_dev.hpp's kernels


def _bgzf(data, blk, level=6):
    out = bytearray()
    for o in range(0, len(data), blk):
        chunk = data[o:o + blk]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        out += bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", 18 + len(comp) + 8 - 1)
        out += comp + struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk))
    return bytes(out) + EOF_MARKER


def _windows(z, window):
    """the inflated offsets at which the device path's windows end (members are taken while they end inside win_start + window, one at least)"""
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


def _inside_a_barcode(text, o):
    """does offset o cut the fourth field of its line in two"""
    a = text.rfind(b"\n", 0, o) + 1
    e = text.find(b"\n", o)
    tabs = [i for i in range(a, e if e >= 0 else len(text)) if text[i:i + 1] == b"\t"]
    return len(tabs) >= 3 and tabs[2] + 1 < o < (tabs[3] if len(tabs) > 3 else (e if e >= 0 else len(text)))


def _both(path, *bounds, on_device=True):
    host = FragmentStore.discover_cells(path, *bounds, device=False)
    dev = FragmentStore.discover_cells(path, *bounds, device=True)
    assert FragmentStore.last_frag_on_device is on_device
    assert_same_table(dev, host)
    return dev


@pytest.fixture(scope="module")
def crafted_text():
    text, _ = crafted()
    return text, cells_ref(text)


@pytest.mark.parametrize("blk,window", [(100, 0), (4000, 0), (0xff00, 0), (100, 2500), (4000, 3000)])
def test_device_table_equals_host_table_on_the_crafted_file(tmp_path, monkeypatch, crafted_text, blk, window):
    text, _ = crafted_text
    # a comment line in front, as long as it takes for the first member border to fall inside a barcode: barcodes straddle members
    text = next(t for t in (b"#" + b"p" * pad + b"\n" + text for pad in range(200)) if _inside_a_barcode(t, blk))
    z = _bgzf(text, blk)
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(z)
    if window:
        monkeypatch.setenv("NATAC_FRAG_DEV_WINDOW", str(window))
        cuts = [0] + _windows(z, window) + [len(text)]
        assert len(cuts) > 17 and any(_inside_a_barcode(text, o) for o in cuts)        # ... and windows: the carry holds half a barcode
        # a barcode first seen in one window is met again in later ones
        bc = b"\t" + cells_ref(text)["barcodes"][0] + b"\n"
        assert sum(1 for a, b in zip(cuts, cuts[1:]) if bc in text[a:b]) > 5
    dev = _both(path)
    assert_table_equals_ref(dev, cells_ref(text))
    assert len(dev) > 45 and dev.n_unassigned > 30 and int(dev.n_frag.sum()) > 2500


def test_other_bounds_on_the_device(tmp_path, crafted_text):
    text, _ = crafted_text
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(_bgzf(text, 4000))
    dev = _both(path, 100, 500)
    assert_table_equals_ref(dev, cells_ref(text, 100, 500))
    assert not np.array_equal(dev.n_nfr, _both(path).n_nfr)


def test_chains_of_equal_hashes_across_windows(tmp_path, monkeypatch):
    text, _ = crafted(seed=5)
    ref = cells_ref(text)
    assert 45 <= len(ref["barcodes"]) <= 55
    z = _bgzf(text, 3000)
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(z)
    want = _both(path)
    monkeypatch.setenv("NATAC_SPLIT_HASH_BITS", "3")          # 8 home slots: nearly every line walks a chain of equal hashes
    assert_same_table(_both(path), want)
    monkeypatch.setenv("NATAC_FRAG_DEV_WINDOW", "2500")       # ... and the chains grow from window to window
    assert len(_windows(z, 2500)) > 15
    assert_same_table(_both(path), want)
    assert_table_equals_ref(want, ref)


def _placed(news, n, shift=b""):
    """n lines of three old cells, but line i (0-based) of the file belongs to a new cell for every i of `news` and, from then on, to
    every later line whose number is a multiple of 97"""
    lines, met = [], []
    for i in range(n):
        j = i - (1 if shift else 0)
        if shift and i == 0:
            lines.append(shift)
            continue
        if j in news:
            met.append(b"NEW%05d-1" % j)
        bc = met[(j // 97) % len(met)] if met and j not in news and j % 97 == 0 else (met[-1] if j in news else b"OLD%d-1" % (j % 3))
        lines.append(b"chr%d\t%d\t%d\t%s\n" % (1 + j // 9000, j, j + 40 + j % 300, bc))
    return b"".join(lines)


def test_first_appearances_on_the_kernels_line_counts(tmp_path):
    news = {WAVE - 1, WAVE, WAVE + 1, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, PART_LINES - 1, PART_LINES}
    assert sorted(news) == [63, 64, 65, 255, 256, 257, 8191, 8192]
    path = str(tmp_path / "f.tsv.gz")
    for shift in (b"", b"# one line more\n"):
        text = _placed(news, PART_LINES + 700, shift)
        open(path, "wb").write(_bgzf(text, 0xff00, 1))
        dev = _both(path)
        assert dev.barcodes == [b"OLD0-1", b"OLD1-1", b"OLD2-1"] + [b"NEW%05d-1" % j for j in sorted(news)]
        assert_table_equals_ref(dev, cells_ref(text))


def test_duplicate_lines_and_a_run_of_one_cell(tmp_path):
    rng = np.random.default_rng(8)
    lines = []
    for i in range(3000):
        bc = b"RUN-1" if 1000 <= i < 1200 else b"CELL%02d-1" % int(rng.integers(0, 20))       # 200 consecutive lines of one cell
        line = b"chr1\t%d\t%d\t%s\t2\n" % (i, i + int(rng.integers(0, 400)), bc)
        lines += [line] * (3 if i % 50 == 0 else 1)                                           # identical lines are separate fragments
    text = b"".join(lines)
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(_bgzf(text, 0xff00, 1))
    dev = _both(path)
    assert_table_equals_ref(dev, cells_ref(text))
    assert dev.n_frag[dev.barcodes.index(b"RUN-1")] >= 200 and dev.n_data == len(lines) == 3120


def _hundred(tmp_path):
    rng = np.random.default_rng(11)
    cells = [b"BC%03d-1" % k for k in range(100)]
    lines = [b"chr1\t%d\t%d\t%s\n" % (i, i + int(rng.integers(0, 400)), cells[int(k)]) for i, k in enumerate(rng.integers(0, 100, 4000))]
    text = b"".join(lines)
    path = str(tmp_path / "hundred.tsv.gz")
    open(path, "wb").write(_bgzf(text, 3000))
    return path, text


def test_a_full_table_is_handed_over_as_documented(tmp_path, monkeypatch):
    """the table has a fixed size and takes at most slots / 2 cells (include/natac.h): 100 barcodes in 64 slots are the host path's, in 128
    slots too, in 256 slots the device's -- at a load at which probing certainly occurs"""
    path, text = _hundred(tmp_path)
    ref = cells_ref(text)
    assert len(ref["barcodes"]) == 100
    monkeypatch.setenv("NATAC_CELLS_DEV_SLOTS", "64")
    assert_table_equals_ref(_both(path, on_device=False), ref)
    monkeypatch.setenv("NATAC_CELLS_DEV_SLOTS", "128")
    assert_table_equals_ref(_both(path, on_device=False), ref)
    monkeypatch.setenv("NATAC_FRAG_DEV_WINDOW", "2500")       # the table fills up window by window
    assert_table_equals_ref(_both(path, on_device=False), ref)
    monkeypatch.setenv("NATAC_CELLS_DEV_SLOTS", "256")
    assert_table_equals_ref(_both(path, on_device=True), ref)
    monkeypatch.delenv("NATAC_FRAG_DEV_WINDOW")
    assert_table_equals_ref(_both(path, on_device=True), ref)


def _raw(path, device):
    """the C entry points called directly -> (return code, message, on_device)"""
    from nucleoatac_amd import _lib as L, get_context
    lib = L.load()
    h = C.c_void_p(0xdead)
    on_dev = C.c_int(1)
    if device:
        rc = lib.natac_frag_cells_device(get_context()._h, path.encode(), 147, 294, C.byref(h), C.byref(on_dev))
    else:
        rc = lib.natac_frag_cells(path.encode(), 0, 147, 294, C.byref(h))
    assert rc != 0 and h.value is None
    return rc, lib.natac_last_error().decode(), on_dev.value if device else 0


@pytest.mark.parametrize("line,reason", [(b"chr1\t5\t9", "no barcode field"), (b"chr1\t5\t7x\tAA", "start / end is not a number")])
def test_malformed_lines_are_the_host_paths(tmp_path, line, reason):
    good = [b"chr1\t%d\t%d\tAA%d\n" % (i, i + 50, i % 9) for i in range(3000)]
    path = str(tmp_path / "bad.tsv.gz")
    open(path, "wb").write(_bgzf(b"".join(good[:2000] + [line + b"\n"] + good[2000:]), 3000))
    host = _raw(path, device=False)
    assert host[:2] == (-1, "%s: line 2001: %s" % (path, reason))
    assert _raw(path, device=True) == (host[0], host[1], 0)


def test_cells_then_cellcounts_equals_cellcounts_of_the_same_barcodes(tmp_path, monkeypatch, crafted_text, capsys):
    from nucleoatac_amd.pyatac.cli import main
    text, ref = crafted_text
    monkeypatch.chdir(tmp_path)
    open("sc.tsv.gz", "wb").write(_bgzf(text, 4000))
    m = 60
    assert main(["cells", "--fragments", "sc.tsv.gz", "--min_fragments", str(m)]) == 0
    assert FragmentStore.last_frag_on_device is True                                  # the command takes the device on a GPU box
    by_hand = [b for b, f in zip(ref["barcodes"], ref["n_frag"].tolist()) if f >= m and not b.startswith(b"#") and not b.endswith(b"\r")]
    assert 20 < len(by_hand) < len(ref["barcodes"])
    assert open("sc.cells.tsv", "rb").read() == b"".join(b + b"\n" for b in by_hand)
    assert_table_equals_ref(_both("sc.tsv.gz"), ref)                                  # and the device's table is the command's
    open("hand.tsv", "wb").write(b"".join(b + b"\n" for b in by_hand))
    open("w.bed", "w").write("".join("chr1\t%d\t%d\n" % (s, s + 50000) for s in range(0, 2_000_000, 400_000)) + "chr2\t0\t1000000\n")
    assert main(["cellcounts", "--fragments", "sc.tsv.gz", "--bed", "w.bed", "--cells", "sc.cells.tsv", "--format", "npz", "--out", "found"]) == 0
    assert main(["cellcounts", "--fragments", "sc.tsv.gz", "--bed", "w.bed", "--cells", "hand.tsv", "--format", "npz", "--out", "hand"]) == 0
    a, b = np.load("found.cellcounts.npz"), np.load("hand.cellcounts.npz")
    assert sorted(a.files) == sorted(b.files) and len(a["data"]) > 100
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert open("found.cellcounts.txt").read() == open("hand.cellcounts.txt").read()
    capsys.readouterr()
