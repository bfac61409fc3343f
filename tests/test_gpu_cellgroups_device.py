"""A fragment file split by cell barcode on the device (natac_frag_split_device, csrc/natac_fragfile_dev.hpp: frag_split_parse, frag_split_compact,
frag_split_hist, frag_split_scatter) against the host path (natac_frag_split, itself checked against two restatements of the rule in
tests/test_cellgroups_host.py): the same arrays and per-barcode counts, exactly, with the device answering -- for members and windows that
cut barcodes, windows without an assigned line and of one group, group changes on the kernels' line counts, the most groups, chains of
equal hashes, a table in which probing certainly occurs; the hand-over to the host path for malformed lines; and `pyatac split` feeding
`pyatac sizes`."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from cellgroups_ref import assert_same_split, crafted
from nucleoatac_amd.pyatac.fragments import FragmentStore

pytestmark = pytest.mark.gpu

EOF_MARKER = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
WORKGROUP, WAVE, PART_LINES = 256, 64, 8192            # TILE_T, PART_T and PART_LINES of csrc/natac_fragfile_dev.hpp
MAX_GROUPS = 255


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


def _both(path, barcodes, group_of, G):
    host = FragmentStore.split_fragments(path, barcodes, group_of, G, device=False)
    dev = FragmentStore.split_fragments(path, barcodes, group_of, G, device=True)
    assert FragmentStore.last_frag_on_device is True
    assert_same_split(dev, host)
    return dev


def _n(split):
    return sum(len(st.pos[c]) for st in split[0] for c in st.references)


@pytest.fixture(scope="module")
def text_and_table():
    text, listed = crafted()
    return text, listed, [k % 7 for k in range(len(listed))]


@pytest.mark.parametrize("blk,window", [(100, 0), (4000, 0), (0xff00, 0), (100, 2500), (4000, 3000)])
def test_device_split_equals_host_split_on_the_crafted_file(tmp_path, monkeypatch, text_and_table, blk, window):
    text, listed, group_of = text_and_table
    # a comment line in front, as long as it takes for the first member border to fall inside a barcode: barcodes straddle members
    text = next(t for t in (b"#" + b"p" * pad + b"\n" + text for pad in range(200)) if _inside_a_barcode(t, blk))
    z = _bgzf(text, blk)
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(z)
    if window:
        monkeypatch.setenv("NATAC_FRAG_DEV_WINDOW", str(window))
        cuts = _windows(z, window)
        assert len(cuts) > 15 and any(_inside_a_barcode(text, o) for o in cuts)        # ... and windows: the carry holds half a barcode
    dev = _both(path, listed, group_of, 7)
    assert _n(dev) > 2000 and dev[2] > 300 and dev[0][0].references == ["chr1", "chr2", "chrOnlyUnassigned", "chr3_random"]


def test_windows_without_an_assigned_line_and_of_one_group(tmp_path, monkeypatch):
    lines = [b"chr1\t%d\t%d\tNOBODY%d-1\n" % (i, i + 100, i % 50) for i in range(4000)]
    lines += [b"chr1\t%d\t%d\tCELL%d-1\t2\n" % (i, i + 100, i % 5) for i in range(4000, 8000)]
    lines += [b"chr2\t%d\t%d\tNOBODY-1\n" % (i, i + 100) for i in range(3000)]
    text = b"".join(lines)
    z = _bgzf(text, 3000)
    cuts = [0] + _windows(z, 2000) + [len(text)]
    first, second = len(b"".join(lines[:4000])), len(b"".join(lines[:8000]))
    assert any(b <= first for a, b in zip(cuts, cuts[1:])) and any(first <= a and b <= second for a, b in zip(cuts, cuts[1:]))
    assert any(second <= a for a in cuts[:-1])
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(z)
    monkeypatch.setenv("NATAC_FRAG_DEV_WINDOW", "2000")
    barcodes = [b"CELL%d-1" % k for k in range(5)] + [b"ABSENT-1"]
    dev = _both(path, barcodes, [1, 1, 1, 1, 1, 0], 3)
    assert [sum(len(st.pos[c]) for c in st.references) for st in dev[0]] == [0, 4000, 0] and dev[2] == 7000
    assert dev[0][0].references == ["chr1", "chr2"] and dev[0][1].lengths == [8099, 3099]
    none = _both(path, [b"ABSENT-1"], [0], 1)                # no line of the whole file is assigned
    assert _n(none) == 0 and none[2] == 11000 and none[0][0].references == ["chr1", "chr2"]


def test_group_changes_on_the_kernels_line_counts(tmp_path):
    """the first 1,024 lines change group at every multiple of the wave's 64 lines (so also at the parse workgroup's 256), the rest at the
    partition tile's 8,192 and at 16,384; a second file shifts everything by one line"""
    n = 2 * PART_LINES + 1024
    group = np.where(np.arange(n) < 1024, np.arange(n) // WAVE, 16 + np.arange(n) // PART_LINES)
    assert group.max() == 18 and WORKGROUP % WAVE == 0
    barcodes = [b"GROUP%02d-1" % g for g in range(19)]
    lines = [b"chr%d\t%d\t%d\t%s\n" % (1 + i // 9000, i, i + 7 + i % 13, barcodes[g]) for i, g in enumerate(group.tolist())]
    path = str(tmp_path / "f.tsv.gz")
    for shift in (b"", b"# one line more\n"):
        open(path, "wb").write(_bgzf(shift + b"".join(lines), 0xff00, 1))
        dev = _both(path, barcodes, list(range(19)), 19)
        assert [sum(len(st.pos[c]) for c in st.references) for st in dev[0]] == np.bincount(group).tolist() and dev[2] == 0


def test_the_most_groups_round_robin(tmp_path):
    barcodes = [b"CELL%03d" % k for k in range(MAX_GROUPS)]
    rng = np.random.default_rng(4)
    start = rng.integers(0, 1_000_000, 12000)
    lines = [b"chr%d\t%d\t%d\t%s\t1\n" % (1 + i // 5000, s, s + 50 + i % 9, barcodes[i % MAX_GROUPS]) for i, s in enumerate(start.tolist())]
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(_bgzf(b"".join(lines), 0xff00, 1))
    dev = _both(path, barcodes, list(range(MAX_GROUPS)), MAX_GROUPS)
    assert _n(dev) == 12000 and len(dev[0]) == MAX_GROUPS and int(dev[1].min()) == 12000 // MAX_GROUPS


def test_chains_of_equal_hashes(tmp_path, monkeypatch):
    text, listed = crafted(seed=5, n_cells=64)
    assert 45 <= len(listed) <= 60
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(_bgzf(text, 4000))
    want = _both(path, listed, [k % 4 for k in range(len(listed))], 4)
    monkeypatch.setenv("NATAC_SPLIT_HASH_BITS", "3")          # 8 hash values: nearly every lookup walks a chain of equal hashes
    assert_same_split(_both(path, listed, [k % 4 for k in range(len(listed))], 4), want)


def test_a_table_in_which_probing_certainly_occurs(tmp_path):
    rng = np.random.default_rng(6)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    cells = list(dict.fromkeys(bytes(letters[rng.integers(0, 4, 16)]) + b"-1" for _ in range(6000)))
    listed = cells[:5000]                                    # 5,000 keys in 16,384 slots: the chance of not one collision is nil
    start = np.sort(rng.integers(0, 30_000_000, 15000))
    lines = [b"chr%d\t%d\t%d\t%s\t1\n" % (1 + i // 6000, s, s + 40 + i % 500, cells[int(k)])
             for i, (s, k) in enumerate(zip(start.tolist(), rng.integers(0, len(cells), 15000)))]
    path = str(tmp_path / "f.tsv.gz")
    open(path, "wb").write(_bgzf(b"".join(lines), 0xff00, 1))
    dev = _both(path, listed, [k % 16 for k in range(5000)], 16)
    assert 11000 < _n(dev) < 14000 and _n(dev) + dev[2] == 15000 and int(dev[1].sum()) == _n(dev)


def _raw(path, barcodes, device):
    """the C entry points called directly -> (return code, message, on_device)"""
    from nucleoatac_amd import _lib as L, get_context
    lib = L.load()
    off = np.zeros(len(barcodes) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in barcodes], out=off[1:])
    blob = np.frombuffer(b"".join(barcodes) + b"\0", dtype=np.uint8)
    grp = np.zeros(len(barcodes), dtype=np.int32)
    handles = (C.c_void_p * 1)(0xdead)
    table = (len(barcodes), blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), grp.ctypes.data_as(C.c_void_p), 1,
             C.cast(handles, C.c_void_p), None, None)
    on_dev = C.c_int(1)
    if device:
        rc = lib.natac_frag_split_device(get_context()._h, path.encode(), *table, C.byref(on_dev))
    else:
        rc = lib.natac_frag_split(path.encode(), 0, *table)
    assert rc != 0 and handles[0] is None
    return rc, lib.natac_last_error().decode(), on_dev.value if device else 0


@pytest.mark.parametrize("line,reason", [(b"chr1\t5\t9", "no barcode field"), (b"chr1\t9\t5", "end before start"),
                                         (b"chr1\t5\t7x\tAA", "start / end is not a number")])
def test_malformed_lines_are_the_host_paths(tmp_path, line, reason):
    good = [b"chr1\t%d\t%d\tAA\n" % (i, i + 50) for i in range(3000)]
    path = str(tmp_path / "bad.tsv.gz")
    open(path, "wb").write(_bgzf(b"".join(good[:2000] + [line + b"\n"] + good[2000:]), 3000))
    host = _raw(path, [b"AA"], device=False)
    assert host[:2] == (-1, "%s: line 2001: %s" % (path, reason))
    assert _raw(path, [b"AA"], device=True) == (host[0], host[1], 0)


def test_split_then_sizes_equals_sizes_of_the_groups_own_file(tmp_path, monkeypatch, text_and_table):
    from nucleoatac_amd.pyatac.cli import main
    text, listed, _ = text_and_table
    listed = [b for b in listed if b"#" not in b]
    monkeypatch.chdir(tmp_path)
    open("cells.tsv.gz", "wb").write(_bgzf(text, 4000))
    open("groups.tsv", "wb").write(b"".join(b"%s\t%s\n" % (b, b"AB"[k % 2:k % 2 + 1]) for k, b in enumerate(listed)))
    assert main(["split", "--fragments", "cells.tsv.gz", "--groups", "groups.tsv"]) == 0
    assert FragmentStore.last_frag_on_device is True and os.path.exists("cells.A.npz") and os.path.exists("cells.B.npz")
    mine = set(listed[0::2])
    body = [x[:-1] if x.endswith(b"\r") else x for x in text.split(b"\n")[:-1]] + [text.split(b"\n")[-1]]      # (the open last line keeps its '\r')
    kept = [x for x in body if x and not x.startswith(b"#") and x.split(b"\t")[3] in mine]
    assert len(kept) > 800
    open("onlyA.tsv.gz", "wb").write(_bgzf(b"\n".join(kept) + b"\n", 4000))
    assert main(["sizes", "--bam", "cells.A.npz", "--out", "split"]) == 0
    assert main(["sizes", "--bam", "onlyA.tsv.gz", "--out", "alone"]) == 0
    a, b = open("split.fragmentsizes.txt", "rb").read(), open("alone.fragmentsizes.txt", "rb").read()
    assert a == b and len(a) > 100
