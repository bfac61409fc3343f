"""The device decoders share one BGZF window stream (csrc/natac_bgzf_dev.hpp: DevWindows -- the file, the member chain and its walker
thread, the pinned staging buffers, the side streams, the carry).  What sharing it can newly get wrong: state that survives from one
decode into the next of another kind on the same context, and the stream's destructor on the failure path (the walker joined, the side
streams freed with work queued on them) before the next decode starts.  Both files go through dozens of windows of 2,500 bytes."""
import struct

import numpy as np
import pytest

from cellgroups_ref import assert_same_split, crafted
from cells_ref import assert_same_table
from helpers import bgzf_bytes, write_bam
from nucleoatac_amd.pyatac.fragments import FragmentStore

pytestmark = pytest.mark.gpu

WINDOW = 2500
GROUPS = 3


def _members(z):
    """file offsets at which the members of z start, and the end of the last"""
    offs, o = [], 0
    while o < len(z):
        offs.append(o)
        o += struct.unpack_from("<H", z, o + 16)[0] + 1
    return offs + [o]


def _window_ends(z, window):
    """the file offsets at which the device path's windows end: members are taken while they end inside win_start + window (one at least)"""
    ends = _members(z)[1:]
    out, win_start, m = [], 0, 0
    while m < len(ends):
        m1 = m
        while m1 < len(ends) and (m1 == m or ends[m1] <= win_start + window):
            m1 += 1
        win_start, m = ends[m1 - 1], m1
        out.append(win_start)
    return out


def _damaged(z):
    """z with two bytes flipped inside the payload of the first member that starts behind the eleventh window"""
    ends = _window_ends(z, WINDOW)
    assert len(ends) > 24
    offs = _members(z)
    k = next(i for i, o in enumerate(offs[:-1]) if o >= ends[10])
    assert offs[k + 1] - offs[k] > 18 + 8 + 8 and k < len(offs) - 3          # a member with a payload, not the last ones
    g = bytearray(z)
    g[offs[k] + 18 + 5] ^= 0x55
    g[offs[k] + 18 + 6] ^= 0xaa
    return bytes(g)


def _same(a, b):
    assert a.references == b.references and list(a.lengths) == list(b.lengths)
    for c in a.references:
        assert np.array_equal(a.pos[c], b.pos[c]) and np.array_equal(a.tlen[c], b.tlen[c]), c


class _Files:
    pass


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the two files, their damaged twins and what the host decoders say of the sound ones (computed once)"""
    d = tmp_path_factory.mktemp("stream")
    f = _Files()
    text, listed = crafted()                                  # ~3,000 lines, 4 chromosomes, ~40 barcodes
    assert 2500 < text.count(b"\n") < 4000
    f.barcodes, f.group_of = listed, [k % GROUPS for k in range(len(listed))]
    f.frag, f.bam = str(d / "f.tsv.gz"), str(d / "a.bam")
    z = bgzf_bytes(text, 300)
    open(f.frag, "wb").write(z)
    rng = np.random.default_rng(41)
    n = 3000
    ref = np.sort(rng.integers(0, 4, n))
    pos = rng.integers(0, 5_000_000, n)
    order = np.lexsort((pos, ref))
    flag = rng.choice([99, 147, 83, 163, 4, 77], n)
    tl = rng.integers(30, 900, n) * np.where(flag & 0x10, -1, 1)
    write_bam(f.bam, [("chr%d" % r, 6_000_000) for r in range(4)], zip(ref[order].tolist(), pos[order].tolist(), flag.tolist(), tl.tolist()), blk=300)
    b = open(f.bam, "rb").read()
    f.bad_frag, f.bad_bam = str(d / "bad.tsv.gz"), str(d / "bad.bam")
    open(f.bad_frag, "wb").write(_damaged(z))
    open(f.bad_bam, "wb").write(_damaged(b))
    f.host_bam = FragmentStore.from_bam(f.bam, device=False)
    f.host_plain = FragmentStore.from_fragments(f.frag, device=False)
    f.host_split = FragmentStore.split_fragments(f.frag, f.barcodes, f.group_of, GROUPS, device=False)
    f.host_cells = FragmentStore.discover_cells(f.frag, device=False)
    assert sum(len(f.host_bam.pos[c]) for c in f.host_bam.references) > 800 and len(f.host_plain.references) == 4
    assert len(f.host_cells) >= 40 and all(sum(len(s.pos[c]) for c in s.references) > 300 for s in f.host_split[0])
    return f


def _bam(f):
    dev = FragmentStore.from_bam(f.bam, device=True)
    assert FragmentStore.last_bam_on_device is True
    _same(dev, f.host_bam)


def _plain(f):
    dev = FragmentStore.from_fragments(f.frag, device=True)
    assert FragmentStore.last_frag_on_device is True
    _same(dev, f.host_plain)


def _split(f):
    dev = FragmentStore.split_fragments(f.frag, f.barcodes, f.group_of, GROUPS, device=True)
    assert FragmentStore.last_frag_on_device is True
    assert_same_split(dev, f.host_split)


def _cells(f):
    dev = FragmentStore.discover_cells(f.frag, device=True)
    assert FragmentStore.last_frag_on_device is True
    assert_same_table(dev, f.host_cells)


@pytest.fixture
def small_windows(monkeypatch):
    monkeypatch.setenv("NATAC_BAM_DEV_WINDOW", str(WINDOW))
    monkeypatch.setenv("NATAC_FRAG_DEV_WINDOW", str(WINDOW))


def test_back_to_back_in_one_process(files, small_windows):
    """BAM, plain fragments, split, cells and the BAM again, one behind the other on one context: every result is the host decoder's and
    every run is the device's"""
    for p in (files.bam, files.frag):
        assert len(_window_ends(open(p, "rb").read(), WINDOW)) > 24
    for run in (_bam, _plain, _split, _cells, _bam):
        run(files)


def test_error_in_a_late_window_then_reuse(files, small_windows):
    """a damaged member behind the tenth window: every device entry point raises what its host path raises, and the sound file decoded
    right afterwards is the device's again"""
    f = files
    calls = [(_bam, lambda dev: FragmentStore.from_bam(f.bad_bam, device=dev)),
             (_plain, lambda dev: FragmentStore.from_fragments(f.bad_frag, device=dev)),
             (_split, lambda dev: FragmentStore.split_fragments(f.bad_frag, f.barcodes, f.group_of, GROUPS, device=dev)),
             (_cells, lambda dev: FragmentStore.discover_cells(f.bad_frag, device=dev))]
    for sound, damaged in calls:
        msgs = []
        for dev in (False, True):
            with pytest.raises(Exception) as e:
                damaged(dev)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1] and ("inflate failed" in msgs[0] or "CRC-32 mismatch" in msgs[0]), msgs
        sound(f)
