"""CPU: a fragment file split by cell barcode (natac_frag_split, csrc/natac_fragfile.hpp: split_line) against the package's pure-Python
restatement (FragmentStore.split_fragments_python) and against the rule written out once more in tests/cellgroups_ref.py; the barcode
table reader (pyatac/cellgroups.py: read_groups) and the `pyatac split` command.

The crafted file (cellgroups_ref.crafted) holds 4 and 5 columns; CRLF lines, one kind directly behind a 4-field barcode; '#' headers and
empty lines inside; duplicate lines; an unsorted stretch with equal starts and different ends in one group; a chromosome that comes
back; a chromosome on which only unassigned lines lie; an open last line ending in '\\r'.  Its barcodes: listed; unlisted of the same
length; empty; 256 bytes long; a strict prefix of a listed one; a listed one plus one byte; two listed ones that differ in the last
byte only; one containing '#'."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from cellgroups_ref import (HASHED, LONGEST, NEVER, TWIN_A, TWIN_B, assert_same_split, assert_split_equals_ref, crafted, every_barcode,
                            split_ref)
from helpers import bgzf_bytes
from nucleoatac_amd.pyatac.fragments import FragmentStore

MAX_GROUPS = 255


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the crafted text in every container, and the reference split for G = 1, 2 and the most groups, computed once"""
    d = tmp_path_factory.mktemp("cells")
    text, listed = crafted()
    paths = {}
    for name, data in (("plain.tsv", text), ("one.tsv.gz", gzip.compress(text)), ("bgzf.tsv.gz", bgzf_bytes(text, blk=700))):
        paths[name] = str(d / name)
        open(paths[name], "wb").write(data)
    tables = {1: [0] * len(listed), MAX_GROUPS: [k % MAX_GROUPS for k in range(len(listed))],
              2: [1 if b == NEVER else 0 for b in listed]}            # G = 2: nobody's line belongs to group 1
    refs = {G: split_ref(text, listed, tables[G], G) for G in tables}
    return dict(text=text, listed=listed, paths=paths, tables=tables, refs=refs)


def test_the_crafted_file_holds_what_the_docstring_says(case):
    text, listed, ref = case["text"], case["listed"], case["refs"][1]
    lines = text.split(b"\n")
    data = [x for x in lines if x.rstrip(b"\r") and not x.startswith(b"#")]
    assert 3000 < len(lines) < 5000 and ref["n_data"] == len(data)
    assert {len(x.rstrip(b"\r").split(b"\t")) for x in data[:-1]} == {4, 5}
    assert any(x.endswith(b"\r") and len(x.split(b"\t")) == 4 for x in data[:-1]) and lines[-1].endswith(b"-1\r")
    assert any(a == b for a, b in zip(data, data[1:]))
    assert any(x.startswith(b"#") for x in lines[10:]) and b"" in lines[10:-1]
    fourth = {x.rstrip(b"\r").split(b"\t")[3] for x in data[:-1]}
    assert {b"", b"Q" * 256, listed[0][:-1], listed[0] + b"X", TWIN_A, TWIN_B, HASHED, LONGEST} <= fourth and NEVER not in fourth
    assert any(len(b) == len(listed[0]) and b not in listed for b in fourth)
    assert ref["names"] == ["chr1", "chr2", "chrOnlyUnassigned", "chr3_random"]
    assert len(ref["pos"][0]["chrOnlyUnassigned"]) == 0 and ref["lengths"][2] > 0
    # the stability stretch: starts 296 and 496 of one cell, the ends in file order
    p, t = ref["pos"][0]["chr2"], ref["tlen"][0]["chr2"]
    assert t[p == 496].tolist() == [408, 208, 308, 108, 158] and t[p == 296].tolist() == [18, 13]
    k = listed.index(TWIN_A)
    assert ref["bc_count"][k] > 0 and ref["bc_count"][k + 1] > 0 and ref["bc_count"][listed.index(NEVER)] == 0
    assert 0 < ref["n_unassigned"] < ref["n_data"]


@pytest.mark.parametrize("G", [1, 2, MAX_GROUPS])
def test_host_python_and_reference_agree_exactly(case, G):
    path, listed, table = case["paths"]["bgzf.tsv.gz"], case["listed"], case["tables"][G]
    assert_split_equals_ref(FragmentStore.split_fragments_python(path, listed, table, G), case["refs"][G])
    got = FragmentStore.split_fragments(path, listed, table, G, n_threads=1, device=False)
    assert FragmentStore.last_frag_on_device is False
    assert_split_equals_ref(got, case["refs"][G])
    if G == 2:
        assert sum(len(got[0][1].pos[c]) for c in got[0][1].references) == 0 and got[0][1].references == got[0][0].references


@pytest.mark.parametrize("G", [2, MAX_GROUPS])
def test_threads_windows_containers_and_short_hashes_change_nothing(case, monkeypatch, G):
    listed, table, ref = case["listed"], case["tables"][G], case["refs"][G]
    for name in ("bgzf.tsv.gz", "one.tsv.gz", "plain.tsv"):
        for n_threads in (1, 3, 16):
            assert_split_equals_ref(FragmentStore.split_fragments(case["paths"][name], listed, table, G, n_threads=n_threads, device=False), ref)
    with monkeypatch.context() as m:
        m.setenv("NATAC_BAM_WINDOW", "4096")
        for name in ("bgzf.tsv.gz", "one.tsv.gz", "plain.tsv"):
            assert_split_equals_ref(FragmentStore.split_fragments(case["paths"][name], listed, table, G, n_threads=3, device=False), ref)
    monkeypatch.setenv("NATAC_SPLIT_HASH_BITS", "3")                   # 8 hash values for ~35 barcodes: chains of equal hashes
    assert_split_equals_ref(FragmentStore.split_fragments(case["paths"]["bgzf.tsv.gz"], listed, table, G, n_threads=3, device=False), ref)


def test_one_group_of_every_barcode_is_the_plain_decode(tmp_path):
    text, _ = crafted(seed=3, n=1200)
    keep = [x for x in text.split(b"\n")[:-1] if x.startswith(b"#") or not x.rstrip(b"\r")
            or 1 <= len(x.rstrip(b"\r").split(b"\t")[3]) <= 255]
    text = b"\n".join(keep) + b"\n"
    path = str(tmp_path / "all.tsv.gz")
    open(path, "wb").write(bgzf_bytes(text, blk=900))
    everyone = every_barcode(text)
    assert len(everyone) > 40
    plain = FragmentStore.from_fragments(path, device=False)
    stores, bc_count, n_unassigned = FragmentStore.split_fragments(path, everyone, [0] * len(everyone), 1, device=False)
    one = FragmentStore.from_fragments(path, device=False, barcodes=everyone)
    n = sum(len(plain.pos[c]) for c in plain.references)
    assert n_unassigned == 0 and int(bc_count.sum()) == n > 1000
    for st in (stores[0], one):
        assert st.references == plain.references and st.lengths == plain.lengths
        for c in plain.references:
            assert np.array_equal(st.pos[c], plain.pos[c]) and np.array_equal(st.tlen[c], plain.tlen[c])
    # a whitelist: the listed cells' lines, the others unassigned; sizes + unassigned = the file's data lines over any table
    some = everyone[::3]
    stores, bc_count, n_unassigned = FragmentStore.split_fragments(path, some, [k % 7 for k in range(len(some))], 7, device=False)
    assert sum(len(st.pos[c]) for st in stores for c in st.references) + n_unassigned == n and 0 < n_unassigned < n
    assert_same_split((stores, bc_count, n_unassigned), FragmentStore.split_fragments_python(path, some, [k % 7 for k in range(len(some))], 7))


HEAD = b"# header\n\n#more\nchr1\t1\t2\tAA\n\r\n"      # five lines, one of them data: a bad line behind it is line 6
BAD = [(b"chr1\t5\t9", "no barcode field"),                            # the new reason: three good fields and nothing else
       (b"chr1\t5\t9\r", "start / end is not a number"),               # (an open last line keeps its '\r'; with '\n' it is the line above)
       (b"chr1\t5", "fewer than three tab-separated fields"),          # every older reason keeps precedence and its text
       (b"\t5\t9", "empty chromosome name"),
       (b"c" * 256 + b"\t5\t9", "chromosome name longer than 255 bytes"),
       (b"chr1\t+5\t9", "start / end is not a number"),
       (b"chr1\t5\t2147483648", "start / end out of range (more than 2147483647)"),
       (b"chr1\t9\t5", "end before start"),
       (b"chr1\t9\t5\tAA", "end before start")]


def _split_raw(path, barcodes, group_of, n_groups, n_threads=1):
    """natac_frag_split called directly -> (return code, message, handles as a list of int or None)"""
    from nucleoatac_amd import _lib as L
    lib = L.load()
    off = np.zeros(len(barcodes) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in barcodes], out=off[1:])
    blob = np.frombuffer(b"".join(barcodes) + b"\0", dtype=np.uint8)
    grp = np.asarray(group_of, dtype=np.int32)
    handles = (C.c_void_p * max(n_groups, 1))(*([0xdead] * max(n_groups, 1)))          # stale values: an error must clear them
    rc = lib.natac_frag_split(path.encode(), n_threads, len(barcodes), blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                              grp.ctypes.data_as(C.c_void_p), n_groups, C.cast(handles, C.c_void_p), None, None)
    return rc, lib.natac_last_error().decode(), list(handles), lib


@pytest.mark.parametrize("k", range(len(BAD)))
def test_malformed_lines_keep_their_order_and_texts(tmp_path, k):
    line, reason = BAD[k]
    path = str(tmp_path / "bad.tsv")
    tails = (b"\nchr1\t7\t8\tAA\n", b"") if k != 1 else (b"",)
    for tail in tails:
        open(path, "wb").write(HEAD + line + tail)
        want = "%s: line 6: %s" % (path, reason)
        with pytest.raises(ValueError) as py:
            FragmentStore.split_fragments_python(path, [b"AA"], [0], 1)
        assert str(py.value) == want
        for n_threads in (1, 16):
            rc, msg, handles, _ = _split_raw(path, [b"AA", b"CC"], [0, 2], 3, n_threads)
            assert rc == -1 and msg == want and handles == [None, None, None]


def test_first_malformed_line_wins_whatever_the_slices(tmp_path):
    good = [b"chr1\t%d\t%d\tAA\n" % (i, i + 50) for i in range(4000)]
    path = str(tmp_path / "bad.tsv.gz")
    open(path, "wb").write(bgzf_bytes(b"".join(good[:2000] + [b"chr1\t5\t9\n"] + good[2000:] + [b"chr1\t9\t5\n"]), blk=700))
    for n_threads in (1, 3, 16):
        with pytest.raises(Exception, match=r"bad\.tsv\.gz: line 2001: no barcode field"):
            FragmentStore.split_fragments(path, [b"AA"], [0], 1, n_threads=n_threads, device=False)


def test_bad_tables_are_argument_errors(tmp_path):
    path = str(tmp_path / "f.tsv")
    open(path, "wb").write(b"chr1\t5\t9\tAA\n")
    rc, msg, handles, lib = _split_raw(path, [b"AA", b"CC", b"AA"], [0, 1, 1], 2)
    assert rc == -1 and "barcodes 0 and 2 are the same" in msg and handles == [None, None]          # NATAC_E_ARG
    for barcodes, group_of, G, what in (([b"AA", b""], [0, 0], 1, "barcode 1 is not 1-255 bytes long"),
                                         ([b"A" * 256], [0], 1, "barcode 0 is not 1-255 bytes long"),
                                         ([b"AA"], [1], 1, "barcode 0: group out of range"),
                                         ([b"AA"], [0], MAX_GROUPS + 1, "n_groups must be in [1, 255]"),
                                         ([b"AA"], [0], 0, "n_groups must be in [1, 255]")):
        rc, msg, handles, _ = _split_raw(path, barcodes, group_of, G)
        assert rc == -1 and what in msg, (what, msg)
    rc, msg, handles, lib = _split_raw(path, [b"AA", b"A"], [0, 1], 2)
    assert rc == 0 and all(handles)
    kept = []
    for h in handles:
        n = C.c_int64(-1)
        r = C.c_int64(-1)
        assert lib.natac_bam_counts(C.c_void_p(h), None, C.byref(r), C.byref(n)) == 0
        kept.append((r.value, n.value))
        lib.natac_bam_close(C.c_void_p(h))
    assert kept == [(1, 1), (1, 0)]                       # n_records = the file's data lines, n_kept = the group's


# ---- the barcode table --------------------------------------------------------------------------------------------------------------
def _table(tmp_path, data, name="groups.tsv"):
    path = str(tmp_path / name)
    open(path, "wb").write(data)
    return path


def test_read_groups(tmp_path):
    from nucleoatac_amd.pyatac.cellgroups import read_groups
    g = read_groups(_table(tmp_path, b"# made by hand\nbarcode\tcluster\n\nAAAC-1\tT.cell\nAAAG-1\tB_cell\r\nAAAC-1\tT.cell\textra\nAAAT-1\tT.cell\n"),
                    header=True)
    assert g.names == ["T.cell", "B_cell"] and g.barcodes == [b"AAAC-1", b"AAAG-1", b"AAAT-1"] and g.group_of == [0, 1, 0]
    assert g.listed() == [2, 1]
    g = read_groups(_table(tmp_path, b"AAAC-1\nAAAG-1\n"))
    assert g.names == ["selected"] and g.group_of == [0, 0]
    g = read_groups(_table(tmp_path, gzip.compress(b"AAAC-1\tx\n"), "groups.tsv.gz"))
    assert g.names == ["x"] and g.barcodes == [b"AAAC-1"]


@pytest.mark.parametrize("data,header,message", [
    (b"AA\tx\nCC\ty\n#c\nAA\ty\n", False, "line 4: barcode AA is in group y here and in group x on line 1"),
    (b"AA\tx\n\tx\n", False, "line 2: empty barcode"),
    (b"h\th\n" + b"A" * 256 + b"\tx\n", True, "line 2: barcode longer than 255 bytes"),
    (b"AA\tx\nCC\tx y\n", False, "line 2: group name 'x y' does not match"),
    (b"AA\tx\nCC\t\n", False, "line 2: group name '' does not match"),
    (b"AA\t" + b"g" * 65 + b"\n", False, "line 1: group name"),
    (b"AA\ta/b\n", False, "line 1: group name 'a/b' does not match"),
    (b"".join(b"B%d\tg%d\n" % (k, k) for k in range(256)), False, "line 256: more than 255 groups"),
    (b"# nothing\n\n", False, "no barcode in the table"),
    (b"barcode\tgroup\n", True, "no barcode in the table"),
])
def test_read_groups_errors_name_the_line(tmp_path, data, header, message):
    from nucleoatac_amd.pyatac.cellgroups import CellGroupError, read_groups
    path = _table(tmp_path, data)
    with pytest.raises(CellGroupError) as e:
        read_groups(path, header=header)
    assert str(e.value).startswith(path + ": line ") and message in str(e.value)


# ---- pyatac split -------------------------------------------------------------------------------------------------------------------
def test_split_parser_defaults():
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    a = pyatac_parser().parse_args(["split", "--fragments", "f.tsv.gz", "--groups", "g.tsv"])
    assert vars(a) == dict(call="split", fragments="f.tsv.gz", groups="g.tsv", header=False, out=None, format="npz")
    a = pyatac_parser().parse_args(["split", "--fragments", "f", "--groups", "g", "--header", "--out", "o", "--format", "fragments"])
    assert (a.header, a.out, a.format) == (True, "o", "fragments")
    with pytest.raises(SystemExit):
        pyatac_parser().parse_args(["split", "--fragments", "f"])


def _same_store(a, b):
    assert a.references == b.references and list(a.lengths) == list(b.lengths)
    for c in a.references:
        assert np.array_equal(a.pos[c], b.pos[c]) and np.array_equal(a.tlen[c], b.tlen[c]), c


def test_split_command_writes_every_group(case, tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac.cli import main
    listed = [b for b in case["listed"] if b"#" not in b]                # ('#' starts a comment line in the table)
    names = ["A", "B.2", "c-3"]
    rows = [b"barcode\tcluster\n"] + [b"%s\t%s\n" % (b, names[k % 3].encode()) for k, b in enumerate(listed)]
    table = _table(tmp_path, b"".join(rows))
    group_of = [k % 3 for k in range(len(listed))]
    frag = case["paths"]["bgzf.tsv.gz"]
    want = FragmentStore.split_fragments_python(frag, listed, group_of, 3)
    monkeypatch.chdir(tmp_path)
    assert main(["split", "--fragments", frag, "--groups", table, "--header"]) == 0
    assert sorted(os.listdir(".")) == ["bgzf.A.npz", "bgzf.B.2.npz", "bgzf.c-3.npz", "bgzf.split.txt", "groups.tsv"]
    for g, name in enumerate(names):
        _same_store(FragmentStore.from_npz("bgzf.%s.npz" % name), want[0][g])
    rows = [x.split("\t") for x in open("bgzf.split.txt").read().splitlines()]
    assert rows[0] == ["group", "barcodes_listed", "barcodes_seen", "fragments"] and rows[-1] == ["unassigned", str(want[2])]
    for g, name in enumerate(names):
        mine = [k for k in range(len(listed)) if group_of[k] == g]
        assert rows[1 + g] == [name, str(len(mine)), str(sum(1 for k in mine if want[1][k] > 0)),
                               str(sum(len(want[0][g].pos[c]) for c in want[0][g].references))]
    assert any(int(r[1]) > int(r[2]) for r in rows[1:-1])                # NEVER is listed and never seen
    out = str(tmp_path / "sub" / "cells")
    os.mkdir(str(tmp_path / "sub"))
    assert main(["split", "--fragments", frag, "--groups", table, "--header", "--out", out, "--format", "fragments"]) == 0
    assert sorted(os.listdir(str(tmp_path / "sub"))) == sorted(["cells.%s.tsv.gz%s" % (n, t) for n in names for t in ("", ".tbi")] + ["cells.split.txt"])
    for g, name in enumerate(names):
        back = FragmentStore.from_fragments("%s.%s.tsv.gz" % (out, name), device=False)
        full = want[0][g]
        assert back.references == [c for c in full.references if len(full.pos[c])]       # three columns: an empty chromosome leaves no line
        for c in back.references:
            assert np.array_equal(back.pos[c], full.pos[c]) and np.array_equal(back.tlen[c], full.tlen[c]), c
        assert len(open("%s.%s.tsv.gz" % (out, name), "rb").read()) > 100 and b"\t" in gzip.open("%s.%s.tsv.gz" % (out, name)).readline()
        assert gzip.open("%s.%s.tsv.gz" % (out, name)).readline().count(b"\t") == 2
    capsys.readouterr()


def test_split_command_writes_nothing_on_error(case, tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac.cli import main
    monkeypatch.chdir(tmp_path)
    good = _table(tmp_path, b"AAAC-1\n")
    bad = _table(tmp_path, b"AA\tx\nAA\ty\n", "bad.tsv")
    three = str(tmp_path / "three.tsv")
    open(three, "wb").write(b"chr1\t5\t9\tAAAC-1\nchr1\t5\t9\n")
    before = sorted(os.listdir("."))
    for argv, message in ((["--fragments", case["paths"]["plain.tsv"], "--groups", bad], "bad.tsv: line 2: barcode AA is in group y"),
                          (["--fragments", three, "--groups", good], "three.tsv: line 2: no barcode field"),
                          (["--fragments", str(tmp_path / "missing.tsv"), "--groups", good], "missing.tsv"),):
        assert main(["split"] + argv) == 1
        err = capsys.readouterr().err
        assert err.startswith("pyatac split: ") and message in err
        assert sorted(os.listdir(".")) == before
