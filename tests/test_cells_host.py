"""CPU: the cells of a fragment file (natac_frag_cells, csrc/natac_fragfile.hpp: barcode_line and the merge of the slices' tables) against the
package's pure-Python restatement (FragmentStore.discover_cells_python) and against the rule written out once more in tests/cells_ref.py;
and the `pyatac cells` command.  The crafted file is the split's (tests/test_cellgroups_host.py lists what it holds)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from cellgroups_ref import HASHED, LONGEST, TWIN_A, TWIN_B
from cells_ref import assert_same_table, assert_table_equals_ref, cells_ref, crafted, every_barcode
from helpers import bgzf_bytes
from nucleoatac_amd.pyatac.fragments import FragmentStore


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the crafted text in every container and its reference table, computed once"""
    d = tmp_path_factory.mktemp("cells")
    text, listed = crafted()
    paths = {}
    for name, data in (("plain.tsv", text), ("one.tsv.gz", gzip.compress(text)), ("bgzf100.tsv.gz", bgzf_bytes(text, blk=100)),
                       ("bgzf.tsv.gz", bgzf_bytes(text, blk=0xff00))):
        paths[name] = str(d / name)
        open(paths[name], "wb").write(data)
    return dict(text=text, listed=listed, paths=paths, ref=cells_ref(text))


@pytest.mark.parametrize("name", ["plain.tsv", "one.tsv.gz", "bgzf100.tsv.gz", "bgzf.tsv.gz"])
def test_host_python_and_reference_agree_exactly(case, name):
    got = FragmentStore.discover_cells(case["paths"][name], n_threads=1, device=False)
    assert FragmentStore.last_frag_on_device is False
    assert_table_equals_ref(got, case["ref"])
    assert_table_equals_ref(FragmentStore.discover_cells_python(case["paths"][name]), case["ref"])


def test_threads_and_windows_change_nothing(case, monkeypatch):
    ref = case["ref"]
    for name in ("bgzf100.tsv.gz", "plain.tsv"):
        for n_threads in (1, 3, 16):
            assert_table_equals_ref(FragmentStore.discover_cells(case["paths"][name], n_threads=n_threads, device=False), ref)
    size = os.path.getsize(case["paths"]["plain.tsv"])
    assert size / 6000 > 15                            # more than 15 windows of the plain text, fewer bytes still of the compressed files
    monkeypatch.setenv("NATAC_BAM_WINDOW", "6000")
    assert os.path.getsize(case["paths"]["bgzf100.tsv.gz"]) / 6000 > 15
    for name in ("bgzf100.tsv.gz", "one.tsv.gz", "plain.tsv"):
        for n_threads in (1, 3, 16):
            assert_table_equals_ref(FragmentStore.discover_cells(case["paths"][name], n_threads=n_threads, device=False), ref)


def test_the_clauses_the_crafted_text_carries(case):
    text, listed, ref = case["text"], case["listed"], case["ref"]
    cells = dict(zip(ref["barcodes"], ref["n_frag"].tolist()))
    assert cells[TWIN_A] > 0 and cells[TWIN_B] > 0                     # twins that differ in the last byte: two cells
    assert cells[HASHED] > 0                                           # '#' inside a barcode
    assert cells[LONGEST] > 0 and b"Q" * 256 not in cells and b"" not in cells      # 255 bytes: a cell; 256 and none: unassigned
    lines = [x for x in text.split(b"\n") if x and not x.startswith(b"#")]
    fourth = [x.split(b"\t")[3] if x is lines[-1] else x.rstrip(b"\r").split(b"\t")[3] for x in lines if x.rstrip(b"\r")]
    assert ref["n_unassigned"] == sum(1 for b in fourth if not 1 <= len(b) <= 255) > 0
    assert text.endswith(listed[1] + b"\r") and cells[listed[1] + b"\r"] == 1      # the open last line keeps its '\r': a cell of its own
    assert listed[0][:-1] in cells and listed[0] + b"X" in cells and b" " + listed[2] in cells and listed[3].lower() in cells
    # a chromosome that comes back: a cell's lines on both stretches of chr1 count for one cell, and the order is that of the file
    assert ref["barcodes"] == list(dict.fromkeys(fourth_ok for fourth_ok in fourth if 1 <= len(fourth_ok) <= 255))
    first = text.index(b"chr1\t"), text.rindex(b"\nchr3_random\t")
    back = text.index(b"\nchr1\t", text.index(b"\nchr3_random\t"))
    assert first[0] < back < first[1]
    got = FragmentStore.discover_cells(case["paths"]["bgzf.tsv.gz"], device=False)
    assert dict(zip(got.barcodes, got.n_frag.tolist())) == cells and len(got) == len(cells) > 45


def _sizes_file(tmp_path):
    rows = [(0, b"A"), (146, b"A"), (147, b"A"), (293, b"A"), (294, b"A"), (146, b"B"), (293, b"B"), (294, b"C"), (0, b"C")]
    text = b"".join(b"chr1\t%d\t%d\t%s\t3\n" % (1000 + i, 1000 + i + ilen, bc) for i, (ilen, bc) in enumerate(rows))
    path = str(tmp_path / "sizes.tsv")
    open(path, "wb").write(text)
    return path, text


@pytest.mark.parametrize("bounds,want", [((147, 294), dict(A=(5, 2, 2), B=(2, 1, 1), C=(2, 1, 0))),
                                        ((146, 147), dict(A=(5, 1, 1), B=(2, 0, 1), C=(2, 1, 0))),
                                        ((1, 295), dict(A=(5, 1, 4), B=(2, 0, 2), C=(2, 1, 1))),
                                        ((294, 2 ** 31 - 1), dict(A=(5, 4, 1), B=(2, 2, 0), C=(2, 1, 1)))])
def test_size_classes_at_their_edges(tmp_path, bounds, want):
    path, text = _sizes_file(tmp_path)
    ref = cells_ref(text, *bounds)
    assert {b.decode(): (int(f), int(n), int(m)) for b, f, n, m in zip(ref["barcodes"], ref["n_frag"], ref["n_nfr"], ref["n_mono"])} == want
    assert_table_equals_ref(FragmentStore.discover_cells(path, *bounds, device=False), ref)
    assert_table_equals_ref(FragmentStore.discover_cells_python(path, *bounds), ref)


@pytest.mark.parametrize("bounds", [(0, 294), (-1, 5), (147, 147), (294, 147)])
def test_bad_bounds_are_an_error(tmp_path, bounds):
    from nucleoatac_amd._lib import NatacError
    path, _ = _sizes_file(tmp_path)
    with pytest.raises(NatacError, match="nfr_upper < mono_upper"):
        FragmentStore.discover_cells(path, *bounds, device=False)
    with pytest.raises(ValueError):
        FragmentStore.discover_cells_python(path, *bounds)


def test_the_handle_calls_check_their_sizes(tmp_path):
    from nucleoatac_amd import _lib as L
    lib = L.load()
    path, _ = _sizes_file(tmp_path)
    h = C.c_void_p()
    assert lib.natac_frag_cells(path.encode(), 1, 147, 294, C.byref(h)) == 0
    n, nb, nd, nu = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    assert lib.natac_cells_counts(h, C.byref(n), C.byref(nb), C.byref(nd), C.byref(nu)) == 0
    assert (n.value, nb.value, nd.value, nu.value) == (3, 3, 9, 0)
    assert lib.natac_cells_read(h, 2, 3, None, None, None, None, None) == -1 and b"3 cells" in lib.natac_last_error()
    off = np.zeros(4, np.int64)
    assert lib.natac_cells_read(h, 3, 3, None, off.ctypes.data_as(C.c_void_p), None, None, None) == 0 and off.tolist() == [0, 1, 2, 3]
    lib.natac_cells_close(h)
    assert lib.natac_cells_counts(None, None, None, None, None) == -1
    h = C.c_void_p(0xdead)
    assert lib.natac_frag_cells(str(tmp_path / "absent.tsv").encode(), 1, 147, 294, C.byref(h)) == -1 and h.value is None


@pytest.mark.parametrize("line,reason", [(b"chr1\t5\t9", "no barcode field"), (b"chr1\t5\t7x\tAA", "start / end is not a number"),
                                         (b"chr1\t9\t5\tAA", "end before start")])
@pytest.mark.parametrize("n_threads", [1, 5])
def test_malformed_lines_give_the_splits_message(tmp_path, line, reason, n_threads):
    from nucleoatac_amd._lib import NatacError
    good = [b"chr1\t%d\t%d\tAA%d\n" % (i, i + 50, i % 7) for i in range(600)]
    path = str(tmp_path / "bad.tsv.gz")
    open(path, "wb").write(bgzf_bytes(b"# head\n" + b"".join(good[:400]) + line + b"\n" + b"".join(good[400:]), blk=900))
    with pytest.raises(NatacError) as split:
        FragmentStore.split_fragments(path, [b"AA0"], [0], 1, n_threads=n_threads, device=False)
    assert str(split.value).endswith("%s: line 402: %s" % (path, reason))
    with pytest.raises(NatacError) as cells:
        FragmentStore.discover_cells(path, n_threads=n_threads, device=False)
    assert str(cells.value) == str(split.value)
    with pytest.raises(ValueError, match="line 402: " + reason.replace("/", ".")):
        FragmentStore.discover_cells_python(path)


def _command_file(tmp_path):
    """five cells: BIG (30 lines: 20 nfr, 10 mono), MID (12: 4 nfr, 8 mono), NONFR (12: all mono), SMALL (3), LONG (12 lines of 500 bases)"""
    rows = [(b"BIG-1", 100)] * 20 + [(b"BIG-1", 200)] * 10 + [(b"MID-1", 100)] * 4 + [(b"MID-1", 200)] * 8 + [(b"NONFR-1", 200)] * 12
    rows += [(b"SMALL-1", 100)] * 3 + [(b"LONG-1", 500)] * 12 + [(b"", 100)] * 2
    order = np.random.default_rng(0).permutation(len(rows))
    text = b"# id=x\n" + b"".join(b"chr%d\t%d\t%d\t%s\t1\n" % (1 + i % 2, 10 * i, 10 * i + rows[k][1], rows[k][0]) for i, k in enumerate(order.tolist()))
    path = str(tmp_path / "sc.tsv.gz")
    open(path, "wb").write(bgzf_bytes(text, blk=500))
    return path, text


def test_the_command_writes_its_three_files(tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac.cellgroups import read_groups
    from nucleoatac_amd.pyatac.cli import main
    path, text = _command_file(tmp_path)
    monkeypatch.chdir(tmp_path)
    ref = cells_ref(text)
    assert main(["cells", "--fragments", path, "--min_fragments", "12"]) == 0
    order = [b for b in ref["barcodes"]]
    passing = [b for b in order if b != b"SMALL-1"]
    assert open("sc.cells.tsv", "rb").read() == b"".join(b + b"\n" for b in passing)
    assert read_groups("sc.cells.tsv").barcodes == passing             # what `split --groups` and `cellcounts --cells` read
    qc = open("sc.cells.qc.tsv", "rb").read().split(b"\n")
    assert qc[0] == b"#barcode\tfragments\tnfr\tmono\tnucleosome_signal\tpass" and qc[-1] == b"" and len(qc) == 7
    rows = {r.split(b"\t")[0]: r.split(b"\t")[1:] for r in qc[1:-1]}
    assert [r.split(b"\t")[0] for r in qc[1:-1]] == order
    assert rows[b"BIG-1"] == [b"30", b"20", b"10", b"0.5000", b"1"] and rows[b"MID-1"] == [b"12", b"4", b"8", b"2.0000", b"1"]
    assert rows[b"NONFR-1"] == [b"12", b"0", b"12", b"NA", b"1"] and rows[b"SMALL-1"] == [b"3", b"3", b"0", b"0.0000", b"0"]
    assert rows[b"LONG-1"] == [b"12", b"0", b"0", b"NA", b"1"]
    assert open("sc.cells.txt").read() == "data_lines\t71\nunassigned_lines\t2\nbarcodes\t5\npassing\t4\nfragments_in_passing\t66\n"
    # the signal filter: NONFR and LONG have no nucleosome-free fragment and fail it; MID is above 1
    assert main(["cells", "--fragments", path, "--min_fragments", "3", "--max_nucleosome_signal", "1", "--out", "strict"]) == 0
    assert open("strict.cells.tsv", "rb").read() == b"".join(b + b"\n" for b in order if b in (b"BIG-1", b"SMALL-1"))
    assert main(["cells", "--fragments", path, "--min_fragments", "3", "--max_nucleosome_signal", "2", "--out", "at2"]) == 0
    assert set(open("at2.cells.tsv", "rb").read().split()) == {b"BIG-1", b"SMALL-1", b"MID-1"}
    # other bounds: with nfr_upper 201 every 200-base fragment is nucleosome-free
    assert main(["cells", "--fragments", path, "--min_fragments", "12", "--nfr_upper", "201", "--mono_upper", "501", "--out", "wide"]) == 0
    wide = {r.split(b"\t")[0]: r.split(b"\t")[1:] for r in open("wide.cells.qc.tsv", "rb").read().split(b"\n")[1:-1]}
    assert wide[b"NONFR-1"][:3] == [b"12", b"12", b"0"] and wide[b"LONG-1"][:4] == [b"12", b"0", b"12", b"NA"]
    capsys.readouterr()


def test_errors_of_the_command_leave_nothing_behind(tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac.cli import main
    path, _ = _command_file(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    monkeypatch.chdir(out)
    assert main(["cells", "--fragments", path]) == 1                   # the default of 1,000 fragments: no cell passes
    err = capsys.readouterr().err
    assert err.startswith("pyatac cells: ") and "no cell passes" in err and "30 fragments" in err
    assert main(["cells", "--fragments", str(tmp_path / "absent.tsv.gz")]) == 1
    assert capsys.readouterr().err == "pyatac cells: %s: no such file\n" % (tmp_path / "absent.tsv.gz")
    bad = str(tmp_path / "bad.tsv")
    open(bad, "wb").write(b"chr1\t1\t50\tAA\nchr1\t5\t9\n")
    assert main(["cells", "--fragments", bad, "--min_fragments", "1"]) == 1
    err = capsys.readouterr().err
    assert err.startswith("pyatac cells: ") and err.endswith("%s: line 2: no barcode field\n" % bad)
    assert main(["cells", "--fragments", path, "--min_fragments", "1", "--nfr_upper", "300"]) == 1
    assert "nfr_upper < mono_upper" in capsys.readouterr().err
    assert os.listdir(str(out)) == []


def test_every_barcode_of_a_clean_file_is_a_cell(tmp_path):
    text, _ = crafted(seed=3, n=1200)
    keep = [x for x in text.split(b"\n")[:-1] if x.startswith(b"#") or not x.rstrip(b"\r") or 1 <= len(x.rstrip(b"\r").split(b"\t")[3]) <= 255]
    text = b"\n".join(keep) + b"\n"
    path = str(tmp_path / "all.tsv.gz")
    open(path, "wb").write(bgzf_bytes(text, blk=900))
    got = FragmentStore.discover_cells(path, device=False)
    assert got.barcodes == every_barcode(text) and got.n_unassigned == 0
    # the table feeds the split: one group of every discovered cell is the whole file
    stores, bc_count, n_unassigned = FragmentStore.split_fragments(path, got.barcodes, [0] * len(got), 1, device=False)
    assert n_unassigned == 0 and np.array_equal(bc_count, got.n_frag)
    assert_same_table(got, FragmentStore.discover_cells(path, n_threads=7, device=False))
