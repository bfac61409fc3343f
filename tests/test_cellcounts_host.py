"""CPU: the cell-tagged read of a fragment file (natac_frag_open_cells / natac_bam_ref_cells, csrc/natac_fragfile.hpp: the one-group split
that keeps every kept record's barcode index) against the package's pure-Python restatement (FragmentStore.cells_fragments_python), against
the records read from the text in this file, and against the one-group split it shares its code with; the restatement of the count
matrix (tests/cellcounts_ref.py) against sites_ref.region_counts_brute; the parser, the default output name and the MatrixMarket text of
`pyatac cellcounts`.

The crafted file (cellcounts_ref.crafted_cells): three chromosomes with records, chr1 coming back; 40 cell barcodes of which 30 are listed; a
10x '#' header; CRLF lines; duplicate lines; a line with an empty barcode, one with a 256-byte barcode, one with end == start; written as
BGZF, plain gzip and text."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

from cellcounts_ref import cell_counts_brute, crafted_cells, row_sums
from cellgroups_ref import TWIN_A
from helpers import bgzf_bytes
from nucleoatac_amd.pyatac.fragments import FragmentStore
from sites_ref import region_counts_brute


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("cellcounts")
    text, barcodes = crafted_cells()
    paths = {}
    for name, data in (("plain.tsv", text), ("one.tsv.gz", gzip.compress(text)), ("bgzf.tsv.gz", bgzf_bytes(text, blk=700))):
        paths[name] = str(d / name)
        open(paths[name], "wb").write(data)
    want = FragmentStore.cells_fragments_python(paths["plain.tsv"], barcodes)
    return dict(text=text, barcodes=barcodes, paths=paths, want=want)


def _records_from_text(text, barcodes):
    """per chromosome the (pos, tlen, cell) of the listed lines, sorted by pos with ties in file order; names; data lines; unassigned"""
    lines = text.split(b"\n")
    lines = [x[:-1] if x.endswith(b"\r") else x for x in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    index = {b: k for k, b in enumerate(barcodes)}
    recs, n_data, n_un = {}, 0, 0
    for x in lines:
        if not x or x.startswith(b"#"):
            continue
        f = x.split(b"\t")
        n_data += 1
        recs.setdefault(f[0].decode(), [])
        k = index.get(f[3])
        if k is None:
            n_un += 1
        else:
            recs[f[0].decode()].append((int(f[1]) - 4, int(f[2]) - int(f[1]) + 8, k))
    return {c: sorted(r, key=lambda t: t[0]) for c, r in recs.items()}, list(recs), n_data, n_un


def _assert_same_tagged(got, want):
    (a, ca, ua), (b, cb, ub) = got, want
    assert a.references == b.references and list(a.lengths) == list(b.lengths)
    for c in a.references:
        assert a.cell[c].dtype == np.int32 and a.pos[c].dtype == np.int64
        assert np.array_equal(a.pos[c], b.pos[c]) and np.array_equal(a.tlen[c], b.tlen[c]) and np.array_equal(a.cell[c], b.cell[c]), c
    assert np.array_equal(ca, cb) and ua == ub


def test_the_crafted_file_holds_what_the_docstring_says(case):
    text, barcodes = case["text"], case["barcodes"]
    lines = text.split(b"\n")
    data = [x.rstrip(b"\r") for x in lines if x.rstrip(b"\r") and not x.startswith(b"#")]
    fourth = {x.split(b"\t")[3] for x in data[:-1]}
    assert 3000 < len(lines) < 5000 and lines[0].startswith(b"#") and len(barcodes) == 30
    assert b"" in fourth and b"Q" * 256 in fourth and len({b for b in fourth if re.fullmatch(rb"[ACGT]{16}-1", b)} - {TWIN_A}) == 40
    assert sum(1 for x in lines if x.endswith(b"\r")) > 1 and any(a == b for a, b in zip(data, data[1:]))
    assert any(x.split(b"\t")[1] == x.split(b"\t")[2] for x in data)
    store, bc_count, n_un = case["want"]
    assert store.references == ["chr1", "chr2", "chrOnlyUnassigned", "chr3_random"]
    assert [len(store.pos[c]) > 0 for c in store.references] == [True, True, False, True] and n_un > 0 and np.count_nonzero(bc_count) == 30
    first = [c for c in (x.split(b"\t")[0] for x in data)]
    assert first.index(b"chr2") < len(first) - 1 - first[::-1].index(b"chr1")          # chr1 comes back behind chr2


def test_python_restatement_equals_the_records_of_the_text(case):
    recs, names, n_data, n_un = _records_from_text(case["text"], case["barcodes"])
    store, bc_count, n_unassigned = case["want"]
    assert store.references == names and n_unassigned == n_un and int(bc_count.sum()) + n_un == n_data
    for c in names:
        assert store.pos[c].tolist() == [r[0] for r in recs[c]] and store.tlen[c].tolist() == [r[1] for r in recs[c]]
        assert store.cell[c].tolist() == [r[2] for r in recs[c]]
        assert np.array_equal(np.bincount(store.cell[c], minlength=30), np.bincount([r[2] for r in recs[c]], minlength=30))
    assert np.array_equal(bc_count, sum(np.bincount(store.cell[c], minlength=30) for c in names))
    p = store.pos["chr2"]
    assert np.any(p[1:] == p[:-1])                       # ties: their cells are in file order by the comparison above


@pytest.mark.parametrize("name", ["bgzf.tsv.gz", "one.tsv.gz", "plain.tsv"])
def test_native_read_equals_python_for_any_threads_and_window(case, monkeypatch, name):
    path, barcodes = case["paths"][name], case["barcodes"]
    for n_threads in (1, 7):
        _assert_same_tagged(FragmentStore.from_fragments_cells(path, barcodes, n_threads=n_threads), case["want"])
    monkeypatch.setenv("NATAC_BAM_WINDOW", "300")
    for n_threads in (1, 7):
        _assert_same_tagged(FragmentStore.from_fragments_cells(path, barcodes, n_threads=n_threads), case["want"])


def test_counts_and_records_equal_the_one_group_split(case):
    path, barcodes = case["paths"]["bgzf.tsv.gz"], case["barcodes"]
    got, bc_count, n_un = FragmentStore.from_fragments_cells(path, barcodes)
    stores, bc2, un2 = FragmentStore.split_fragments(path, barcodes, [0] * len(barcodes), 1, device=False)
    assert np.array_equal(bc_count, bc2) and n_un == un2
    plain = FragmentStore.from_fragments(path, device=False, barcodes=barcodes)
    for st in (stores[0], plain):
        assert st.references == got.references and list(st.lengths) == list(got.lengths) and st.cell is None
        for c in st.references:
            assert np.array_equal(st.pos[c], got.pos[c]) and np.array_equal(st.tlen[c], got.tlen[c])


def test_tagged_stores_stay_out_of_the_cache_and_plain_npz_files_are_unchanged(case, tmp_path):
    from nucleoatac_amd.pyatac import fragments as F
    path = case["paths"]["plain.tsv"]
    F._CACHE.pop(path, None)
    tagged = FragmentStore.from_fragments_cells(path, case["barcodes"])
    assert path not in F._CACHE and path not in F._PENDING
    tagged[0].save_npz(str(tmp_path / "tagged.npz"))                 # a tagged store keeps its cells through an .npz
    back = FragmentStore.from_npz(str(tmp_path / "tagged.npz"))
    _assert_same_tagged((back, tagged[1], tagged[2]), tagged)
    plain = FragmentStore.from_fragments(path, device=False)
    plain.save_npz(str(tmp_path / "plain.npz"))
    keys = set(np.load(str(tmp_path / "plain.npz")).files)
    assert keys == {"chrom_names", "chrom_lengths"} | {k + c for k in ("pos_", "tlen_") for c in plain.references}
    assert FragmentStore.from_npz(str(tmp_path / "plain.npz")).cell is None


HEAD = b"# header\n\n#more\nchr1\t1\t2\tAA\n\r\n"      # five lines, one of them data: a bad line behind it is line 6
BAD = [(b"chr1\t5\t9", "no barcode field"),
       (b"chr1\t5", "fewer than three tab-separated fields"),
       (b"\t5\t9", "empty chromosome name"),
       (b"c" * 256 + b"\t5\t9", "chromosome name longer than 255 bytes"),
       (b"chr1\t+5\t9", "start / end is not a number"),
       (b"chr1\t5\t2147483648", "start / end out of range (more than 2147483647)"),
       (b"chr1\t9\t5\tAA", "end before start")]


def _table(barcodes):
    off = np.zeros(len(barcodes) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in barcodes], out=off[1:])
    blob = np.frombuffer(b"".join(barcodes) + b"\0", dtype=np.uint8)
    return len(barcodes), blob, off


def _open_cells_raw(path, barcodes, n_threads=1):
    """natac_frag_open_cells called directly -> (return code, message, handle or None, lib)"""
    from nucleoatac_amd import _lib as L
    lib = L.load()
    n, blob, off = _table(barcodes)
    h = C.c_void_p(0xdead)                               # a stale value: an error must clear it
    rc = lib.natac_frag_open_cells(path.encode(), n_threads, n, blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), C.byref(h),
                                   None, None)
    return rc, lib.natac_last_error().decode(), h.value, lib


def _split_message(path, barcodes, n_threads=1):
    from nucleoatac_amd import _lib as L
    lib = L.load()
    n, blob, off = _table(barcodes)
    grp = np.zeros(max(n, 1), dtype=np.int32)
    handles = (C.c_void_p * 1)()
    rc = lib.natac_frag_split(path.encode(), n_threads, n, blob.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                              grp.ctypes.data_as(C.c_void_p), 1, C.cast(handles, C.c_void_p), None, None)
    msg = lib.natac_last_error().decode()
    if rc == 0:
        lib.natac_bam_close(C.c_void_p(handles[0]))
    return rc, msg


@pytest.mark.parametrize("k", range(len(BAD)))
def test_malformed_lines_give_the_splits_messages(tmp_path, k):
    line, reason = BAD[k]
    path = str(tmp_path / "bad.tsv")
    for tail in (b"\nchr1\t7\t8\tAA\n", b""):
        open(path, "wb").write(HEAD + line + tail)
        want = "%s: line 6: %s" % (path, reason)
        with pytest.raises(ValueError) as py:
            FragmentStore.cells_fragments_python(path, [b"AA"])
        assert str(py.value) == want
        for n_threads in (1, 7):
            rc, msg, h, _ = _open_cells_raw(path, [b"AA", b"CC"], n_threads)
            assert (rc, msg, h) == (-1, want, None)
            assert _split_message(path, [b"AA", b"CC"], n_threads) == (-1, want)


def test_bad_tables_give_the_splits_errors_and_plain_handles_hold_no_cells(tmp_path):
    path = str(tmp_path / "f.tsv")
    open(path, "wb").write(b"chr1\t5\t9\tAA\nchr1\t6\t9\tCC\nchr1\t7\t9\tGG\n")
    for barcodes, what in (([b"AA", b"CC", b"AA"], "barcodes 0 and 2 are the same"), ([b"AA", b""], "barcode 1 is not 1-255 bytes long"),
                           ([b"A" * 256], "barcode 0 is not 1-255 bytes long")):
        rc, msg, h, _ = _open_cells_raw(path, barcodes)
        rc2, msg2 = _split_message(path, barcodes)
        assert (rc, h) == (-1, None) and rc2 == -1 and what in msg and msg == msg2
    rc, msg, h, lib = _open_cells_raw(path, [])
    assert (rc, h) == (-1, None) and "n_barcodes must be in [1, 8388608]" in msg
    rc, msg, h, lib = _open_cells_raw(path, [b"CC", b"AA"])
    assert rc == 0 and h
    cell = np.full(2, -7, np.int32)
    n_rec, n_kept = C.c_int64(-1), C.c_int64(-1)
    assert lib.natac_bam_counts(C.c_void_p(h), None, C.byref(n_rec), C.byref(n_kept)) == 0 and (n_rec.value, n_kept.value) == (3, 2)
    assert lib.natac_bam_ref_cells(C.c_void_p(h), 0, cell.ctypes.data_as(C.c_void_p)) == 0 and cell.tolist() == [1, 0]
    assert lib.natac_bam_ref_cells(C.c_void_p(h), 1, cell.ctypes.data_as(C.c_void_p)) == -1
    lib.natac_bam_close(C.c_void_p(h))
    plain = C.c_void_p()
    assert lib.natac_frag_open(path.encode(), 1, C.byref(plain)) == 0
    assert lib.natac_bam_ref_cells(plain, 0, cell.ctypes.data_as(C.c_void_p)) == -1 and "no cell indices" in lib.natac_last_error().decode()
    lib.natac_bam_close(plain)


# ---- the restatement of the matrix ----------------------------------------------------------------------------------------------------
def test_restatement_row_sums_are_the_region_counts():
    rng = np.random.default_rng(5)
    pos = np.sort(rng.integers(-20, 3000, 1500))
    tlen = rng.integers(0, 400, 1500)
    cell = rng.integers(0, 23, 1500)
    starts = rng.integers(-50, 3000, 120)
    ends = starts + rng.integers(0, 600, 120)
    for atac in (0, 1):
        ptr, col, val = cell_counts_brute(pos, tlen, cell, starts, ends, 30, 250, atac)
        assert np.array_equal(row_sums(ptr, val), region_counts_brute(pos, tlen, starts, ends, 30, 250, atac)) and ptr[-1] == len(col) > 200
        assert all(np.all(np.diff(col[a:b]) > 0) for a, b in zip(ptr[:-1], ptr[1:])) and val.min() >= 1
        b = 7                                            # one cell's column = the counts of its records alone
        column = np.array([int(val[a:e][col[a:e] == b].sum()) for a, e in zip(ptr[:-1], ptr[1:])])
        assert np.array_equal(column, region_counts_brute(pos[cell == b], tlen[cell == b], starts, ends, 30, 250, atac))


# ---- pyatac cellcounts -----------------------------------------------------------------------------------------------------------------
def test_parser_flags_and_defaults():
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    a = pyatac_parser().parse_args(["cellcounts", "--fragments", "f.tsv.gz", "--bed", "w.bed", "--cells", "c.tsv"])
    assert vars(a) == dict(call="cellcounts", fragments="f.tsv.gz", bed="w.bed", cells="c.tsv", header=False, lower=0, upper=500, out=None,
                           format="mtx")
    a = pyatac_parser().parse_args(["cellcounts", "--fragments", "f", "--bed", "w", "--cells", "c", "--header", "--lower", "10", "--upper", "90",
                                    "--out", "o", "--format", "npz"])
    assert (a.header, a.lower, a.upper, a.out, a.format) == (True, 10, 90, "o", "npz")
    for argv in (["--fragments", "f", "--bed", "w"], ["--fragments", "f", "--cells", "c"], ["--bed", "w", "--cells", "c"],
                 ["--fragments", "f", "--bed", "w", "--cells", "c", "--format", "csv"]):
        with pytest.raises(SystemExit):
            pyatac_parser().parse_args(["cellcounts"] + argv)


def test_default_output_name_is_set_before_anything_is_read(tmp_path):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    from nucleoatac_amd.pyatac.get_cellcounts import get_cellcounts
    from nucleoatac_amd.pyatac.get_counts import CountsError
    missing = str(tmp_path / "nowhere")
    a = pyatac_parser().parse_args(["cellcounts", "--fragments", missing, "--bed", os.path.join(missing, "peaks.narrow.bed"), "--cells", missing])
    with pytest.raises(ValueError, match="nowhere: no such file"):
        get_cellcounts(a)
    assert a.out == "peaks.narrow"
    a = pyatac_parser().parse_args(["cellcounts", "--fragments", missing, "--bed", "w.bed", "--cells", missing, "--lower", "5", "--upper", "5"])
    with pytest.raises(CountsError, match=r"--upper \(5\) must be larger than --lower \(5\)"):
        get_cellcounts(a)
    assert a.out == "w" and os.listdir(str(tmp_path)) == []


def test_mtx_text_reads_back(monkeypatch):
    import io

    import scipy.io
    import scipy.sparse
    from nucleoatac_amd.pyatac import get_cellcounts as G
    indptr = np.array([0, 2, 2, 5, 6], np.int64)
    indices = np.array([0, 6, 1, 2, 3, 6], np.int32)
    data = np.array([1, 2147483647, 3, 1, 2, 9], np.int32)
    want = scipy.sparse.csr_matrix((data.astype(np.int64), indices, indptr), shape=(4, 7)).toarray()
    monkeypatch.setattr(G, "TEXT_ROWS", 4)               # more than one block of entries
    text = G.mtx_text(indptr, indices, data, 7)
    assert text.startswith(b"%%MatrixMarket matrix coordinate integer general\n4 7 6\n1 1 1\n1 7 2147483647\n3 2 3\n") and text.endswith(b"4 7 9\n")
    back = scipy.io.mmread(io.BytesIO(text))
    assert back.shape == (4, 7) and np.array_equal(back.toarray(), want)
    empty = G.mtx_text(np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), 5)
    assert empty == b"%%MatrixMarket matrix coordinate integer general\n2 5 0\n"
