"""CPU: the host side of `pyatac cellqc` (nucleoatac_amd/pyatac/get_cellqc.py): the parser, the argument rules, the default output base,
the centring of the sites, the peak merge, the two NumPy restatements of tests/cellqc_ref.py against each other, and the host finish --
formulas, NA, pass and the four file texts -- from hand-made integer arrays."""
import os

import numpy as np
import pytest

import cellqc_ref as R


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


def _args(*argv):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    return pyatac_parser().parse_args(["cellqc"] + list(argv))


def test_parser_flags_and_defaults():
    a = _args("--fragments", "f.tsv.gz", "--cells", "c.tsv")
    assert vars(a) == dict(call="cellqc", fragments="f.tsv.gz", cells="c.tsv", header=False, tss=None, strand=None, peaks=None, flank=1000,
                           center=500, edge=100, min_tss_enrichment=None, min_frip=None, out=None)
    a = _args("--fragments", "f", "--cells", "c", "--header", "--tss", "t.bed", "--strand", "6", "--peaks", "p.bed", "--flank", "2000",
              "--center", "50", "--edge", "200", "--min_tss_enrichment", "4.5", "--min_frip", "0.25", "--out", "o")
    assert vars(a) == dict(call="cellqc", fragments="f", cells="c", header=True, tss="t.bed", strand=6, peaks="p.bed", flank=2000, center=50,
                           edge=200, min_tss_enrichment=4.5, min_frip=0.25, out="o")
    for argv in (["--fragments", "f"], ["--cells", "c"], ["--fragments", "f", "--cells", "c", "--flank", "x"]):
        with pytest.raises(SystemExit):
            _args(*argv)


RULES = [([], "at least one of --tss and --peaks is required"),
         (["--peaks", "P", "--min_tss_enrichment", "2"], "--min_tss_enrichment needs --tss"),
         (["--tss", "T", "--min_frip", "0.1"], "--min_frip needs --peaks"),
         (["--tss", "T", "--center", "-1"], "--center (-1) must not be negative"),
         (["--tss", "T", "--edge", "0"], "--edge (0) must be at least 1"),
         (["--tss", "T", "--center", "901", "--edge", "100"], "--center (901) + --edge (100) must not exceed --flank (1000)"),
         (["--tss", "T", "--flank", "0", "--center", "0", "--edge", "1"], "--flank (0) must be in [1, "),
         (["--peaks", "P", "--flank", "0"], "--flank (0) must be in [1, "),
         (["--tss", "T", "--flank", "MAX+1"], "--flank (MAX+1) must be in [1, MAX]"),
         (["--tss", "MISSING"], "missing.bed: no such file"),
         (["--peaks", "MISSING"], "missing.bed: no such file"),
         (["--tss", "T", "--cells", "MISSING"], "missing.bed: no such file"),
         (["--tss", "T", "--fragments", "MISSING"], "missing.bed: no such file")]


@pytest.mark.parametrize("k", range(len(RULES)))
def test_every_argument_rule_exits_1_and_writes_nothing(tmp_path, monkeypatch, capsys, k):
    from nucleoatac_amd._lib import CELLQC_MAX_FLANK
    from nucleoatac_amd.pyatac.cli import main
    monkeypatch.chdir(tmp_path)
    for name, text in (("t.bed", b"chr1\t10\t20\n"), ("p.bed", b"chr1\t10\t20\n"), ("c.tsv", b"AA\n"), ("f.tsv", b"chr1\t5\t9\tAA\n")):
        open(name, "wb").write(text)
    before = sorted(os.listdir("."))
    extra, message = RULES[k]
    sub = {"T": "t.bed", "P": "p.bed", "MISSING": "missing.bed", "MAX+1": str(CELLQC_MAX_FLANK + 1)}
    argv = ["cellqc", "--fragments", "f.tsv", "--cells", "c.tsv"] + [sub.get(x, x) for x in extra]
    assert main(argv) == 1
    out = capsys.readouterr()
    want = message.replace("MAX+1", str(CELLQC_MAX_FLANK + 1)).replace("MAX", str(CELLQC_MAX_FLANK))
    assert out.err.startswith("pyatac cellqc: ") and want in out.err and out.out.startswith("---------")
    assert sorted(os.listdir(".")) == before


def test_the_bindings_constants_are_the_headers():
    import re

    from conftest import ROOT
    from nucleoatac_amd._lib import CELLQC_MAX_FLANK, SPLIT_MAX_BARCODES
    hdr = open(os.path.join(ROOT, "include", "natac.h")).read()
    assert CELLQC_MAX_FLANK == int(re.search(r"#define NATAC_CELLQC_MAX_FLANK (\d+)", hdr).group(1)) >= 2000
    assert SPLIT_MAX_BARCODES == int(re.search(r"#define NATAC_SPLIT_MAX_BARCODES (\d+)", hdr).group(1))


def test_default_output_base(tmp_path, monkeypatch):
    from nucleoatac_amd.pyatac import get_cellqc as G
    from nucleoatac_amd.pyatac.cellgroups import default_base
    assert default_base("/data/run1/atac.fragments.tsv.gz") == "atac.fragments"
    # the command takes its base from the fragment file, not from a BED: with a table that lists no barcode the error comes before any file
    monkeypatch.chdir(tmp_path)
    open("t.bed", "wb").write(b"chr1\t10\t20\n")
    open("c.tsv", "wb").write(b"AA\n")
    open("my.sample.tsv", "wb").write(b"chr1\t5\t9\tCC\n")
    a = _args("--fragments", "my.sample.tsv", "--cells", "c.tsv", "--tss", "t.bed", "--min_tss_enrichment", "1")
    with pytest.raises(G.CellQCError, match="no cell passes"):
        G.get_cellqc(a)
    assert sorted(os.listdir(".")) == ["c.tsv", "my.sample.tsv", "t.bed"]
    a = _args("--fragments", "my.sample.tsv", "--cells", "c.tsv", "--tss", "t.bed")
    ok, texts = G.get_cellqc(a)                          # nothing in reach: zeros, no device needed for a store without listed records
    assert ok.tolist() == [True]
    assert sorted(os.listdir(".")) == sorted(["c.tsv", "my.sample.tsv", "t.bed"] + ["my.sample" + s for s in texts])
    assert open("my.sample.cellqc.tsv", "rb").read() == G.HEADER + b"AA\t0\t0\t0\tNA\tNA\tNA\t1\n"
    assert open("my.sample.cellqc.txt").read() == ("barcodes_listed\t1\nbarcodes_seen\t0\ndata_lines\t1\nunassigned_lines\t1\nsites\t1\n"
                                                   "peak_intervals\t0\npassing\t1\n")


def test_centring_of_even_and_odd_rows_on_both_strands():
    from nucleoatac_amd.pyatac.chunk import Chunk
    from nucleoatac_amd.pyatac.get_cellqc import site_centers, sites_by_chrom
    start = np.array([100, 100, 100, 100, 7, 7], np.int64)
    end = np.array([110, 111, 101, 102, 8, 9], np.int64)
    assert site_centers(start, end, np.zeros(6, bool)).tolist() == [105, 105, 100, 101, 7, 8]
    assert site_centers(start, end, np.ones(6, bool)).tolist() == [104, 105, 100, 100, 7, 7]
    for s, e in zip(start.tolist(), end.tolist()):
        for strand, minus in (("+", False), ("-", True)):
            ch = Chunk("chr1", s, e, strand=strand)
            ch.center()
            assert ch.start == site_centers(np.array([s]), np.array([e]), np.array([minus]))[0]
    # per chromosome, ascending and stable, the strand carried along
    chrom = np.array([0, 1, 0, 0, 1, 0], np.int32)
    minus = np.array([1, 0, 0, 1, 1, 0], bool)
    by = sites_by_chrom(["a", "b"], chrom, start, end, minus)
    assert by["a"][0].tolist() == [8, 100, 100, 104] and by["a"][1].tolist() == [0, 0, 1, 1] and by["a"][1].dtype == np.uint8
    assert by["b"][0].tolist() == [7, 105] and by["b"][1].tolist() == [1, 0]


def test_peak_merge():
    from nucleoatac_amd.pyatac.get_cellqc import merge_peaks, peaks_by_chrom
    s, e = merge_peaks([10, 15, 40], [20, 30, 50])                       # overlapping
    assert (s.tolist(), e.tolist()) == ([10, 40], [30, 50]) and s.dtype == e.dtype == np.int64
    s, e = merge_peaks([10, 12, 13, 60], [50, 20, 14, 61])               # nested
    assert (s.tolist(), e.tolist()) == ([10, 60], [50, 61])
    s, e = merge_peaks([10, 20], [20, 30])                               # touching: apart or joined, the same bases either way
    assert (s.tolist(), e.tolist()) in (([10, 20], [20, 30]), ([10], [30]))
    s, e = merge_peaks([40, 10, 45, 15, 10], [50, 20, 47, 30, 12])       # unsorted
    assert (s.tolist(), e.tolist()) == ([10, 40], [30, 50])
    s, e = merge_peaks([10, 25, 25, 40], [20, 25, 24, 41])               # zero-length and negative rows are dropped
    assert (s.tolist(), e.tolist()) == ([10, 40], [20, 41])
    assert [x.tolist() for x in merge_peaks([], [])] == [[], []] and [x.tolist() for x in merge_peaks([5], [5])] == [[], []]
    rng = np.random.default_rng(3)                                       # seeded: the covered bases are those of the rows
    a = rng.integers(0, 400, 60)
    b = a + rng.integers(-2, 30, 60)
    s, e = merge_peaks(a, b)
    covered = np.zeros(500, bool)
    for x, y in zip(a, b):
        covered[x:max(x, y)] = True
    mine = np.zeros(500, bool)
    for x, y in zip(s, e):
        assert y > x
        mine[x:y] = True
    assert np.array_equal(mine, covered) and np.all(s[1:] >= e[:-1]) and np.all(np.diff(s) > 0)
    by = peaks_by_chrom(["a", "b"], np.array([0, 1, 0], np.int32), np.array([10, 10, 15], np.int64), np.array([20, 20, 30], np.int64))
    assert [x.tolist() for x in by["a"]] == [[10], [30]] and [x.tolist() for x in by["b"]] == [[10], [20]]


@pytest.mark.parametrize("fce", [(1, 0, 1), (50, 10, 5), (1000, 500, 100), (300, 0, 300)])
@pytest.mark.parametrize("n_cells", [7, 1])
def test_brute_and_fast_restatement_agree(fce, n_cells):
    pos, tlen, cell, sc, sm, ps, pe = R.mixed_case(11, n_cells, *fce)
    brute = R.cellqc_brute(pos, tlen, cell, n_cells, sc, sm, *fce, ps, pe)
    R.assert_same(R.cellqc_ref(pos, tlen, cell, n_cells, sc, sm, *fce, ps, pe), brute)
    R.assert_same(R.cellqc_ref(pos, tlen, cell, n_cells, sc, None, *fce, None, None),
                  R.cellqc_brute(pos, tlen, cell, n_cells, sc, None, *fce, None, None))
    assert brute[3].sum() > 0 and brute[2].sum() > 0 and brute[0].sum() <= brute[3].sum() and brute[2].sum() <= len(pos)
    # the classes by hand from the profile: symmetric in d, so the strand does not move them
    f, c, e = fce
    off = np.abs(np.arange(-f, f + 1))
    assert brute[0].sum() == brute[3][off <= c].sum() and brute[1].sum() == brute[3][off > f - e].sum()


def test_restatement_on_a_hand_made_case():
    # one plus site at 100, one minus site at 100; one record l = 98, r = 103 (pos 94, tlen 14)
    out = R.cellqc_brute([94], [14], [1], 3, [100, 100], [0, 1], 3, 2, 1, [103, 200], [104, 300])
    assert out[3].tolist() == [1, 1, 0, 0, 0, 1, 1]      # plus: d = -2, +3; minus: d = +2, -3
    assert out[0].tolist() == [0, 2, 0] and out[1].tolist() == [0, 2, 0] and out[2].tolist() == [0, 1, 0]
    R.assert_same(R.cellqc_ref([94], [14], [1], 3, [100, 100], [0, 1], 3, 2, 1, [103, 200], [104, 300]), out)
    # both ends in peaks count once; ilen == 0 puts r at l - 1
    out = R.cellqc_brute([96], [8], [0], 1, [100], None, 1, 0, 1, [99, 100], [100, 101])
    assert out[3].tolist() == [1, 1, 0] and out[0].tolist() == [1] and out[1].tolist() == [1] and out[2].tolist() == [1]


# ---- the host finish ------------------------------------------------------------------------------------------------------------------
BARCODES = [b"AA-1", b"CC-1", b"GG-1", b"TT-1"]
FRAGS = np.array([100, 40, 0, 10], np.int64)
TC = np.array([2002, 1001, 0, 5], np.int64)
TF = np.array([400, 0, 0, 200], np.int64)
IP = np.array([25, 40, 0, 1], np.int64)
PROFILE = np.array([3, 0, 7, 1, 2], np.int64)


def test_finish_formulas_na_and_pass():
    from nucleoatac_amd.pyatac.get_cellqc import HEADER, finish
    ok, texts = finish(BARCODES, FRAGS, TC, TF, IP, PROFILE, 2, 1, 1, min_tss_enrichment=0.5, min_frip=0.25, n_unassigned=6, n_sites=9,
                       n_peaks=4)
    # (tss_center / (2 * 1 + 1)) / (tss_flank / (2 * 1)); NA with tss_flank == 0 and with fragments == 0, and an NA fails its threshold
    assert "%.4f" % ((2002 / 3.0) / (400 / 2.0)) == "3.3367" and "%.4f" % ((5 / 3.0) / (200 / 2.0)) == "0.0167"
    assert ok.tolist() == [True, False, False, False]
    assert texts[".cellqc.tsv"] == (HEADER + b"AA-1\t100\t2002\t400\t3.3367\t25\t0.2500\t1\n" + b"CC-1\t40\t1001\t0\tNA\t40\t1.0000\t0\n"
                                    + b"GG-1\t0\t0\t0\tNA\t0\tNA\t0\n" + b"TT-1\t10\t5\t200\t0.0167\t1\t0.1000\t0\n")
    assert HEADER == b"#barcode\tfragments\ttss_center\ttss_flank\ttss_enrichment\tin_peaks\tfrip\tpass\n"
    assert texts[".cellqc.cells.tsv"] == b"AA-1\n"
    assert texts[".cellqc.tss_profile.txt"] == b"-2\t3\n-1\t0\n0\t7\n1\t1\n2\t2\n"
    assert texts[".cellqc.txt"] == (b"barcodes_listed\t4\nbarcodes_seen\t3\ndata_lines\t156\nunassigned_lines\t6\nsites\t9\npeak_intervals\t4\n"
                                    b"passing\t1\n")
    assert list(texts) == [".cellqc.tsv", ".cellqc.cells.tsv", ".cellqc.tss_profile.txt", ".cellqc.txt"]
    # thresholds hold with >=; without thresholds every listed cell passes, the NA ones too
    ok, _ = finish(BARCODES, FRAGS, TC, TF, IP, PROFILE, 2, 1, 1, min_tss_enrichment=(5 / 3.0) / 100.0, min_frip=0.1)
    assert ok.tolist() == [True, False, False, True]
    ok, texts = finish(BARCODES, FRAGS, TC, TF, IP, PROFILE, 2, 1, 1)
    assert ok.all() and texts[".cellqc.cells.tsv"] == b"AA-1\nCC-1\nGG-1\nTT-1\n"
    ok, _ = finish(BARCODES, FRAGS, TC, TF, IP, PROFILE, 2, 1, 1, min_frip=0.0)
    assert ok.tolist() == [True, True, False, True]      # fragments == 0: NA fails even a bound of 0
    ok, _ = finish(BARCODES, FRAGS, TC, TF, IP, PROFILE, 2, 1, 1, min_tss_enrichment=0.0)
    assert ok.tolist() == [True, False, False, True]


def test_finish_columns_of_an_input_that_was_not_given_hold_na():
    from nucleoatac_amd.pyatac.get_cellqc import HEADER, finish
    ok, texts = finish(BARCODES, FRAGS, None, None, IP, None, 2, 1, 1, min_frip=0.5, n_peaks=4)
    assert ok.tolist() == [False, True, False, False] and ".cellqc.tss_profile.txt" not in texts and len(texts) == 3
    assert texts[".cellqc.tsv"] == (HEADER + b"AA-1\t100\tNA\tNA\tNA\t25\t0.2500\t0\n" + b"CC-1\t40\tNA\tNA\tNA\t40\t1.0000\t1\n"
                                    + b"GG-1\t0\tNA\tNA\tNA\t0\tNA\t0\n" + b"TT-1\t10\tNA\tNA\tNA\t1\t0.1000\t0\n")
    ok, texts = finish(BARCODES, FRAGS, TC, TF, None, PROFILE, 2, 1, 1, n_sites=2)
    assert ok.all() and texts[".cellqc.tsv"].splitlines()[1] == b"AA-1\t100\t2002\t400\t3.3367\tNA\tNA\t1"
    assert b"sites\t2\npeak_intervals\t0\n" in texts[".cellqc.txt"]


def test_no_cell_passes_leaves_nothing_behind(tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac import get_cellqc as G
    from nucleoatac_amd.pyatac.cli import main
    with pytest.raises(G.CellQCError, match="no cell passes"):
        G.finish(BARCODES, FRAGS, TC, TF, IP, PROFILE, 2, 1, 1, min_tss_enrichment=1000.0)
    # through the command: the counting is replaced by the hand-made arrays, the finish and the writing are the command's own
    monkeypatch.chdir(tmp_path)
    open("t.bed", "wb").write(b"chr1\t10\t20\n")
    open("p.bed", "wb").write(b"chr1\t10\t20\n")
    open("c.tsv", "wb").write(b"".join(b + b"\n" for b in BARCODES))
    open("f.tsv", "wb").write(b"".join(b"chr1\t5\t9\t" + b + b"\n" for b, n in zip(BARCODES, [3, 2, 0, 1]) for _ in range(n)))
    monkeypatch.setattr(G, "cell_qc", lambda *a, **k: (TC, TF, IP, PROFILE))
    before = sorted(os.listdir("."))
    argv = ["cellqc", "--fragments", "f.tsv", "--cells", "c.tsv", "--tss", "t.bed", "--peaks", "p.bed", "--flank", "2", "--center", "1", "--edge", "1"]
    assert main(argv + ["--min_tss_enrichment", "1000"]) == 1
    err = capsys.readouterr().err
    assert err.startswith("pyatac cellqc: ") and "no cell passes" in err and sorted(os.listdir(".")) == before
    assert main(argv + ["--min_tss_enrichment", "3"]) == 0
    assert sorted(set(os.listdir(".")) - set(before)) == sorted("f.cellqc." + x for x in ("cells.tsv", "tsv", "tss_profile.txt", "txt"))
    assert open("f.cellqc.cells.tsv", "rb").read() == b"AA-1\n"
    assert open("f.cellqc.tsv", "rb").read().splitlines()[1] == b"AA-1\t3\t2002\t400\t3.3367\t25\t8.3333\t1"
    capsys.readouterr()
