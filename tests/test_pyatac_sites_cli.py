"""`pyatac counts` and `pyatac nucleotide` without a device: the parsers against the reference's (pyatac/cli.py:90-107, 175-193), the
default output names, the site rule (centre / slop / clip / skip) and the counting rules restated in Python against the reference's
own outputs (tests/golden/pyatac_sites.npz, made by tests/golden/make_golden_sites.py), the host finish and the value text, the
per-line dinucleotide background, and the error exits that need no device."""
import argparse
import gzip
import os

import numpy as np
import pytest

import sites_ref as R
from conftest import load_golden
from nucleoatac_amd.pyatac.cli import main, pyatac_parser

G = load_golden("pyatac_sites")
NAMES = [str(x) for x in G["chrom_names"]]
SIZES = dict(zip(NAMES, [int(x) for x in G["chrom_lengths"]]))
SEQS = {c: G["seq_" + c] for c in NAMES}
COUNT_CASES = [str(x) for x in G["count_cases"]]
NUC_CASES = [str(x) for x in G["nuc_cases"]]
BED_ROWS = [x.split("\t") for x in str(G["bed_text"]).splitlines()]
KEPT = [(f[0], int(f[1]), int(f[2]), f[5]) for f in BED_ROWS if int(f[2]) - int(f[1]) >= 1]


def golden_text(key):
    return gzip.decompress(G["text_" + key].tobytes()).decode("ascii")


def write_inputs(d):
    bed = str(d / "sites.bed")
    with open(bed, "w") as f:
        f.write(str(G["bed_text"]))
    fasta = str(d / "genome.npz")
    np.savez(fasta, chrom_names=G["chrom_names"], chrom_lengths=G["chrom_lengths"], **{"seq_" + c: SEQS[c] for c in NAMES})
    frags = str(d / "frags.npz")
    np.savez(frags, chrom_names=G["chrom_names"], chrom_lengths=G["chrom_lengths"], **{"pos_" + c: G["pos_" + c] for c in NAMES},
             **{"tlen_" + c: G["tlen_" + c] for c in NAMES})
    text = str(d / "genome.fa")
    with open(text, "wb") as f:
        f.write(R.fasta_text(NAMES, SEQS, int(G["fasta_line_width"])))
    return bed, fasta, frags, text


def test_parsers_have_the_references_flags_and_defaults():
    p = pyatac_parser()
    a = p.parse_args(["counts", "--bam", "x.bam", "--bed", "w.bed"])
    assert vars(a) == dict(call="counts", bam="x.bam", bed="w.bed", out=None, atac=True, lower=0, upper=500)
    a = p.parse_args(["counts", "--bam", "x.bam", "--bed", "w.bed", "--out", "o", "--not_atac", "--lower", "30", "--upper", "200"])
    assert (a.out, a.atac, a.lower, a.upper) == ("o", False, 30, 200)
    a = p.parse_args(["nucleotide", "--fasta", "g.fa", "--bed", "s.bed"])
    assert vars(a) == dict(call="nucleotide", fasta="g.fa", bed="s.bed", dinucleotide=False, up=250, down=250, strand=None, out=None,
                           cores=1, norm=False)
    a = p.parse_args(["nucleotide", "--fasta", "g.fa", "--bed", "s.bed", "--dinucleotide", "--up", "10", "--down", "73", "--strand", "6",
                      "--out", "o", "--cores", "8", "--norm"])
    assert (a.dinucleotide, a.up, a.down, a.strand, a.out, a.cores, a.norm) == (True, 10, 73, 6, "o", 8, True)
    for bad in (["counts", "--bam", "x.bam"], ["counts", "--bed", "w.bed"], ["nucleotide", "--fasta", "g.fa"],
                ["nucleotide", "--bed", "s.bed"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_vplot_and_signal_are_still_rejected():
    for tool in ("vplot", "bias_vplot", "signal"):
        with pytest.raises(SystemExit):
            pyatac_parser().parse_args([tool, "--bam", "x.bam", "--bed", "w.bed"])


def test_default_output_names():
    """the BED's basename minus its last extension, set before anything is read"""
    from nucleoatac_amd.pyatac.get_counts import CountsError, get_counts
    from nucleoatac_amd.pyatac.get_nucleotide import NucleotideError, get_nucleotide
    a = argparse.Namespace(bam="x.bam", bed="/some/dir/my.peaks.bed", out=None, atac=True, lower=5, upper=5)
    with pytest.raises(CountsError):
        get_counts(a)
    assert a.out == "my.peaks"
    a = argparse.Namespace(fasta="g.fa", bed="/some/dir/nucpos.bed.gz", out=None, dinucleotide=False, up=-1, down=0, strand=None,
                           cores=1, norm=False)
    with pytest.raises(NucleotideError):
        get_nucleotide(a)
    assert a.out == "nucpos.bed"


def python_site(start, end, strand, up, down, di, chrom_len):
    """Chunk.center then Chunk.slop(up, down + di) with Python-2 integer division, clipped: (centre, window start, window end)"""
    half = (end - start) // 2
    if strand == "-":
        e = end - half
        s = e - 1
        ws, we = max(0, s - (down + di)), min(chrom_len, e + up)
    else:
        s = start + half
        e = s + 1
        ws, we = max(0, s - up), min(chrom_len, e + down + di)
    return s, ws, we


@pytest.mark.parametrize("key", NUC_CASES)
def test_site_rule_gives_the_references_sites(key):
    from nucleoatac_amd.pyatac.get_nucleotide import site_centers
    di, strand_col, _norm, up, down = [int(x) for x in G["args_" + key]]
    sites = [python_site(s, e, st if strand_col else "+", up, down, di, SIZES[c]) for c, s, e, st in KEPT]
    used = np.array([we - ws == up + down + 1 + di for _, ws, we in sites])
    assert np.array_equal(used, G["used_" + key]), key
    assert 0 < used.sum() < len(used)
    start, end = np.array([k[1] for k in KEPT]), np.array([k[2] for k in KEPT])
    minus = np.array([bool(strand_col) and k[3] == "-" for k in KEPT])
    assert np.array_equal(site_centers(start, end, minus), [s[0] for s in sites])
    if strand_col:      # even-length regions centre one base apart by strand, odd-length ones on the same base
        by = {(c, s, e, st): x[0] for (c, s, e, st), x in zip(KEPT, sites)}
        assert by[("chrA", 1000, 1500, "+")] == 1250 and by[("chrA", 1000, 1500, "-")] == 1249
        assert by[("chrA", 1000, 1501, "+")] == by[("chrA", 1000, 1501, "-")] == 1250
    for (c, s, e, st), (ctr, _, _), u in zip(KEPT, sites, used):     # site_window, which the GPU tests' restatement uses, agrees
        assert R.site_window(ctr, bool(strand_col) and st == "-", up, down, 1 + di, SIZES[c])[2] == u


def read_columns(tmp_path, strand_col):
    from nucleoatac_amd.pyatac.chunk import ChunkList, read_bed_columns
    bed = write_inputs(tmp_path)[0]
    names, chrom, start, end, minus = read_bed_columns(bed, strand_col=strand_col)
    chunks = ChunkList.read(bed, strand_col=strand_col)
    assert [(c.chrom, c.start, c.end, c.strand == "-") for c in chunks] == [
        (names[k], s, e, m) for k, s, e, m in zip(chrom.tolist(), start.tolist(), end.tolist(), minus.tolist())]
    return names, chrom, start, end, minus


@pytest.mark.parametrize("key", NUC_CASES)
def test_restated_counts_and_host_finish_give_the_references_matrix_and_text(key, tmp_path):
    """the NumPy restatement of the window counts, then the package's host finish and value text: the stored float64 matrix bit for
    bit and the file's text byte for byte"""
    from nucleoatac_amd.pyatac.get_nucleotide import ACGT, DINUCLEOTIDES, nucfreq_text, site_centers
    di, strand_col, norm, up, down = [int(x) for x in G["args_" + key]]
    names, chrom, start, end, minus = read_columns(tmp_path, strand_col or None)
    center = site_centers(start, end, minus)
    M, n = 0, 0
    for k, c in enumerate(names):
        idx = np.flatnonzero((chrom == k) & (center >= 0) & (center < SIZES[c]))
        m, u = R.site_counts_ref(SEQS[c], center[idx], minus[idx], up, down, 1 + di)
        M, n = M + m, n + u
    assert n == int(G["used_" + key].sum())
    result = np.asarray(M, np.float64) / float(n)
    if norm:
        bg = G["bg_di"] if di else G["bg_mono"]
        result = result / np.reshape(np.repeat(bg, result.shape[1]), result.shape)
    assert np.array_equal(result, G["mat_" + key]), key
    assert nucfreq_text(DINUCLEOTIDES if di else ACGT, result) == golden_text(key), key
    assert DINUCLEOTIDES == R.DINUCLEOTIDES and DINUCLEOTIDES[:5] == ["CC", "CG", "CA", "CT", "GC"]


def test_soft_masked_minus_site_is_reversed_but_not_complemented():
    """the golden's minus-strand site over the lower-case stretch (with upper-case islands) against seq.get_sequence on the cased
    sequence, and against what a complement after upper-casing would give"""
    from nucleoatac_amd.pyatac.chunk import Chunk
    from nucleoatac_amd.pyatac.seq import FastaStore, get_sequence
    fs = FastaStore({c: SEQS[c] for c in NAMES})
    ch = Chunk("chrA", 1290, 1311, strand="-")
    ch.center()
    ch.slop(SIZES, up=40, down=40)
    want = get_sequence(ch, fs)
    raw = SEQS["chrA"][ch.start:ch.end].tobytes().decode()
    assert any(x.islower() for x in raw) and any(x.isupper() for x in raw)
    naive = raw.upper()[::-1].translate(str.maketrans("ACGT", "TGCA"))
    assert want != naive
    M, n = R.site_counts_ref(SEQS["chrA"], [ch.start + 40], [True], 40, 40, 1)
    assert n == 1
    for j, letter in enumerate(want):
        assert M[:, j].tolist() == [int(letter == x) for x in "ACGT"], j


@pytest.mark.parametrize("key", COUNT_CASES)
def test_restated_counting_rule_gives_the_references_counts(key, tmp_path):
    atac, lower, upper = [int(x) for x in G["args_" + key]]
    names, chrom, start, end, _ = read_columns(tmp_path, None)
    out = np.zeros(len(start), np.int64)
    for k, c in enumerate(names):
        idx = np.flatnonzero(chrom == k)
        out[idx] = R.region_counts_brute(G["pos_" + c], G["tlen_" + c], start[idx], end[idx], lower, upper, atac)
        assert np.array_equal(out[idx], R.region_counts_ref(G["pos_" + c], G["tlen_" + c], start[idx], end[idx], lower, upper, atac))
    assert "".join("%d\n" % v for v in out) == golden_text(key), key
    assert out.max() > 50 and len(out) == len(KEPT)


def test_insert_size_zero_counts_through_its_right_end():
    """ilen == 0: r = l - 1.  The window that ends at l holds r only and counts the record when lower <= 0"""
    pos, tlen = np.array([2500]), np.array([8])
    for (s, e), want in (((2494, 2504), 1), ((2504, 2510), 1), ((2494, 2503), 0), ((2505, 2510), 0)):
        assert R.region_counts_brute(pos, tlen, [s], [e], 0, 500, 1).tolist() == [want], (s, e)
        assert R.region_counts_ref(pos, tlen, [s], [e], 0, 500, 1).tolist() == [want], (s, e)
    assert R.region_counts_brute(pos, tlen, [2494], [2504], 1, 500, 1).tolist() == [0]
    vals = [int(x) for x in golden_text("counts_atac_0_500").split()]
    assert vals[[k[:3] for k in KEPT].index(("chrA", 2494, 2504))] == 1       # the reference counts it too


def test_value_text_rule():
    from nucleoatac_amd.pyatac.get_nucleotide import value_text
    assert value_text(8.33333333333e-05) == "8.33e-05"          # the deliberate deviation: the 8-byte cut would say 8.333333
    assert value_text(0.30000000000000004) == "0.3"
    assert value_text(1.0) == "1.0"
    assert value_text(0.0) == "0.0"
    assert value_text(0.123456789012345) == "0.123456"
    assert value_text(1.0 / 3) == "0.333333"
    assert value_text(12.5) == "12.5"
    assert value_text(0.0001) == "0.0001"                       # the smallest value Python 2 writes without an exponent
    assert value_text(9.99e-05) == "9.99e-05"
    assert all(len(value_text(v)) <= 8 for v in (1e-99, 123456.789012, 2.0 / 3, 1e-5))


def test_dinucleotide_background_counts_per_line(tmp_path):
    from nucleoatac_amd.pyatac.get_nucleotide import DINUCLEOTIDES, dinucleotide_line_freqs
    text = write_inputs(tmp_path)[3]
    assert np.array_equal(dinucleotide_line_freqs(text, DINUCLEOTIDES), G["bg_di"])
    # it depends on the line layout: non-overlapping per line, blind across line breaks
    p = tmp_path / "t.fa"
    p.write_text(">x\nAAAC\nCaa\n")
    f = dict(zip(DINUCLEOTIDES, dinucleotide_line_freqs(str(p), DINUCLEOTIDES) * 7))
    assert f["AA"] == 2 and f["AC"] == 1 and f["CA"] == 1 and f["CC"] == 0


def run_main(argv, capsys):
    rc = main(argv)
    err = [x for x in capsys.readouterr().err.splitlines() if x.strip()]
    return rc, err


def test_error_exits_without_a_device(tmp_path, capsys):
    bed, fasta, frags, text = write_inputs(tmp_path)
    out = str(tmp_path / "o")

    def refused(argv, word):
        rc, err = run_main(argv + ["--out", out], capsys)
        assert rc == 1 and len(err) == 1 and word in err[0], (argv, err)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")], argv

    refused(["counts", "--bam", frags, "--bed", bed, "--lower", "200", "--upper", "200"], "--upper")
    refused(["counts", "--bam", frags, "--bed", bed, "--lower", "200", "--upper", "100"], "--upper")
    refused(["nucleotide", "--fasta", fasta, "--bed", bed, "--up", "-1"], "--up")
    refused(["nucleotide", "--fasta", fasta, "--bed", bed, "--down", "-5"], "--down")
    refused(["nucleotide", "--fasta", fasta, "--bed", bed, "--dinucleotide", "--norm"], "no lines")
    other = tmp_path / "other.bed"
    other.write_text("chrA\t10\t20\nchrQ\t5\t50\n")
    refused(["counts", "--bam", frags, "--bed", str(other)], "chrQ")
    refused(["nucleotide", "--fasta", fasta, "--bed", str(other)], "chrQ")
    short = tmp_path / "short.bed"
    short.write_text("chrA\t10\t20\tn\t0\t+\nchrA\t30\t40\tn\n")
    refused(["nucleotide", "--fasta", fasta, "--bed", str(short), "--strand", "6"], "line 2")
    nowhere = tmp_path / "nowhere.bed"
    nowhere.write_text("chrA\t5000\t5100\nchrC\t100\t101\n")          # every centre lies past its chromosome's end: n == 0
    refused(["nucleotide", "--fasta", fasta, "--bed", str(nowhere)], "no site")


def test_empty_bed_writes_an_empty_counts_file(tmp_path, capsys):
    _, _, frags, _ = write_inputs(tmp_path)
    empty = tmp_path / "empty.bed"
    empty.write_text("chrA\t7\t7\n")            # its only region is dropped
    rc, err = run_main(["counts", "--bam", frags, "--bed", str(empty), "--out", str(tmp_path / "e")], capsys)
    assert rc == 0 and not err
    with gzip.open(str(tmp_path / "e.counts.txt.gz"), "rb") as f:
        assert f.read() == b""


def test_cased_fasta_loader_keeps_the_files_case(tmp_path):
    from nucleoatac_amd.pyatac.seq import FastaStore
    _, fasta, _, text = write_inputs(tmp_path)
    for src in (fasta, text):
        fs = FastaStore.open_cased(src)
        assert fs.references == NAMES
        for c in NAMES:
            assert np.array_equal(fs.seqs[c], SEQS[c]), (src, c)
    gz = str(tmp_path / "genome.fa.gz")
    with open(text, "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read().replace(b"\n", b"\r\n"))
    assert all(np.array_equal(FastaStore.open_cased(gz).seqs[c], SEQS[c]) for c in NAMES)
