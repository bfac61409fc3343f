"""`pyatac pwm | sizes` (nucleoatac_amd/pyatac/cli.py): the parser's flags and defaults, the region lists, the host finish of the PWM
fit (normalise, symmetrise) against a numpy restatement and against the reference's matrices, the descriptor writer; on the GPU,
`pyatac sizes` with and without --bed against the reference's .fragmentsizes.txt byte for byte."""
import numpy as np
import pytest

from conftest import load_golden

G = load_golden("pwm_fit")


def test_parser_flags_and_defaults():
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    p = pyatac_parser()
    a = p.parse_args(["pwm", "--fasta", "g.fa", "--bam", "x.bam"])
    assert (a.call, a.fasta, a.bam, a.bed, a.flank, a.lower, a.upper, a.atac, a.sym, a.dinucleotide, a.out, a.cores) == \
        ("pwm", "g.fa", "x.bam", None, 10, 0, 2000, True, True, False, None, 1)
    a = p.parse_args(["pwm", "--fasta", "g.fa", "--bam", "x.bam", "--bed", "r.bed", "--flank", "25", "--lower", "3", "--upper", "500",
                      "--not_atac", "--no_sym", "--dinucleotide", "--cores", "8", "--out", "o"])
    assert (a.bed, a.flank, a.lower, a.upper, a.atac, a.sym, a.dinucleotide, a.cores, a.out) == ("r.bed", 25, 3, 500, False, False, True, 8, "o")
    a = p.parse_args(["sizes", "--bam", "x.bam"])
    assert (a.call, a.bam, a.bed, a.out, a.atac, a.lower, a.upper, a.no_plot) == ("sizes", "x.bam", None, None, True, 0, 500, False)
    a = p.parse_args(["sizes", "--bam", "x.bam", "--bed", "r.bed", "--out", "o", "--not_atac", "--lower", "5", "--upper", "100",
                      "--no_plot"])
    assert (a.bed, a.out, a.atac, a.lower, a.upper, a.no_plot) == ("r.bed", "o", False, 5, 100, True)
    for bad in (["pwm", "--bam", "x.bam"], ["pwm", "--fasta", "g.fa"], ["sizes"], ["vplot", "--bam", "x.bam"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_genome_regions_tile_every_chromosome():
    from nucleoatac_amd.pyatac.get_pwm import genome_regions
    chrs = {"b": 25, "a": 10000, "c": 20}
    for flank, tile in ((10, 3000), (0, 4096), (10, 1 << 22)):
        r = genome_regions(chrs, flank, tile=tile)
        assert all(c.end - c.start <= tile and c.end > c.start for c in r)
        for name, L in chrs.items():
            mine = [c for c in r if c.chrom == name]
            cover = np.zeros(L, int)
            for c in mine:
                cover[c.start:c.end] += 1
            want = np.zeros(L, int)
            want[flank:max(flank, L - flank)] = 1
            assert np.array_equal(cover, want), (name, flank)
        assert [c.chrom for c in r] == sorted(c.chrom for c in r)


def test_bed_regions_clip_drop_and_keep_overlaps(tmp_path):
    from nucleoatac_amd.pyatac.get_pwm import bed_regions
    bed = tmp_path / "r.bed"
    bed.write_text("chrA\t0\t50\nchrA\t30\t80\nchrA\t2\t8\nchrA\t90\t130\nchrZ\t5\t50\nchrB\t10\t20\n")
    chrs = {"chrA": 100, "chrB": 25}
    with pytest.warns(UserWarning, match="chrZ"):
        r = bed_regions(str(bed), chrs, 10)
    assert [(c.chrom, c.start, c.end) for c in r] == [("chrA", 10, 50), ("chrA", 30, 80), ("chrA", 90, 90)][:2] + [("chrB", 10, 15)]
    with pytest.warns(UserWarning):
        r = bed_regions(str(bed), chrs, 0)
    assert [(c.chrom, c.start, c.end) for c in r] == [("chrA", 0, 50), ("chrA", 30, 80), ("chrA", 2, 8), ("chrA", 90, 100),
                                                      ("chrB", 10, 20)]


def _restated_finish(M, n, freqs, flank, sym):
    """the finish of pyatac/get_pwm.py:80-93 written out column by column"""
    K = 2 * flank + 1
    P = np.empty((4, K))
    for i in range(4):
        for j in range(K):
            P[i, j] = (float(M[i, j]) / float(n)) / float(freqs[i])
    if not sym:
        return P
    out = np.empty_like(P)
    for i in range(4):
        for j in range(flank + 1):
            out[i, j] = (P[i, j] + P[3 - i, K - 1 - j]) / 2
    for i in range(4):
        for j in range(flank + 1, K):
            out[i, j] = out[3 - i, K - 1 - j]
    return out


@pytest.mark.parametrize("flank", [0, 1, 10, 100])
@pytest.mark.parametrize("sym", [True, False])
def test_finish_against_a_restatement(flank, sym):
    from nucleoatac_amd.pyatac.get_pwm import finish_pwm
    rng = np.random.default_rng(flank + 7 * sym)
    M = rng.integers(0, 10 ** 9, (4, 2 * flank + 1))
    freqs = rng.uniform(0.1, 0.4, 4)
    n = int(M.sum(axis=0).max()) + 5
    got = finish_pwm(M, n, freqs, flank, sym)
    want = _restated_finish(M, n, freqs, flank, sym)
    assert got.shape == (4, 2 * flank + 1) and np.array_equal(got, want)


def test_finish_reproduces_the_reference_matrices():
    from nucleoatac_amd.pyatac.get_pwm import finish_pwm
    for key in (str(x) for x in G["cases"]):
        p = dict((x[0], x[1:]) for x in key.split("_"))
        got = finish_pwm(G["M_" + key], int(G["n_" + key]), G["freqs_" + key], int(p["f"]), p["s"] == "1")
        ref = G["pwm_" + key]
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), key


def test_pwm_writer_default_unchanged_and_py2_form(tmp_path):
    from nucleoatac_amd.pyatac.bias import PWM
    m = np.array([[0.1, 1.0 / 3], [2.0, 1e-20]])
    w = PWM(m, 0, 1, ["A", "C"])
    w.save(str(tmp_path / "a.txt"))
    w.save(str(tmp_path / "b.txt"), py2_floats=True)
    head = "#PWM Descriptor File\n#Contains PWM and pertinent information\n#up\n0\n#down\n1\n#nucleotides\nA\tC\n#mat\n"
    assert (tmp_path / "a.txt").read_text() == head + "0.1\t0.3333333333333333\n2.0\t1e-20\n"
    assert (tmp_path / "b.txt").read_text() == head + "0.1\t0.333333333333\n2.0\t1e-20\n"
    assert PWM.open(w) is w


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sizes_all_l0_u500_a1", "sizes_all_l30_u250_a0", "sizes_bed_l0_u500_a1", "sizes_bed_l30_u250_a0"])
def test_sizes_matches_the_reference_text(tmp_path, case, capsys):
    from nucleoatac_amd.pyatac.cli import main
    from nucleoatac_amd.pyatac.tracks import _py2_float_str
    names = [str(x) for x in G["chrom_names"]]
    empty = np.zeros(0, np.int64)
    bam = str(tmp_path / "reads.npz")
    np.savez(bam, chrom_names=G["chrom_names"], chrom_lengths=G["chrom_lengths"],
             **{k + c: (G[k + c] if k + c in G else empty) for c in names for k in ("pos_", "tlen_")})
    bed = tmp_path / "r.bed"
    bed.write_text(str(G["bed_sizes_text"]))
    _, kind, lo, up, at = case.split("_")
    argv = ["sizes", "--bam", bam, "--lower", lo[1:], "--upper", up[1:], "--out", str(tmp_path / "o")]
    if kind == "bed":
        argv += ["--bed", str(bed)]
    if at == "a0":
        argv += ["--not_atac"]
    assert main(argv) == 0
    assert capsys.readouterr().out.count("plots are not produced") == 1
    ref = str(G["text_" + case]).split("\n")
    ref[5] = "\t".join(_py2_float_str(float(x)) for x in ref[5].split("\t"))      # the reference's values as Python 2 printed them
    assert (tmp_path / "o.fragmentsizes.txt").read_text() == "\n".join(ref)
