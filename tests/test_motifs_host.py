"""The host side of `pyatac motifs` (nucleoatac_amd/pyatac/get_motifs.py) without a GPU: the two motif file formats, the integer scores,
the exact threshold against brute force over all words, and the argument rules of the command."""
import argparse
import os

import numpy as np
import pytest

import motifs_ref as R
from nucleoatac_amd.pyatac import get_motifs as G

BG = (0.3, 0.2, 0.2, 0.3)


def write(tmp_path, name, text):
    p = str(tmp_path / name)
    with open(p, "w") as fh:
        fh.write(text)
    return p


# ---- the motif files ----------------------------------------------------------------------------------------------------------------
def test_both_formats_give_the_same_counts(tmp_path):
    meme = G.parse_motifs(write(tmp_path, "m.meme", R.meme_text()))
    jaspar = G.parse_motifs(write(tmp_path, "m.jaspar", R.jaspar_text()))
    assert [m[:2] for m in meme] == [m[:2] for m in jaspar] == [(k, v[0]) for k, v in R.EXAMPLE_COUNTS.items()]
    for a, b, (_alt, want) in zip(meme, jaspar, R.EXAMPLE_COUNTS.values()):
        assert a[2].dtype == b[2].dtype == np.float64 and a[2].shape == b[2].shape == want.shape
        assert np.array_equal(b[2], want)                            # counts as written
        assert np.allclose(a[2], want, rtol=0, atol=20 * 5e-7)       # probabilities of six digits times 20 sites
        assert np.array_equal(G.scores(a[2], BG, 0.8), G.scores(b[2], BG, 0.8))


def test_meme_nsites_defaults_to_20(tmp_path):
    text = "MEME version 4\n\nMOTIF m1\nletter-probability matrix: alength= 4 w= 2\n0.5 0.5 0 0\n0 0 0 1\n"
    (mid, alt, c), = G.parse_motifs(write(tmp_path, "m.meme", text))
    assert (mid, alt) == ("m1", "") and np.array_equal(c, [[10, 10, 0, 0], [0, 0, 0, 20]])


def test_comments_and_blank_lines_before_the_first_line(tmp_path):
    text = "# a comment\n\n" + R.jaspar_text()
    assert len(G.parse_motifs(write(tmp_path, "m.txt", text))) == 2


MALFORMED = [
    ("hello\n", 1, "neither"),
    ("MEME version 4\n\nMOTIF\n", 3, "without an id"),
    ("MEME version 4\nMOTIF a\nMOTIF b\n", 3, "no letter-probability matrix"),
    ("MEME version 4\nMOTIF a\nletter-probability matrix: alength= 4 w= 2 nsites= 5\n0.25 0.25 0.25 0.25\n0.5 0.5 x 0\n", 5, "row 2 of 2"),
    ("MEME version 4\nMOTIF a\nletter-probability matrix: alength= 4 w= 1\n0.5 0.5 0.5 0\n", 4, "sum to"),
    ("MEME version 4\nMOTIF a\nletter-probability matrix: alength= 20 w= 1\n", 3, "alength"),
    ("MEME version 4\nMOTIF a\nletter-probability matrix: alength= 4 w= 3\n0.25 0.25 0.25 0.25\n", 4, "ends after 1 of 3"),
    (">a\nA [ 1 2 ]\nC [ 1 2 ]\nT [ 1 2 ]\nG [ 1 2 ]\n", 4, "expected row G"),
    (">a\nA [ 1 2 ]\nC [ 1 2 3 ]\nG [ 1 2 ]\nT [ 1 2 ]\n", 3, "3 columns"),
    (">a\nA [ 1 2 ]\nC [ 1 z ]\nG [ 1 2 ]\nT [ 1 2 ]\n", 3, "not a row of counts"),
    (">a\nA [ 1 2 ]\nC [ 1 2 ]\n", 3, "ends before row G"),
    (">a\nA [ 1 ]\nC [ 1 ]\nG [ 1 ]\nT [ 1 ]\nA [ 1 ]\n", 6, "expected a `>id` header"),
    (">a b\nA [ 1 ]\nC [ 1 ]\nG [ 1 ]\nT [ 1 ]\n>a\nA [ 1 ]\nC [ 1 ]\nG [ 1 ]\nT [ 1 ]\n", 6, "motif id a is already used at line 1"),
    (">a,b\nA [ 1 ]\nC [ 1 ]\nG [ 1 ]\nT [ 1 ]\n", 1, "does not match"),
    (">%s\nA [ 1 ]\nC [ 1 ]\nG [ 1 ]\nT [ 1 ]\n" % ("x" * 65), 1, "does not match"),
    (">wide\n" + "".join("%s [ %s ]\n" % (b, " ".join(["1"] * 65)) for b in "ACGT"), 1, "motif wide: width 65 is outside 1 .. 64"),
    (">empty\nA [ ]\nC [ ]\nG [ ]\nT [ ]\n", 1, "motif empty: width 0"),
]


@pytest.mark.parametrize("text,line,reason", MALFORMED)
def test_malformed_file_names_the_line(tmp_path, text, line, reason):
    path = write(tmp_path, "bad.txt", text)
    with pytest.raises(G.MotifsError) as e:
        G.parse_motifs(path)
    assert str(e.value).startswith("%s: line %d: " % (path, line)), str(e.value)
    assert reason in str(e.value)


def test_too_many_motifs(tmp_path):
    text = "".join(">m%d\nA [ 1 ]\nC [ 1 ]\nG [ 1 ]\nT [ 1 ]\n" % k for k in range(R.MAX_MOTIFS + 1))
    path = write(tmp_path, "many.txt", text)
    with pytest.raises(G.MotifsError) as e:
        G.parse_motifs(path)
    assert str(e.value).startswith("%s: line %d: motif m%d: more than %d motifs" % (path, 5 * R.MAX_MOTIFS + 1, R.MAX_MOTIFS, R.MAX_MOTIFS))


# ---- scores ---------------------------------------------------------------------------------------------------------------------
def test_scores_by_hand():
    # column 1: 8 A of 8 sites, uniform background, pseudocount 0.8: p(A) = 8.2 / 8.8, the others 0.2 / 8.8
    #   100 log2(8.2 / 8.8 / 0.25) = 100 log2(3.72727) = 189.81 -> 190;  100 log2(0.2 / 8.8 / 0.25) = 100 log2(0.0909091) = -345.94 -> -346
    # column 2: 2 of each: p = 2.2 / 8.8 = 0.25 -> 0
    S = G.scores([[8, 0, 0, 0], [2, 2, 2, 2]], [0.25] * 4, 0.8)
    assert S.dtype == np.int32 and S.tolist() == [[190, -346, -346, -346], [0, 0, 0, 0]]
    # a skewed background moves the zero: column 2 with bg (0.4, 0.1, 0.1, 0.4): p(A) = (2 + 0.32) / 8.8 = 0.263636, / 0.4 -> -60.14 -> -60
    #   p(C) = (2 + 0.08) / 8.8 = 0.236364, / 0.1 -> 100 log2(2.36364) = 124.10 -> 124
    S = G.scores([[2, 2, 2, 2]], [0.4, 0.1, 0.1, 0.4], 0.8)
    assert S.tolist() == [[-60, 124, 124, -60]]
    assert np.array_equal(R.scores([[8, 0, 0, 0], [2, 2, 2, 2]]), [[190, -346, -346, -346], [0, 0, 0, 0]])


# ---- thresholds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 5, 8])
def test_threshold_against_brute_force(W):
    rng = np.random.default_rng(40 + W)
    S = G.scores(R.random_counts(rng, W, nsites=30), BG, 0.8)
    tails = R.brute_tails(S, BG)                     # all 4^W words
    lo, hi = int(S.min(axis=1).sum()), int(S.max(axis=1).sum())
    assert min(tails) == lo and max(tails) == hi and abs(tails[lo] - 1.0) < 1e-12

    def tail_at(t):                                  # P(score >= t) for any integer t
        above = [s for s in tails if s >= t]
        return tails[min(above)] if above else 0.0
    for p in (1e-1, 1e-2, 1e-3, 1e-4):
        T, reached, top = G.threshold(S, BG, p)
        assert (T, top) == R.threshold(S, BG, p)[::2] and top == hi
        if reached is None:
            assert T == hi + 1 and tail_at(hi) > p
            continue
        assert abs(reached - tail_at(T)) < 1e-12
        assert tail_at(T) <= p
        assert T == lo or tail_at(T - 1) > p
        assert R.brute_tail(S, BG, T) <= p if W <= 5 else True          # the plain enumeration, where it is quick


def test_threshold_unreachable_for_a_short_motif():
    # four columns under a uniform background: the best word has probability 4^-4 = 0.0039 > 1e-4
    S = G.scores([[20, 0, 0, 0], [0, 20, 0, 0], [0, 0, 20, 0], [0, 0, 0, 20]], [0.25] * 4, 0.8)
    T, reached, top = G.threshold(S, [0.25] * 4, 1e-4)
    assert top == int(S.max(axis=1).sum()) and T == top + 1 and reached is None
    T, reached, _ = G.threshold(S, [0.25] * 4, 4.0 ** -4 + 1e-9)
    # the smallest INTEGER t: one above the second-best word's score (the integers between it and the best are no word's score)
    second = sorted(R.brute_tails(S, [0.25] * 4))[-2]
    assert T == second + 1 and T < top and abs(reached - 4.0 ** -4) < 1e-15


def test_merge_intervals():
    s, e = G.merge_intervals([50, 10, 20, 70, 5, 90], [60, 20, 30, 70, 12, 95])
    assert s.tolist() == [5, 50, 90] and e.tolist() == [30, 60, 95]
    assert R.merged([50, 10, 20, 70, 5, 90], [60, 20, 30, 70, 12, 95]) == [(5, 30), (50, 60), (90, 95)]
    assert [len(a) for a in G.merge_intervals([], [])] == [0, 0]


# ---- the argument rules ---------------------------------------------------------------------------------------------------------------
def args_for(tmp_path, **kw):
    fasta = write(tmp_path, "g.fa", ">chr1\n" + "ACGT" * 25 + "\n>chr2\n" + "GATTACA" * 10 + "\n")
    motifs = write(tmp_path, "m.jaspar", R.jaspar_text())
    out = tmp_path / "out"
    out.mkdir()
    a = dict(fasta=fasta, motifs=motifs, bed=None, only=None, pvalue=1e-4, pseudocount=0.8, bg=["uniform"], format="mtx", no_sites=False,
             out=str(out / "run"))
    a.update(kw)
    return argparse.Namespace(**a), str(out)


@pytest.mark.parametrize("kw,reason", [
    (dict(pvalue=0.0), "--pvalue"), (dict(pvalue=1.0), "--pvalue"), (dict(pvalue=-0.5), "--pvalue"),
    (dict(pseudocount=0.0), "--pseudocount"), (dict(pseudocount=-1.0), "--pseudocount"),
    (dict(bg=["0.3", "0.3", "0.3", "0.3"]), "--bg"), (dict(bg=["0.5", "0.5", "0", "0"]), "--bg"), (dict(bg=["0.5", "0.5"]), "--bg"),
    (dict(bg=["gc"]), "--bg"), (dict(format="csv"), "--format"),
    (dict(only=["MA0001.1", "nope"]), "no motif nope"),
    (dict(fasta="/nonexistent/g.fa"), "no such file"), (dict(motifs="/nonexistent/m"), "no such file"), (dict(bed="/nonexistent/b"), "no such file"),
])
def test_argument_rules(tmp_path, kw, reason):
    args, out = args_for(tmp_path, **kw)
    with pytest.raises(G.MotifsError) as e:
        G.get_motifs(args)
    assert reason in str(e.value)
    assert os.listdir(out) == []


def test_malformed_motif_file_writes_nothing(tmp_path):
    args, out = args_for(tmp_path, motifs=write(tmp_path, "bad.meme", "MEME version 4\nMOTIF a\nMOTIF b\n"))
    with pytest.raises(G.MotifsError) as e:
        G.get_motifs(args)
    assert ": line 3: " in str(e.value) and os.listdir(out) == []


def test_window_past_the_chromosome_end(tmp_path):
    bed = write(tmp_path, "w.bed", "chr1\t10\t50\nchr2\t60\t71\n")            # chr2 has 70 bases
    args, out = args_for(tmp_path, bed=bed)
    with pytest.raises(G.MotifsError) as e:
        G.get_motifs(args)
    assert "chr2:60-71" in str(e.value) and os.listdir(out) == []


def test_bed_rows_kept_in_order_and_unknown_chromosomes_dropped(tmp_path):
    from nucleoatac_amd.pyatac.seq import FastaStore
    args, _ = args_for(tmp_path)
    bed = write(tmp_path, "w.bed", "chr2\t5\t20\nchrX\t1\t9\nchr1\t7\t7\nchr1\t30\t90\nchr2\t0\t70\n")
    with pytest.warns(UserWarning, match="chrX"):
        fc, start, end = G.read_windows(bed, FastaStore.open(args.fasta))
    assert fc.tolist() == [1, 0, 1] and start.tolist() == [5, 30, 0] and end.tolist() == [20, 90, 70]      # the zero-length row is gone
    fc, start, end = G.read_windows(None, FastaStore.open(args.fasta))
    assert fc.tolist() == [0, 1] and start.tolist() == [0, 0] and end.tolist() == [100, 70]


def test_cli_reports_one_line(tmp_path, capsys):
    from nucleoatac_amd.pyatac.cli import main
    args, out = args_for(tmp_path)
    rc = main(["motifs", "--fasta", args.fasta, "--motifs", args.motifs, "--pvalue", "2", "--out", args.out])
    err = capsys.readouterr().err
    assert rc == 1 and err.startswith("pyatac motifs: --pvalue") and err.count("\n") == 1 and os.listdir(out) == []
