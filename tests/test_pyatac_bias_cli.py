"""`pyatac bias` (nucleoatac_amd/pyatac/cli.py, make_bias_track.py) without a GPU: the parser's flags and defaults against the
reference's (pyatac/cli.py:133-152), the default output names (make_bias_track.py:61-65), and the region / trim function against the
reference's own outputs (tests/golden/pyatac_bias.npz, made by tests/golden/make_golden_bias.py): for every golden case the trimmed
track intervals cover exactly the bases the reference's text covers and every interval boundary is a line boundary there.  BED regions
on a chromosome the FASTA lacks are dropped with a warning; regions whose trimmed interval is empty are set aside."""
import argparse
import gzip
import warnings

import numpy as np
import pytest

from conftest import load_golden

G = load_golden("pyatac_bias")
CASES = [str(x) for x in G["cases"]]
SIZES = dict(zip([str(x) for x in G["chrom_names"]], [int(x) for x in G["chrom_lengths"]]))


def golden_text(key):
    return gzip.decompress(G["text_" + key].tobytes()).decode("ascii")


def case_pwm(key, tmp_path):
    """the --pwm argument of a golden case: a built-in name, or the stored asymmetric descriptor written to a file"""
    pwm = str(G["args_" + key][1])
    if pwm != "asym":
        return pwm
    p = tmp_path / "asym.PWM.txt"
    p.write_text(str(G["asym_pwm_text"]))
    return str(p)


def test_bias_flags_and_defaults():
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    p = pyatac_parser()
    a = p.parse_args(["bias", "--fasta", "g.fa"])
    assert (a.call, a.fasta, a.pwm, a.bed, a.out, a.cores) == ("bias", "g.fa", "Human", None, None, 1)
    a = p.parse_args(["bias", "--fasta", "g.fa", "--pwm", "my.PWM.txt", "--bed", "r.bed", "--out", "o", "--cores", "8"])
    assert (a.fasta, a.pwm, a.bed, a.out, a.cores) == ("g.fa", "my.PWM.txt", "r.bed", "o", 8)
    for bad in (["bias"], ["bias", "--pwm", "Human"], ["bias", "--fasta", "g.fa", "--bam", "x.bam"],
                ["bias", "--fasta", "g.fa", "--smooth", "3"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_default_out_names():
    from nucleoatac_amd.pyatac.make_bias_track import default_out
    ns = lambda **k: argparse.Namespace(**dict(dict(out=None, bed=None, fasta="dir/hg19.fa"), **k))
    assert default_out(ns()) == "hg19"
    assert default_out(ns(fasta="dir/genome.fa.gz")) == "genome.fa"
    assert default_out(ns(bed="x/peaks.narrow.bed")) == "peaks.narrow"
    assert default_out(ns(out="given", bed="x/peaks.bed")) == "given"
    assert default_out(ns(fasta="noext")) == ""


def _covered(text):
    out = {c: np.zeros(n, bool) for c, n in SIZES.items()}
    starts, ends = set(), set()
    for line in text.splitlines():
        c, s, e, _ = line.split("\t")
        assert not out[c][int(s):int(e)].any(), line          # the reference writes no base twice
        out[c][int(s):int(e)] = True
        starts.add((c, int(s)))
        ends.add((c, int(e)))
    return out, starts, ends


@pytest.mark.parametrize("key", CASES)
def test_trimmed_regions_are_what_the_reference_text_covers(tmp_path, key):
    from nucleoatac_amd.pyatac.bias import PWM
    from nucleoatac_amd.pyatac.make_bias_track import bias_regions
    pwm = PWM.open(case_pwm(key, tmp_path))
    bed = None
    if str(G["args_" + key][0]) == "bed":
        bed = str(tmp_path / "regions.bed")
        with open(bed, "w") as f:
            f.write(str(G["bed_text"]))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tracks, empty = bias_regions(SIZES, pwm.up, pwm.down, bed)
    dropped = [str(w.message) for w in caught if "not included in" in str(w.message)]
    if bed is None:
        assert not dropped
        assert len(tracks) == sum((n + 999) // 1000 for n in SIZES.values())
    else:
        assert len(dropped) == 1 and "chrZ" in dropped[0]
        assert all(c.chrom != "chrZ" for c in tracks)
    assert empty == []                                          # the golden grid holds no empty trimmed interval
    want, starts, ends = _covered(golden_text(key))
    mine = {c: np.zeros(n, bool) for c, n in SIZES.items()}
    order = [(c.chrom, c.start) for c in tracks]
    assert order == sorted(order)
    for c in tracks:
        assert 0 <= c.start < c.end <= SIZES[c.chrom]
        assert not mine[c.chrom][c.start:c.end].any()
        mine[c.chrom][c.start:c.end] = True
        assert (c.chrom, c.start) in starts and (c.chrom, c.end) in ends   # lines break at every region boundary
    for c in SIZES:
        assert np.array_equal(mine[c], want[c]), (key, c)


def test_first_track_starts_at_up_and_last_ends_at_length_minus_down():
    from nucleoatac_amd.pyatac.make_bias_track import bias_regions
    tracks, empty = bias_regions({"c2": 2500, "c1": 1000}, 7, 12)
    assert [(c.chrom, c.start, c.end) for c in tracks] == [("c1", 7, 988), ("c2", 7, 1000), ("c2", 1000, 2000), ("c2", 2000, 2488)]
    assert empty == []


def test_empty_trimmed_intervals_are_set_aside(tmp_path):
    """the deliberate divergence: the reference raises on these; here they are returned apart and write nothing"""
    from nucleoatac_amd.pyatac.make_bias_track import bias_regions
    # a last chunk of 5 <= down bases; a chromosome of exactly up + down bases; one of up + down + 1 has a single value
    tracks, empty = bias_regions({"a": 3005, "b": 20, "c": 21}, 10, 10)
    assert [(c.chrom, c.start, c.end) for c in tracks] == [("a", 10, 1000), ("a", 1000, 2000), ("a", 2000, 2995), ("c", 10, 11)]
    assert [(c.chrom, c.start, c.end) for c in empty] == [("a", 3000, 3005), ("b", 0, 20)]
    bed = tmp_path / "r.bed"
    bed.write_text("a\t3005\t3100\na\t2996\t3000\na\t2980\t2990\na\t2994\t2996\n")
    tracks, empty = bias_regions({"a": 3005}, 10, 10, str(bed))
    # [2994, 2996) keeps the one base before L - down; [2996, 3000) starts past L - down and [3005, 3100) at L
    assert [(c.chrom, c.start, c.end) for c in tracks] == [("a", 2980, 2990), ("a", 2994, 2995)]
    assert [(c.chrom, c.start, c.end) for c in empty] == [("a", 2996, 3000), ("a", 3005, 3100)]


def test_bed_regions_on_missing_chromosomes_are_dropped_with_a_warning(tmp_path):
    from nucleoatac_amd.pyatac.make_bias_track import bias_regions
    bed = tmp_path / "r.bed"
    bed.write_text("chrQ\t5\t50\nchrA\t100\t300\nchrP\t0\t10\n")
    with pytest.warns(UserWarning, match="2 chromosome names in bed file not included in fasta file") as rec:
        tracks, empty = bias_regions({"chrA": 1000}, 10, 10, str(bed))
    assert "chrP" in str(rec[0].message) and "chrQ" in str(rec[0].message)
    assert [(c.chrom, c.start, c.end) for c in tracks] == [("chrA", 100, 300)] and empty == []
