"""`pyatac ins | cov` (nucleoatac_amd/pyatac/cli.py, trackfiles.py) without a GPU: the parsers' flags and defaults against the reference's
(pyatac/cli.py:310-352), the default output names (get_ins.py:66-70), the genome-wide region list (1-kb chunks, chromosomes by name, short
last chunks), the merged BED list, the Gaussian window, and the refusal of a BED region on a chromosome the BAM lacks."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_ins_and_cov_flags_and_defaults():
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    p = pyatac_parser()
    a = p.parse_args(["ins", "--bam", "x.bam"])
    assert (a.call, a.bam, a.bed, a.out, a.cores, a.lower, a.upper, a.smooth, a.atac) == ("ins", "x.bam", None, None, 1, 0, 2000, None, True)
    a = p.parse_args(["ins", "--bam", "x.bam", "--bed", "r.bed", "--out", "o", "--cores", "4", "--lower", "3", "--upper", "500",
                      "--smooth", "75", "--not_atac"])
    assert (a.bed, a.out, a.cores, a.lower, a.upper, a.smooth, a.atac) == ("r.bed", "o", 4, 3, 500, 75, False)
    a = p.parse_args(["cov", "--bam", "x.bam"])
    assert (a.call, a.bam, a.bed, a.out, a.cores, a.lower, a.upper, a.window, a.scale, a.atac) == \
        ("cov", "x.bam", None, None, 1, 0, 2000, 121, 10, True)
    a = p.parse_args(["cov", "--bam", "x.bam", "--bed", "r.bed", "--window", "100", "--scale", "1", "--lower", "50", "--upper", "300",
                      "--not_atac", "--out", "o"])
    assert (a.bed, a.window, a.scale, a.lower, a.upper, a.atac, a.out) == ("r.bed", 100, 1.0, 50, 300, False, "o")
    for bad in (["ins"], ["cov"], ["cov", "--bam", "x.bam", "--smooth", "3"], ["ins", "--bam", "x.bam", "--window", "3"],
                ["vplot", "--bam", "x.bam"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_default_out_names():
    import argparse
    from nucleoatac_amd.pyatac.trackfiles import default_out
    ns = lambda **k: argparse.Namespace(**dict(dict(out=None, bed=None, bam="dir/sample.sorted.bam"), **k))
    assert default_out(ns()) == "sample.sorted"
    assert default_out(ns(bed="x/peaks.bed")) == "peaks"
    assert default_out(ns(bed="x/peaks.bed.gz")) == "peaks.bed"
    assert default_out(ns(out="given")) == "given"
    assert default_out(ns(bam="noext")) == ""


def _reads_npz(path, chroms):
    arrs = {"chrom_names": np.array(list(chroms)), "chrom_lengths": np.array(list(chroms.values()))}
    for c in chroms:
        arrs["pos_" + c] = np.array([5, 10], np.int64)
        arrs["tlen_" + c] = np.array([100, -60], np.int64)
    np.savez(path, **arrs)


def test_genome_regions_are_the_references_1kb_chunks(tmp_path):
    from nucleoatac_amd.pyatac.trackfiles import track_regions
    bam = str(tmp_path / "reads.npz")
    _reads_npz(bam, {"chrB": 2500, "chr10": 1000, "chrA": 999, "chr2": 1})
    r = [(c.chrom, c.start, c.end) for c in track_regions(bam)]
    assert r == [("chr10", 0, 1000), ("chr2", 0, 1), ("chrA", 0, 999), ("chrB", 0, 1000), ("chrB", 1000, 2000), ("chrB", 2000, 2500)]


def test_bed_regions_are_merged_not_clipped(tmp_path):
    from nucleoatac_amd.pyatac.trackfiles import track_regions
    bam = str(tmp_path / "reads.npz")
    _reads_npz(bam, {"chrA": 1000, "chrB": 500})
    bed = tmp_path / "r.bed"
    bed.write_text("chrB\t400\t700\nchrA\t100\t300\nchrA\t250\t400\nchrA\t400\t450\nchrA\t10\t20\nchrA\t900\t1200\nchrA\t5\t5\n")
    r = [(c.chrom, c.start, c.end) for c in track_regions(bam, str(bed))]
    # overlapping regions merge, touching ones do not (ChunkList.merge, sep = -1); nothing is clipped to the chromosome; empty ones drop
    assert r == [("chrA", 10, 20), ("chrA", 100, 400), ("chrA", 400, 450), ("chrA", 900, 1200), ("chrB", 400, 700)]


def test_gaussian_window_is_utils_smooth_window():
    from scipy import signal
    from nucleoatac_amd.pyatac.trackfiles import gaussian_window
    for S, M in ((1, 1), (10, 11), (21, 21), (301, 301)):
        w, wsum = gaussian_window(S)
        assert np.array_equal(w, signal.windows.gaussian(M, (M - 1) / 6.0))
        assert wsum == np.convolve(w, np.ones(M), "valid")[0]
    assert np.array_equal(gaussian_window(1)[0], [1.0])


@pytest.mark.parametrize("call", ["ins", "cov"])
def test_bed_on_a_missing_chromosome_is_refused(tmp_path, call):
    bam = str(tmp_path / "reads.npz")
    _reads_npz(bam, {"chrA": 1000})
    bed = tmp_path / "r.bed"
    bed.write_text("chrA\t100\t300\nchrZ\t10\t20\n")
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "nucleoatac_amd.pyatac.cli", call, "--bam", bam, "--bed", str(bed), "--out", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "chrZ" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")]
