"""`pyatac nucleotide` on the GPU (natac_site_seq_counts; nucleoatac_amd/pyatac/get_nucleotide.py) against the reference's own
outputs (tests/golden/pyatac_sites.npz, made by tests/golden/make_golden_sites.py): the .nucfreq.txt of every case equals the
reference's byte for byte and the returned matrix equals the stored float64 matrix bit for bit -- integer counts and one or two IEEE
divisions in the reference's order, no tolerance.  The kernel against the NumPy restatement of tests/sites_ref.py on seeded inputs
that cross every arm of the launch geometry: windows of 1, 2, 64, 65, 501, 512, 513 and 10,001 columns (SS_TILE = 512 columns per
block), word lengths 1 and 2, site counts either side of the SS_SEG = 4096 sites a block takes between two flushes, any split of
the sites into calls.  A text FASTA gives what the .npz store gives; the error exits and NATAC_E_ARG."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import sites_ref as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

G = load_golden("pyatac_sites")
CASES = [str(x) for x in G["nuc_cases"]]
NAMES = [str(x) for x in G["chrom_names"]]
SEQS = {c: G["seq_" + c] for c in NAMES}
SS_SEG, SS_TILE = 4096, 512


def golden_text(key):
    return gzip.decompress(G["text_" + key].tobytes()).decode("ascii")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("nuc_inputs")
    bed = str(d / "sites.bed")
    with open(bed, "w") as f:
        f.write(str(G["bed_text"]))
    fasta = str(d / "genome.npz")
    np.savez(fasta, chrom_names=G["chrom_names"], chrom_lengths=G["chrom_lengths"], **{"seq_" + c: SEQS[c] for c in NAMES})
    text = str(d / "genome.fa")
    with open(text, "wb") as f:
        f.write(R.fasta_text(NAMES, SEQS, int(G["fasta_line_width"])))
    return d, bed, fasta, text


def case_argv(key, fasta, bed, out):
    di, strand, norm, up, down = [int(x) for x in G["args_" + key]]
    return (["nucleotide", "--fasta", fasta, "--bed", bed, "--out", out, "--up", str(up), "--down", str(down)] +
            (["--dinucleotide"] if di else []) + (["--strand", str(strand)] if strand else []) + (["--norm"] if norm else []))


def run_cli(argv, timeout=300):
    return subprocess.run([sys.executable, "-m", "nucleoatac_amd.pyatac.cli"] + argv, cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout)


def needs_text(key):
    di, _, norm, _, _ = [int(x) for x in G["args_" + key]]
    return bool(di and norm)


@pytest.mark.parametrize("key", CASES)
def test_file_equals_the_references_byte_for_byte(inputs, key):
    d, bed, fasta, text = inputs
    r = run_cli(case_argv(key, text if needs_text(key) else fasta, bed, str(d / key)))
    assert r.returncode == 0, (key, r.stdout[-2000:], r.stderr[-2000:])
    used = G["used_" + key]
    assert "%d sites used, %d skipped" % (used.sum(), len(used) - used.sum()) in r.stdout
    with open(str(d / key) + ".nucfreq.txt", "rb") as f:
        assert f.read().decode("ascii") == golden_text(key), key


@pytest.mark.parametrize("key", CASES)
def test_text_fasta_and_store_agree_and_the_matrix_is_bit_identical(inputs, tmp_path, key):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    from nucleoatac_amd.pyatac.get_nucleotide import get_nucleotide
    _, bed, fasta, text = inputs
    for tag, src in (("text", text),) + ((() if needs_text(key) else (("npz", fasta),))):
        out = str(tmp_path / tag)
        result = get_nucleotide(pyatac_parser().parse_args(case_argv(key, src, bed, out)))
        assert result.dtype == np.float64 and np.array_equal(result, G["mat_" + key]), (key, tag)
        with open(out + ".nucfreq.txt") as f:
            assert f.read() == golden_text(key), (key, tag)


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _genome(rng, n):
    s = rng.choice(np.frombuffer(b"ACGTacgtNnRy", np.uint8), size=n, p=[0.18] * 4 + [0.05] * 4 + [0.03, 0.02, 0.02, 0.01])
    s[n // 3:n // 3 + 700] = ord("N")
    return s


GEOMETRY = [  # (up, down, sites): up + down + 1 columns
    (0, 0, 5000), (1, 0, 5000), (0, 1, 70), (31, 32, 4095), (32, 32, 4096), (3, 61, 4097), (250, 250, 3 * 4096 + 5), (255, 256, 300),
    (256, 256, 4100), (100, 412, 40), (5000, 5000, 900), (700, 9300, 64),
]


@pytest.mark.parametrize("word", [1, 2])
@pytest.mark.parametrize("up, down, ns", GEOMETRY)
def test_kernel_matches_numpy_across_the_launch_geometry(up, down, ns, word):
    rng = np.random.default_rng(1000 * up + down + 7 * word)
    n = 60000
    seq = _genome(rng, n)
    centers = rng.integers(0, n, size=ns)
    centers[:min(ns, 6)] = [0, n - 1, up, n - down - word, max(up - 1, 0), min(n - down - word + 1, n - 1)][:min(ns, 6)]   # both edges
    minus = rng.random(ns) < 0.5
    want, n_want = R.site_counts_ref(seq, centers, minus, up, down, word)
    got, n_got, ms = _ctx().site_seq_counts(seq, centers, minus, up, down, word, with_kernel_ms=True)
    assert got.shape == (16 if word == 2 else 4, up + down + 1) and got.dtype == np.int64
    assert n_got == n_want and np.array_equal(got, want) and ms > 0
    if ns > 100:
        assert 0 < n_want < ns or up + down == 0
    # all plus through minus=None; and however the sites are split into calls
    p_want, p_n = R.site_counts_ref(seq, centers, None, up, down, word)
    p_got, p_got_n = _ctx().site_seq_counts(seq, centers, None, up, down, word)
    assert p_got_n == p_n and np.array_equal(p_got, p_want)
    parts = [np.arange(0, ns // 3), np.arange(ns // 3, ns // 3 + 1), np.arange(ns // 3 + 1, ns)]
    tot, tot_n = 0, 0
    for p in parts:
        m, k = _ctx().site_seq_counts(seq, centers[p], minus[p], up, down, word)
        tot, tot_n = tot + m, tot_n + k
    assert tot_n == n_want and np.array_equal(tot, want)


def test_no_site_and_a_chromosome_shorter_than_the_window():
    seq = np.frombuffer(b"ACGTTGCAAC", np.uint8)
    m, n = _ctx().site_seq_counts(seq, np.zeros(0, np.int64), None, 2, 2, 1)
    assert n == 0 and m.shape == (4, 5) and not m.any()
    m, n = _ctx().site_seq_counts(seq, np.arange(10), np.arange(10) % 2, 6, 6, 2)          # every window is clipped
    assert n == 0 and m.shape == (16, 13) and not m.any()
    m, n = _ctx().site_seq_counts(seq, [4], [1], 5, 4, 1)                                    # the whole chromosome, reversed
    want = "GTTGCAACGT"
    assert n == 1 and ["ACGT"[int(np.argmax(m[:, j]))] for j in range(10)] == list(want) and m.sum() == 10


def test_error_exits(inputs, tmp_path):
    _, bed, fasta, _ = inputs
    out = str(tmp_path / "o")

    def refused(argv, word):
        r = run_cli(argv + ["--out", out])
        err = [x for x in r.stderr.splitlines() if x.strip()]
        assert r.returncode == 1 and len(err) == 1 and word in err[0], (argv, r.stderr[-2000:])
        assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")]
    refused(["nucleotide", "--fasta", fasta, "--bed", bed, "--up", "-3"], "--up")
    refused(["nucleotide", "--fasta", fasta, "--bed", bed, "--dinucleotide", "--norm"], "no lines")
    refused(["nucleotide", "--fasta", fasta, "--bed", bed, "--strand", "7"], "line 1")
    other = tmp_path / "other.bed"
    other.write_text("chrA\t10\t20\nchrQ\t5\t50\n")
    refused(["nucleotide", "--fasta", fasta, "--bed", str(other)], "chrQ")
    clipped = tmp_path / "clipped.bed"
    clipped.write_text("chrA\t10\t20\nchrC\t5\t50\nchrA\t3990\t4000\n")       # on the chromosomes, every default window clipped
    refused(["nucleotide", "--fasta", fasta, "--bed", str(clipped)], "no site")


def test_bad_arguments_are_refused():
    import ctypes as C
    from nucleoatac_amd import _lib as Lb
    lib, h = Lb.load(), _ctx()._h
    seq = np.frombuffer(b"ACGTACGTAC" * 5, np.uint8).copy()
    cen = np.array([10, 20, 49], np.int64)
    out = np.full((4, 5), -7, np.int64)
    n = C.c_int64(-7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(h_=h, s=seq, ln=50, ns=3, c=cen, up=2, down=2, word=1, o=out, nn=n):
        return lib.natac_site_seq_counts(h_, None if s is None else vp(s), ln, ns, None if c is None else vp(c), None, up, down, word,
                                         None if o is None else vp(o), None if nn is None else C.byref(nn), None)
    assert call() == 0 and n.value == 2 and out.sum() == 10
    for kw in (dict(h_=None), dict(s=None), dict(c=None), dict(o=None), dict(nn=None), dict(ln=-1), dict(ns=-1), dict(up=-1),
               dict(down=-1), dict(word=0), dict(word=3), dict(up=1 << 20), dict(c=np.array([10, 50, 20], np.int64)),
               dict(c=np.array([-1, 10, 20], np.int64))):
        assert call(**kw) == -1, kw                     # NATAC_E_ARG
        assert lib.natac_last_error(), kw
    with pytest.raises(Lb.NatacError) as err:
        _ctx().site_seq_counts(seq, [50], None, 2, 2)
    assert err.value.code == -1 and "centre" in str(err.value)
    with pytest.raises(ValueError):
        _ctx().site_seq_counts(seq, cen, [0, 1], 2, 2)
