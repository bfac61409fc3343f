"""`pyatac bias` on the GPU (natac_run_pwm_track; nucleoatac_amd/pyatac/make_bias_track.py) against the reference's own outputs
(tests/golden/pyatac_bias.npz, made by tests/golden/make_golden_bias.py): the same chromosomes and covered bases, every value within
the tight tier (1e-10 relative + 1e-12; the kernel's association and scipy's direct correlate differ in the last bit, so neither the
bytes nor the line boundaries are compared with the reference).  The line structure is compared with ourselves: the file's text is the
host writer's text of the downloaded track, byte for byte.  NATAC_T_BIAS is bit-identical to natac_pwm_bias on the same windows for
chunks of 1, 1023, 1024, 1025 and 1,000,003 bases and PWMs of 1, 20, 21 and 300 columns with 4, 5 and 2 rows.  The output does not
depend on the sub-batching, the .tbi answers region queries with the text's lines, regions with an empty trimmed interval write no
line and warn, a k-mer PWM exits 1 without a file, and bad arguments are NATAC_E_ARG."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import TIGHT_ATOL, TIGHT_RTOL

pytestmark = pytest.mark.gpu

G = load_golden("pyatac_bias")
CASES = [str(x) for x in G["cases"]]
NAMES = [str(x) for x in G["chrom_names"]]
SIZES = dict(zip(NAMES, [int(x) for x in G["chrom_lengths"]]))


def golden_text(key):
    return gzip.decompress(G["text_" + key].tobytes()).decode("ascii")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bias_inputs")
    fasta = str(d / "genome.npz")
    np.savez(fasta, chrom_names=G["chrom_names"], chrom_lengths=G["chrom_lengths"], **{"seq_" + c: G["seq_" + c] for c in NAMES})
    bed = str(d / "regions.bed")
    with open(bed, "w") as f:
        f.write(str(G["bed_text"]))
    asym = str(d / "asym.PWM.txt")
    with open(asym, "w") as f:
        f.write(str(G["asym_pwm_text"]))
    return d, fasta, bed, asym


def case_argv(key, inputs, out):
    _, fasta, bed, asym = inputs
    region, pwm = [str(x) for x in G["args_" + key]]
    argv = ["bias", "--fasta", fasta, "--pwm", asym if pwm == "asym" else pwm, "--out", out]
    if region == "bed":
        argv += ["--bed", bed]
    return argv


def run_cli(argv, timeout=300):
    return subprocess.run([sys.executable, "-m", "nucleoatac_amd.pyatac.cli"] + argv, cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout)


@pytest.fixture(scope="module")
def cli_outputs(inputs):
    """every golden case through `python -m nucleoatac_amd.pyatac.cli bias`, each in its own subprocess with a time limit"""
    d = inputs[0]
    out = {}
    for key in CASES:
        r = run_cli(case_argv(key, inputs, str(d / key)))
        assert r.returncode == 0, (key, r.stdout[-2000:], r.stderr[-2000:])
        assert "---------Making Tn5 Bias Track" in r.stdout
        assert ("chrZ" in r.stderr) == key.startswith("bed_"), (key, r.stderr[-2000:])     # the dropped chromosome is named
        assert "wrote no lines" not in r.stderr, key
        out[key] = str(d / key) + ".Scores.bedgraph.gz"
    return out


def per_base(text):
    """{chrom: (covered mask, values)} of a bedGraph text"""
    out = {}
    for line in text.splitlines():
        c, s, e, v = line.split("\t")
        s, e = int(s), int(e)
        if c not in out:
            out[c] = (np.zeros(SIZES[c], bool), np.zeros(SIZES[c]))
        assert not out[c][0][s:e].any(), line
        out[c][0][s:e] = True
        out[c][1][s:e] = float(v)
    return out


@pytest.mark.parametrize("key", CASES)
def test_text_matches_the_reference(cli_outputs, key):
    with gzip.open(cli_outputs[key], "rt") as f:
        mine = f.read()
    a, b = per_base(mine), per_base(golden_text(key))
    assert sorted(a) == sorted(b), key
    for c in a:
        assert np.array_equal(a[c][0], b[c][0]), (key, c)
        m = a[c][0]
        d = np.abs(a[c][1][m] - b[c][1][m])
        print("%s %s: %d bases, max |d| = %.3g, max |d| / (rtol |ref| + atol) = %.3g" % (
            key, c, int(m.sum()), d.max(), (d / (TIGHT_RTOL * np.abs(b[c][1][m]) + TIGHT_ATOL)).max()))
        np.testing.assert_allclose(a[c][1][m], b[c][1][m], rtol=TIGHT_RTOL, atol=TIGHT_ATOL, err_msg=key)


def _case_batch(key, inputs):
    """(pk, logp, nucs): every trimmed region of a golden case as one fragment-free batch"""
    from nucleoatac_amd.pyatac.bias import PWM
    from nucleoatac_amd.pyatac.make_bias_track import bias_regions, pack_seq_windows
    from nucleoatac_amd.pyatac.seq import FastaStore
    argv = case_argv(key, inputs, "unused")
    pwm = PWM.open(argv[argv.index("--pwm") + 1])
    fs = FastaStore.open(inputs[1])
    tracks, empty = bias_regions(fs.chrom_sizes(), pwm.up, pwm.down, argv[argv.index("--bed") + 1] if "--bed" in argv else None)
    assert not empty
    return pack_seq_windows(tracks, fs, pwm.up, pwm.down), pwm


@pytest.mark.parametrize("key", CASES)
def test_line_structure_is_the_host_writers(cli_outputs, inputs, tmp_path, key):
    from nucleoatac_amd import _lib as Lb
    from nucleoatac_amd import get_context
    from nucleoatac_amd.writer import write_bedgraph
    pk, pwm = _case_batch(key, inputs)
    b = get_context().upload(pk)
    try:
        b.run_pwm_track(pk.track_seq_off, pk.track_seq, np.log(pwm.mat), pwm.nucleotides)
        vals = b.track(Lb.T_BIAS).copy()
    finally:
        b.free()
    host = str(tmp_path / "host.bedgraph")
    write_bedgraph(host, pk.chroms, pk.chunk_start, pk.out_off, vals)
    with gzip.open(cli_outputs[key], "rb") as f:
        mine = f.read()
    with open(host, "rb") as f:
        assert mine == f.read(), key
    # the homopolymer and all-N stretches of the golden genome: equal neighbours are exactly equal, one line each
    if key.startswith("genome_"):
        assert any(int(x.split("\t")[2]) - int(x.split("\t")[1]) >= 30 for x in mine.decode().splitlines() if x.startswith("chrA\t5"))
        assert any(x.endswith("\t0.0") and int(x.split("\t")[2]) - int(x.split("\t")[1]) >= 5 for x in mine.decode().splitlines())


def _random_pwm(rng, nrow, K):
    return np.exp(rng.normal(0.0, 0.5, size=(nrow, K)))


GEOMETRY = [  # (chunk lengths, nrow, K)
    ([1, 1023, 1024, 1025, 2048, 2049, 7], 4, 21),
    ([1, 1024, 1025, 3000], 4, 20),               # up != down: 7 + 12 + 1 columns
    ([1, 5, 1024, 1300], 4, 1),
    ([1, 1023, 1025, 2500], 5, 21),               # N as a fifth row letter
    ([1, 1024, 4100], 2, 300),                    # an overhang longer than a stride of the staging loop
    ([1000003], 4, 21),
    ([1000003, 3], 5, 20),
]


@pytest.mark.parametrize("lens, nrow, K", GEOMETRY)
def test_track_is_bit_identical_to_pwm_bias(lens, nrow, K):
    from nucleoatac_amd import _lib as Lb
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.make_bias_track import SeqTrackChunks
    rng = np.random.default_rng(1000 * K + nrow + len(lens))
    nucs = ["A", "C", "G", "T", "N"][:nrow]
    mat = _random_pwm(rng, nrow, K)
    nc = len(lens)
    wins = [rng.choice(np.frombuffer(b"ACGTNacgtnRy", np.uint8), size=n + K - 1, p=[0.2, 0.2, 0.2, 0.2, 0.04] + [0.03] * 4 + [0.02, 0.01, 0.01])
            for n in lens]
    marked = [n >= 50 + 6 * K for n in lens]
    for w, m in zip(wins, marked):
        if m:
            w[50:50 + 3 * K] = ord("A")            # a homopolymer stretch
            w[-2 * K:] = ord("n")                  # and a soft-masked run of N at the end
    off = np.concatenate(([0], np.cumsum([len(w) for w in wins]))).astype(np.int64)
    pk = SeqTrackChunks(chunk_start=np.arange(nc, dtype=np.int64) * 2000000, chunk_len=np.array(lens, np.int32),
                        frag_off=np.zeros(nc + 1, np.int64), frag_lpos=np.zeros(0, np.int32), frag_ilen=np.zeros(0, np.int32), bias_off=None,
                        bias_log=None, chroms=["c"] * nc, track_seq_off=off, track_seq=np.concatenate(wins))
    ctx = get_context()
    b = ctx.upload(pk)
    try:
        b.run_pwm_track(pk.track_seq_off, pk.track_seq, np.log(mat), nucs)
        got = b.split(b.track(Lb.T_BIAS))
    finally:
        b.free()
    for i, w in enumerate(wins):
        want = ctx.pwm_bias(np.frombuffer(w.tobytes().upper(), np.uint8), mat, nucs)     # natac_pwm_score reads upper case only
        assert got[i].shape == want.shape == (lens[i],)
        assert np.array_equal(got[i], want), (i, lens[i])
        if marked[i]:
            assert np.all(got[i][50:50 + 2 * K] == got[i][50]) and np.all(got[i][-K:] == got[i][-1])
    assert any(np.abs(g).max() > 0 for g in got)


def _run_in_process(argv, **kw):
    import argparse
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    from nucleoatac_amd.pyatac.make_bias_track import make_bias_track
    args = pyatac_parser().parse_args(argv)
    assert isinstance(args, argparse.Namespace)
    path = make_bias_track(args, **kw)
    with open(path, "rb") as f:
        raw = f.read()
    with open(path + ".tbi", "rb") as f:
        return raw, f.read()


@pytest.mark.parametrize("key", ["genome_Human", "bed_asym"])
def test_independent_of_sub_batching(cli_outputs, inputs, tmp_path, key):
    with open(cli_outputs[key], "rb") as f:
        want = f.read()
    with gzip.open(cli_outputs[key], "rb") as f:
        want_text = f.read()
    timing = {}
    raw, _ = _run_in_process(case_argv(key, inputs, str(tmp_path / "d")), timing=timing)
    assert raw == want and timing["sub_batches"] == 1
    for mc in (1, 7):
        timing = {}
        raw, _ = _run_in_process(case_argv(key, inputs, str(tmp_path / ("m%d" % mc))), max_chunks=mc, timing=timing)
        assert timing["sub_batches"] > (1 if mc == 1 else 0)          # 7 regions genome-wide: one region, or all, per sub-batch
        assert gzip.decompress(raw) == want_text, (key, mc)


def test_tabix_index_answers_region_queries(cli_outputs):
    from nucleoatac_amd.tabix import TabixFile
    for key in CASES:
        path = cli_outputs[key]
        assert os.path.exists(path + ".tbi"), key
        with gzip.open(path, "rt") as f:
            lines = f.read().splitlines()
        tb = TabixFile(path)
        try:
            for c in NAMES:
                n = SIZES[c]
                for s, e in ((0, n), (0, 1), (0, 11), (n // 3, n // 2 + 7), (999, 1001), (max(0, n - 5), n + 500)):
                    want = [x for x in lines if x.split("\t")[0] == c and int(x.split("\t")[2]) > s and int(x.split("\t")[1]) < e]
                    assert list(tb.fetch(c, s, e)) == want, (key, c, s, e)
        finally:
            tb.close()


def test_empty_trimmed_intervals_write_no_line_and_warn(tmp_path):
    """the deliberate divergence from the reference, which raises in Track.write_track on these regions: a last chunk of 5 <= down bases
    (chrA, 3005 bases), a chromosome of up + down bases (chrS) and, with --bed, a region that starts at the chromosome's end"""
    rng = np.random.default_rng(5)
    sizes = {"chrA": 3005, "chrS": 20, "chrT": 21}
    fasta = str(tmp_path / "g.npz")
    np.savez(fasta, chrom_names=np.array(list(sizes)), chrom_lengths=np.array(list(sizes.values())),
             **{"seq_" + c: rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n) for c, n in sizes.items()})
    r = run_cli(["bias", "--fasta", fasta, "--out", str(tmp_path / "g")])
    assert r.returncode == 0, r.stderr[-2000:]
    warn = [x for x in r.stderr.splitlines() if "wrote no lines" in x]
    assert len(warn) == 1 and "chrA:3000-3005" in warn[0] and "chrS:0-20" in warn[0] and "chrT" not in warn[0]
    with gzip.open(str(tmp_path / "g.Scores.bedgraph.gz"), "rt") as f:
        a = per_base_sizes(f.read(), sizes)
    assert sorted(a) == ["chrA", "chrT"]
    assert np.array_equal(np.flatnonzero(a["chrA"]), np.arange(10, 2995)) and np.array_equal(np.flatnonzero(a["chrT"]), [10])
    assert os.path.exists(str(tmp_path / "g.Scores.bedgraph.gz.tbi"))
    bed = tmp_path / "r.bed"
    bed.write_text("chrA\t3005\t3100\nchrA\t100\t200\nchrS\t3\t9\n")
    r = run_cli(["bias", "--fasta", fasta, "--bed", str(bed), "--out", str(tmp_path / "b")])
    assert r.returncode == 0, r.stderr[-2000:]
    warn = [x for x in r.stderr.splitlines() if "wrote no lines" in x]
    assert len(warn) == 1 and "chrA:3005-3100" in warn[0] and "chrS:3-9" in warn[0] and "chrA:100-200" not in warn[0]
    with gzip.open(str(tmp_path / "b.Scores.bedgraph.gz"), "rt") as f:
        a = per_base_sizes(f.read(), sizes)
    assert sorted(a) == ["chrA"] and np.array_equal(np.flatnonzero(a["chrA"]), np.arange(100, 200))
    # nothing but empty intervals: an empty track and its index, exit 0
    bed.write_text("chrS\t3\t9\n")
    r = run_cli(["bias", "--fasta", fasta, "--bed", str(bed), "--out", str(tmp_path / "e")])
    assert r.returncode == 0, r.stderr[-2000:]
    with gzip.open(str(tmp_path / "e.Scores.bedgraph.gz"), "rt") as f:
        assert f.read() == ""


def per_base_sizes(text, sizes):
    out = {}
    for line in text.splitlines():
        c, s, e, _ = line.split("\t")
        out.setdefault(c, np.zeros(sizes[c], bool))[int(s):int(e)] = True
    return out


def test_kmer_pwm_exits_1_without_a_file(inputs, tmp_path):
    words = [a + b for a in "ACGT" for b in "ACGT"]
    p = tmp_path / "di.PWM.txt"
    p.write_text("#PWM Descriptor File\n#Contains PWM and pertinent information\n#up\n2\n#down\n2\n#nucleotides\n%s\n#mat\n%s" % (
        "\t".join(words), "".join("\t".join(["1.0"] * 5) + "\n" for _ in words)))
    r = run_cli(["bias", "--fasta", inputs[1], "--pwm", str(p), "--out", str(tmp_path / "o")])
    assert r.returncode == 1
    err = [x for x in r.stderr.splitlines() if x.strip()]
    assert len(err) == 1 and "k-mer" in err[0]
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")]


def test_bad_arguments_are_refused():
    from nucleoatac_amd import _lib as Lb
    from nucleoatac_amd import get_context
    from nucleoatac_amd.pyatac.make_bias_track import SeqTrackChunks
    lens = np.array([10, 30], np.int32)
    K = 5
    seq = np.frombuffer(b"ACGT" * 12, np.uint8)[:int(lens.sum()) + 2 * (K - 1)].copy()
    off = np.array([0, 14, 48], np.int64)
    pk = SeqTrackChunks(chunk_start=np.array([0, 100]), chunk_len=lens, frag_off=np.zeros(3, np.int64), frag_lpos=np.zeros(0, np.int32),
                        frag_ilen=np.zeros(0, np.int32), bias_off=None, bias_log=None, chroms=["c", "c"], track_seq_off=off, track_seq=seq)
    logp = np.log(np.full((4, K), 0.25))
    acgt = np.frombuffer(b"ACGT", np.uint8)
    b = get_context().upload(pk)

    def refused(*a):
        with pytest.raises(Lb.NatacError) as e:
            b.run_pwm_track(*a)
        assert e.value.code == -1                      # NATAC_E_ARG
        with pytest.raises(Lb.NatacError) as e:        # nothing was launched: the track still holds nothing
            b.track(Lb.T_BIAS)
        assert e.value.code == -3                      # NATAC_E_STATE
    try:
        refused(np.array([0, 15, 48], np.int64), seq, logp, acgt)               # windows of the wrong lengths
        refused(np.array([1, 15, 48], np.int64), seq, logp, acgt)               # seq_off[0] != 0
        refused(off, seq, np.log(np.full((4, K + 1), 0.25)), acgt)              # another K: every window is one base short
        refused(off, seq, np.zeros((4, 0)), acgt)                               # K < 1
        refused(off, seq, np.zeros((0, K)), acgt[:0])                           # nrow < 1
        for bad in (np.nan, np.inf, -np.inf):                                   # log(0) = -inf: a zero in the PWM
            t = logp.copy()
            t[2, 3] = bad
            refused(off, seq, t, acgt)
        refused(off, seq, logp, np.frombuffer(b"ACGA", np.uint8))               # two rows with one letter
        refused(np.array([0, 4106, 8232], np.int64), np.full(8232, 65, np.uint8), np.zeros((4, 4097)), acgt)   # more than 4096 cells
        with pytest.raises(ValueError):
            b.run_pwm_track(off, seq[:-1], logp, acgt)                          # seq shorter than seq_off says
        with pytest.raises(NotImplementedError):
            b.run_pwm_track(off, seq, logp, ["AA", "AC", "AG", "AT"])
        b.run_pwm_track(off, seq, logp, acgt)
        np.testing.assert_allclose(b.track(Lb.T_BIAS), np.full(40, K * np.log(0.25)), rtol=1e-14)
    finally:
        b.free()
