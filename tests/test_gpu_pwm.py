"""`pyatac pwm` on the GPU (natac_insertion_seq_counts, natac_base_counts; nucleoatac_amd/pyatac/get_pwm.py) against the reference's
own outputs (tests/golden/pwm_fit.npz, made by tests/golden/make_golden_pwm.py): for every case of the golden grid the window counts,
the insertion count and the background counts are the reference's exactly, the fitted matrix is bit-identical and the written
.PWM.txt is the reference's text with its floats as Python 2 printed them.  Also: counts independent of the tiling, the sub-batching
and the order of the fragments; empty input; refused arguments; n == 0; a fitted PWM used by `nucleoatac occ --pwm`."""
import argparse
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

G = load_golden("pwm_fit")
CASES = [str(x) for x in G["cases"]]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pwm_inputs")
    names = [str(x) for x in G["chrom_names"]]
    fa = str(d / "genome.npz")
    np.savez(fa, chrom_names=G["chrom_names"], chrom_lengths=G["chrom_lengths"], **{"seq_" + c: G["seq_" + c] for c in names})
    empty = np.zeros(0, np.int64)
    arrs = {}
    for c in names:
        arrs["pos_" + c] = G["pos_" + c] if "pos_" + c in G else empty
        arrs["tlen_" + c] = G["tlen_" + c] if "tlen_" + c in G else empty
    bam = str(d / "reads.npz")
    np.savez(bam, chrom_names=G["chrom_names"], chrom_lengths=G["chrom_lengths"], **arrs)
    beds = {}
    for key in ("bed", "bed_f0", "bed_sizes"):
        beds[key] = str(d / (key + ".bed"))
        with open(beds[key], "w") as f:
            f.write(str(G[key + "_text"]))
    return dict(dir=d, fa=fa, bam=bam, beds=beds, chrs=dict(zip(names, [int(x) for x in G["chrom_lengths"]])))


def _params(key):
    p = dict((x[0], x[1:]) for x in key.split("_"))
    return dict(sym=p["s"] == "1", bed=p["b"] == "1", flank=int(p["f"]), lower=int(p["l"]), upper=int(p["u"]), atac=p["a"] == "1")


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _py2_text(ref_text):
    """the reference's .PWM.txt (written by the scratch copy's Python 3 str(float) = repr) with every value as Python 2 wrote it"""
    from nucleoatac_amd.pyatac.tracks import _py2_float_str
    head, mat = ref_text.split("#mat\n")
    rows = [r for r in mat.split("\n") if r]
    return head + "#mat\n" + "".join("\t".join(_py2_float_str(float(x)) for x in r.split("\t")) + "\n" for r in rows)


@pytest.mark.parametrize("key", CASES)
def test_golden_case(inputs, key, tmp_path):
    from nucleoatac_amd.pyatac import get_pwm as GP
    from nucleoatac_amd.pyatac.seq import ACGT, FastaStore, getNucFreqs, getNucFreqsFromChunkList
    p = _params(key)
    bed = inputs["beds"]["bed_f0" if p["flank"] == 0 else "bed"] if p["bed"] else None
    chunks = GP.genome_regions(inputs["chrs"], p["flank"]) if bed is None else GP.bed_regions(bed, inputs["chrs"], p["flank"])
    M, n = GP.count_windows(chunks, inputs["bam"], inputs["fa"], p["flank"], p["lower"], p["upper"], p["atac"], p["sym"])
    assert np.array_equal(M, G["M_" + key])
    assert n == int(G["n_" + key])
    # background counts, numerator and denominator
    fs = FastaStore.open(inputs["fa"])
    if bed is None:
        bg = sum(_ctx().base_counts(fs.seqs[c]) for c in fs.references)
        bg_n = sum(len(fs.seqs[c]) for c in fs.references)
        freqs = getNucFreqs(inputs["fa"], ACGT)
    else:
        bg = sum(_ctx().base_counts(fs.seqs[c.chrom], [c.start], [c.end]) for c in chunks)
        bg_n = sum(c.end - c.start for c in chunks)
        freqs = getNucFreqsFromChunkList(chunks, inputs["fa"], ACGT)
    assert np.array_equal(bg, G["bg_counts_" + key]) and bg_n == int(G["bg_n_" + key])
    assert np.array_equal(freqs, G["freqs_" + key])
    # the whole command: bit-identical matrix, the reference's text
    out = str(tmp_path / key)
    args = argparse.Namespace(bam=inputs["bam"], fasta=inputs["fa"], bed=bed, flank=p["flank"], lower=p["lower"], upper=p["upper"],
                              atac=p["atac"], sym=p["sym"], dinucleotide=False, cores=1, out=out)
    result = GP.get_pwm(args)
    ref = G["pwm_" + key]
    assert result.shape == ref.shape and np.array_equal(result.view(np.uint64), ref.view(np.uint64))
    with open(out + ".PWM.txt") as f:
        assert f.read() == _py2_text(str(G["pwm_text_" + key]))


@pytest.mark.parametrize("flank", [10, 100])
def test_genome_wide_counts_do_not_depend_on_the_tiling(inputs, flank):
    from nucleoatac_amd.pyatac import get_pwm as GP
    from nucleoatac_amd.pyatac.chunk import ChunkList
    key = "s1_b0_f%d_l0_u2000_a1" % flank
    chrs = inputs["chrs"]
    kb = ChunkList.convertChromSizes(chrs, splitsize=1000, offset=flank)        # the reference's 1-kb chunks
    tiles = GP.genome_regions(chrs, flank)                                       # large tiles
    small = GP.genome_regions(chrs, flank, tile=777)
    for chunks, sub_bp in ((kb, GP.SUB_BATCH_BP), (tiles, GP.SUB_BATCH_BP), (small, 3000), (kb, 1)):
        M, n = GP.count_windows(chunks, inputs["bam"], inputs["fa"], flank, 0, 2000, True, True, sub_bp=sub_bp)
        assert np.array_equal(M, G["M_" + key]) and n == int(G["n_" + key])


def test_fragment_order_does_not_change_the_counts(inputs):
    from nucleoatac_amd.pyatac import get_pwm as GP
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    from nucleoatac_amd.pyatac.seq import FastaStore
    st, fs = FragmentStore.open(inputs["bam"]), FastaStore.open(inputs["fa"])
    chunks = GP.genome_regions(inputs["chrs"], 10, tile=5000)
    cl, fo, lpos, ilen, so, seq = GP.pack_windows(chunks, st, fs, 10, 0, 2000, True)
    rng = np.random.default_rng(7)
    for sym in (True, False):
        M0, n0 = _ctx().insertion_seq_counts(cl, fo, lpos, ilen, so, seq, 10, 0, 2000, sym=sym)
        perm = np.concatenate([fo[k] + rng.permutation(fo[k + 1] - fo[k]) for k in range(len(cl))])
        M1, n1 = _ctx().insertion_seq_counts(cl, fo, lpos[perm], ilen[perm], so, seq, 10, 0, 2000, sym=sym)
        assert n0 > 0 and n0 == n1 and np.array_equal(M0, M1)


def _restated_counts(cl, fo, lpos, ilen, so, seq, flank, lower, upper, sym):
    """numpy restatement of the window counts (pyatac/tracks.py:179-201 over fragments)"""
    K = 2 * flank + 1
    row = np.full(256, 4, np.int64)
    for i, b in enumerate(b"ACGT"):
        row[b] = row[b + 32] = i
    M = np.zeros((5, K), np.int64)
    n = 0
    for k in range(len(cl)):
        w = row[seq[so[k]:so[k + 1]]]
        for f in range(fo[k], fo[k + 1]):
            l, m = int(lpos[f]), int(ilen[f])
            if not lower <= m < upper:
                continue
            r = l + m - 1
            if 0 <= l < cl[k]:
                n += 1
                np.add.at(M, (w[l:l + K], np.arange(K)), 1)
            if 0 <= r < cl[k]:
                n += 1
                if sym:
                    np.add.at(M, (w[r:r + K], np.arange(K)), 1)
                else:
                    b = w[r:r + K][::-1]
                    np.add.at(M, (np.where(b < 4, 3 - b, 4), np.arange(K)), 1)
    return M[:4], n


@pytest.mark.parametrize("flank", [0, 31, 32, 63, 64, 1000])
def test_column_tiles_against_a_restatement(flank):
    """K = 2*flank + 1 below, at and across the 64-column tiles of the kernel, up to the largest flank"""
    rng = np.random.default_rng(flank)
    nc = 5
    cl = rng.integers(0, 400, nc).astype(np.int32)
    cl[2] = 0
    nfk = rng.integers(0, 60, nc)
    nfk[3] = 0
    fo = np.concatenate(([0], np.cumsum(nfk))).astype(np.int64)
    lpos = rng.integers(-300, 500, fo[-1]).astype(np.int32)
    ilen = rng.integers(-5, 400, fo[-1]).astype(np.int32)
    so = np.concatenate(([0], np.cumsum(cl.astype(np.int64) + 2 * flank))).astype(np.int64)
    seq = rng.choice(np.frombuffer(b"ACGTNacgtn", np.uint8), so[-1])
    for sym in (True, False):
        M, n = _ctx().insertion_seq_counts(cl, fo, lpos, ilen, so, seq, flank, -3, 350, sym=sym)
        Mr, nr = _restated_counts(cl, fo, lpos, ilen, so, seq, flank, -3, 350, sym)
        assert n == nr and np.array_equal(M, Mr)
        assert n > 0


def test_empty_inputs_give_zeros():
    M, n = _ctx().insertion_seq_counts([], [0], [], [], [0], [], 10)
    assert n == 0 and M.shape == (4, 21) and not M.any()
    cl = np.array([100, 50], np.int32)
    so = np.array([0, 120, 190], np.int64)
    M, n = _ctx().insertion_seq_counts(cl, [0, 0, 0], [], [], so, np.full(190, ord("A"), np.uint8), 10)
    assert n == 0 and not M.any()
    assert not _ctx().base_counts(np.zeros(0, np.uint8)).any()
    assert np.array_equal(_ctx().base_counts(np.frombuffer(b"ACGTNacgtx", np.uint8), [0, 0, 5], [10, 4, 5]), [3, 3, 3, 3])


def test_bad_arguments_are_refused():
    from nucleoatac_amd import _lib as L
    cl = np.array([10], np.int32)
    fo = np.array([0, 1], np.int64)
    lp, il = np.array([2], np.int32), np.array([5], np.int32)

    def call(flank, lower=0, upper=2000, so=None):
        so = np.array([0, 10 + 2 * max(flank, 0)], np.int64) if so is None else np.asarray(so, np.int64)
        return _ctx().insertion_seq_counts(cl, fo, lp, il, so, np.full(int(so[-1]), 65, np.uint8), flank, lower, upper)

    assert call(1000)[1] == 2
    for kw in (dict(flank=-1), dict(flank=1001), dict(flank=10, lower=5, upper=5), dict(flank=10, lower=6, upper=5),
               dict(flank=10, so=[0, 29]), dict(flank=10, so=[0, 31])):
        with pytest.raises(L.NatacError) as e:
            call(**kw)
        assert e.value.code == -1
    lib = L.load()
    import ctypes as C
    with pytest.raises(L.NatacError) as e:     # frag_off that does not start at 0
        _ctx().insertion_seq_counts(cl, np.array([1, 1], np.int64), lp, il, [0, 30], np.zeros(30, np.uint8), 10)
    assert e.value.code == -1
    out = np.zeros(4, np.int64)
    s = np.zeros(10, np.uint8)
    st, en = np.array([5], np.int64), np.array([11], np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.natac_base_counts(_ctx()._h, vp(s), 10, 1, vp(st), vp(en), vp(out)) == -1


def test_no_insertion_exits_nonzero_and_writes_nothing(inputs, tmp_path):
    out = str(tmp_path / "none")
    r = subprocess.run([sys.executable, "-m", "nucleoatac_amd.pyatac.cli", "pwm", "--bam", inputs["bam"], "--fasta", inputs["fa"],
                        "--lower", "5000", "--upper", "6000", "--out", out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "nothing to fit" in r.stderr
    assert not os.path.exists(out + ".PWM.txt")


def test_track_api_against_the_reference_loop(inputs):
    """InsertionTrack.getInsertionSequences / getStrandedInsertionSequences with up != down and a permuted row order, against the
    reference's per-base loop restated in numpy"""
    from nucleoatac_amd.pyatac.seq import FastaStore, complement, seq_to_mat
    from nucleoatac_amd.pyatac.tracks import InsertionTrack
    nucs = ["C", "G", "A", "T"]
    up, down = 7, 12
    t = InsertionTrack("chrA", 3000, 6000)
    t.calculateStrandedInsertions(inputs["bam"], lower=0, upper=2000)
    off = max(up, down)
    s = FastaStore.open(inputs["fa"]).fetch("chrA", t.start - off, t.end + off)
    sm, mm = seq_to_mat(s, nucs), seq_to_mat(complement(s), nucs)
    ref_u = np.zeros((4, up + down + 1))
    ref_s = np.zeros((4, up + down + 1))
    for i in range(t.length()):
        ref_u += t.vals[i] * sm[:, off + i - up:off + i + down + 1]
        ref_s += t.plus[i] * sm[:, off + i - up:off + i + down + 1]
        ref_s += t.minus[i] * np.fliplr(mm[:, off + i - down:off + i + up + 1])
    assert t.vals.sum() > 0
    assert np.array_equal(t.getInsertionSequences(inputs["fa"], nucs, up=up, down=down), ref_u)
    assert np.array_equal(t.getStrandedInsertionSequences(inputs["fa"], nucs, up=up, down=down), ref_s)


def test_fitted_pwm_drives_occ_like_the_api_object(tmp_path):
    """`nucleoatac occ --pwm <fitted .PWM.txt>` gives the same tracks as run_occ handed the PWM object read from that file"""
    from helpers import GOLDEN as HG, read_bed3, synth_saccer3
    from nucleoatac_amd.nucleoatac.cli import main, nucleoatac_parser
    from nucleoatac_amd.nucleoatac.run_occ import run_occ
    from nucleoatac_amd.pyatac.bias import PWM
    from nucleoatac_amd.pyatac.cli import main as pyatac_main
    bed = os.path.join(HG, "ref_example.bed")
    bam, fa = synth_saccer3(str(tmp_path), read_bed3(bed), seed=3)
    base = str(tmp_path / "fit")
    assert pyatac_main(["pwm", "--bam", bam, "--fasta", fa, "--bed", bed, "--out", base]) == 0
    pwm = PWM.open(base + ".PWM.txt")
    assert pwm.mat.shape == (4, 21) and np.all(np.isfinite(pwm.mat)) and pwm.nucleotides == ["A", "C", "G", "T"]
    main(["occ", "--bed", bed, "--bam", bam, "--fasta", fa, "--pwm", base + ".PWM.txt", "--out", str(tmp_path / "cli")])
    args = nucleoatac_parser().parse_args(["occ", "--bed", bed, "--bam", bam, "--fasta", fa, "--out", str(tmp_path / "api")])
    args.pwm = pwm
    run_occ(args)
    for suffix in ("occ.bedgraph.gz", "occ.lower_bound.bedgraph.gz", "occ.upper_bound.bedgraph.gz", "occpeaks.bed.gz"):
        a = gzip.open(str(tmp_path / "cli") + "." + suffix, "rb").read()
        b = gzip.open(str(tmp_path / "api") + "." + suffix, "rb").read()
        assert a == b and len(a) > 0, suffix
