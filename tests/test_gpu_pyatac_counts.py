"""`pyatac counts` on the GPU (natac_region_counts; nucleoatac_amd/pyatac/get_counts.py) against the reference's own outputs
(tests/golden/pyatac_sites.npz, made by tests/golden/make_golden_sites.py): the decompressed text of every case equals the
reference's exactly -- integer counts, no tolerance.  The kernels against the NumPy restatement of tests/sites_ref.py on seeded
inputs that cross every arm of the launch geometry: regions with 0, 1, 63, 64, 65, 2047, 2048, 2049 (the slice bound RC_SLICE) and
several hundred thousand candidate records, one region and 100,000 regions, any split of the regions into calls.  A real BAM gives
what the .npz store gives; the error exits and NATAC_E_ARG."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import sites_ref as R
from conftest import ROOT, load_golden
from helpers import write_bam

pytestmark = pytest.mark.gpu

G = load_golden("pyatac_sites")
CASES = [str(x) for x in G["count_cases"]]
NAMES = [str(x) for x in G["chrom_names"]]
RC_SLICE = 2048


def golden_text(key):
    return gzip.decompress(G["text_" + key].tobytes()).decode("ascii")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("counts_inputs")
    bed = str(d / "sites.bed")
    with open(bed, "w") as f:
        f.write(str(G["bed_text"]))
    frags = str(d / "frags.npz")
    np.savez(frags, chrom_names=G["chrom_names"], chrom_lengths=G["chrom_lengths"], **{"pos_" + c: G["pos_" + c] for c in NAMES},
             **{"tlen_" + c: G["tlen_" + c] for c in NAMES})
    bam = str(d / "frags.bam")
    recs = [(i, int(p), 0x63, int(t)) for i, c in enumerate(NAMES) for p, t in zip(G["pos_" + c], G["tlen_" + c])]
    decoys = [(0, 1000, 0x53, 150), (0, 1001, 0x61, 150), (1, 700, 0x93, -120)]       # reverse strand / not a proper pair: never kept
    write_bam(bam, [(c, int(n)) for c, n in zip(NAMES, G["chrom_lengths"])], sorted(recs + decoys, key=lambda r: (r[0], r[1])))
    return d, bed, frags, bam


def case_argv(key, bam, bed, out):
    atac, lower, upper = [int(x) for x in G["args_" + key]]
    return ["counts", "--bam", bam, "--bed", bed, "--out", out, "--lower", str(lower), "--upper", str(upper)] + ([] if atac else ["--not_atac"])


def run_cli(argv, timeout=300):
    return subprocess.run([sys.executable, "-m", "nucleoatac_amd.pyatac.cli"] + argv, cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout)


def read_text(path):
    with gzip.open(path, "rt") as f:
        return f.read()


@pytest.mark.parametrize("key", CASES)
def test_text_equals_the_references(inputs, key):
    d, bed, frags, _ = inputs
    r = run_cli(case_argv(key, frags, bed, str(d / key)))
    assert r.returncode == 0, (key, r.stdout[-2000:], r.stderr[-2000:])
    assert read_text(str(d / key) + ".counts.txt.gz") == golden_text(key), key


@pytest.mark.parametrize("key", ["counts_atac_0_500", "counts_notatac_100_300"])
def test_a_real_bam_gives_what_the_store_gives(inputs, key):
    d, bed, _, bam = inputs
    r = run_cli(case_argv(key, bam, bed, str(d / ("bam_" + key))))
    assert r.returncode == 0, (key, r.stdout[-2000:], r.stderr[-2000:])
    assert read_text(str(d / ("bam_" + key)) + ".counts.txt.gz") == golden_text(key), key


def test_default_output_name_and_empty_bed(inputs, tmp_path):
    _, _, frags, _ = inputs
    bed = tmp_path / "my.windows.bed"
    bed.write_text("chrA\t0\t4000\nchrA\t9\t9\n")
    r = subprocess.run([sys.executable, "-m", "nucleoatac_amd.pyatac.cli", "counts", "--bam", frags, "--bed", str(bed)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    assert read_text(str(tmp_path / "my.windows.counts.txt.gz")) == golden_text("counts_atac_0_500").splitlines()[
        [x.split("\t")[3] for x in str(G["bed_text"]).splitlines() if int(x.split("\t")[2]) > int(x.split("\t")[1])].index("whole")] + "\n"


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _store(rng, n, span):
    pos = np.sort(rng.integers(0, span, size=n)).astype(np.int64)
    tlen = np.where(rng.random(n) < 0.8, rng.integers(20, 400, size=n), rng.integers(0, 900, size=n)).astype(np.int64)
    tlen[rng.random(n) < 0.02] = 8
    return pos, tlen


GRID = 1000          # spacing of the sparse tail of the geometry store


def _geometry_store(rng, n):
    """n records at distinct positions about 4 bases apart, then 3000 records on a grid of GRID bases: regions in the dense part have
    hundreds to hundreds of thousands of candidate records, regions on the grid as few as none"""
    dense = np.sort(rng.choice(4 * n, size=n, replace=False))
    grid = 4 * n + 10 * GRID + GRID * np.arange(3000)
    pos = np.concatenate((dense, grid)).astype(np.int64)
    return pos, _store(rng, len(pos), 10)[1]


def _candidates(pos, starts, ends, lower, upper, shift):
    """the records the device has to look at for each region: s - max(upper, 1) < l < e + max(0, 1 - lower)"""
    l = pos + shift
    return np.searchsorted(l, np.asarray(ends) + max(0, 1 - lower), "left") - np.searchsorted(l, np.asarray(starts) - max(upper, 1), "right")


@pytest.mark.parametrize("atac, lower, upper", [(1, 0, 500), (0, 0, 500), (1, 100, 300), (1, -20, 40), (0, 1, 2)])
def test_kernels_match_numpy_across_the_launch_geometry(atac, lower, upper):
    rng = np.random.default_rng(77 + 13 * upper + atac)
    n = 700000
    pos, tlen = _geometry_store(rng, n)
    shift = 4 if atac else 0
    below, above = max(upper, 1), max(0, 1 - lower)
    l = pos + shift
    starts, ends = [], []
    for k in (1, 2, 63, 64, 65, 66):                      # on the grid: records a .. a + k - 1 and nothing else within reach
        for a in rng.integers(n + 5, n + 2900, size=3):
            starts.append(int(l[a]) - 10), ends.append(int(l[a + k - 1]) + 10)
    for a in rng.integers(n + 5, n + 2900, size=3):       # an empty region between two grid points: no candidate
        starts.append(int(l[a]) + 600), ends.append(int(l[a]) + 600)
    for k in (RC_SLICE - 1, RC_SLICE, RC_SLICE + 1, RC_SLICE + 2, 3 * RC_SLICE + 5, 250000, 600000):     # in the dense part
        for a in rng.integers(1, n - k - 1, size=3):
            starts.append(int(l[a]) + below - 1), ends.append(int(l[a + k - 1]) + 1 - above)
    for w in (0, 1, 37, 500, 3000, 9000, 40000):          # plain windows: about 100 .. 10,000 records each
        s = rng.integers(-2000, 4 * n + 2000, size=40)
        starts += s.tolist()
        ends += (s + w).tolist()
    starts, ends = np.array(starts, np.int64), np.array(ends, np.int64)
    want = R.region_counts_ref(pos, tlen, starts, ends, lower, upper, atac)
    cand = set(_candidates(pos, starts, ends, lower, upper, shift).tolist())
    assert {0, 1, 63, 64, 65, RC_SLICE - 1, RC_SLICE, RC_SLICE + 1, 250000, 600000} <= cand, sorted(cand)[:20]
    sample = rng.choice(len(starts), size=25, replace=False)
    assert np.array_equal(want[sample], R.region_counts_brute(pos, tlen, starts[sample], ends[sample], lower, upper, atac))
    got = _ctx().region_counts(pos, tlen, starts, ends, lower, upper, atac)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert want.max() > (100000 if upper >= 300 else 0)
    # however the regions are split into calls, and in any order
    perm = rng.permutation(len(starts))
    assert np.array_equal(_ctx().region_counts(pos, tlen, starts[perm], ends[perm], lower, upper, atac), want[perm])
    for i in (0, len(starts) // 2, len(starts) - 1):
        assert _ctx().region_counts(pos, tlen, starts[i:i + 1], ends[i:i + 1], lower, upper, atac).tolist() == [want[i]]
    parts = np.array_split(np.arange(len(starts)), 7)
    assert np.array_equal(np.concatenate([_ctx().region_counts(pos, tlen, starts[p], ends[p], lower, upper, atac) for p in parts]), want)


def test_one_hundred_thousand_regions_and_duplicate_positions():
    rng = np.random.default_rng(5)
    pos, tlen = _store(rng, 400000, 3000000)           # duplicates among the positions
    s = rng.integers(-500, 3000500, size=100000)
    e = s + rng.choice([0, 1, 200, 500, 501, 20000], size=len(s))
    want = R.region_counts_ref(pos, tlen, s, e, 0, 500, 1)
    got, ms = _ctx().region_counts(pos, tlen, s, e, 0, 500, True, with_kernel_ms=True)
    assert np.array_equal(got, want) and ms > 0 and want.max() > RC_SLICE
    # a store of one record, of none, and regions without records
    assert _ctx().region_counts(pos[:1], tlen[:1], s[:50], e[:50]).tolist() == R.region_counts_brute(pos[:1], tlen[:1], s[:50], e[:50], 0, 500, 1).tolist()
    assert _ctx().region_counts(pos[:0], tlen[:0], s[:50], e[:50]).tolist() == [0] * 50
    assert _ctx().region_counts(pos, tlen, s[:0], e[:0]).shape == (0,)


def test_insert_size_zero_on_the_device():
    pos, tlen = np.array([2500], np.int64), np.array([8], np.int64)
    s, e = np.array([2494, 2504, 2494, 2505]), np.array([2504, 2510, 2503, 2510])
    assert _ctx().region_counts(pos, tlen, s, e, 0, 500, True).tolist() == [1, 1, 0, 0]
    assert _ctx().region_counts(pos, tlen, s, e, 1, 500, True).tolist() == [0, 0, 0, 0]
    assert _ctx().region_counts(pos, tlen, s, e, -3, 1, True).tolist() == [1, 1, 0, 0]


def test_error_exits(inputs, tmp_path):
    _, bed, frags, _ = inputs
    out = str(tmp_path / "o")

    def refused(argv, word):
        r = run_cli(argv + ["--out", out])
        err = [x for x in r.stderr.splitlines() if x.strip()]
        assert r.returncode == 1 and len(err) == 1 and word in err[0], (argv, r.stderr[-2000:])
        assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")]
    refused(["counts", "--bam", frags, "--bed", bed, "--lower", "300", "--upper", "300"], "--upper")
    other = tmp_path / "other.bed"
    other.write_text("chrA\t10\t20\nchrQ\t5\t50\n")
    refused(["counts", "--bam", frags, "--bed", str(other)], "chrQ")


def test_bad_arguments_are_refused():
    import ctypes as C
    from nucleoatac_amd import _lib as Lb
    lib, h = Lb.load(), _ctx()._h
    pos, tlen = np.array([10, 20, 30], np.int64), np.array([100, 100, 100], np.int64)
    s, e = np.array([0, 50], np.int64), np.array([40, 90], np.int64)
    out = np.full(2, -7, np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(h_=h, nf=3, p=pos, t=tlen, nr=2, s_=s, e_=e, lower=0, upper=500, o=out):
        return lib.natac_region_counts(h_, nf, None if p is None else vp(p), None if t is None else vp(t), nr, None if s_ is None else vp(s_),
                                       None if e_ is None else vp(e_), lower, upper, 1, None if o is None else vp(o), None)
    assert call() == 0 and out.tolist() == [3, 0]
    for kw in (dict(h_=None), dict(p=None), dict(t=None), dict(s_=None), dict(e_=None), dict(o=None), dict(nf=-1), dict(nr=-1),
               dict(upper=0), dict(lower=500), dict(e_=np.array([40, 49], np.int64)), dict(p=np.array([10, 30, 20], np.int64))):
        assert call(**kw) == -1, kw                     # NATAC_E_ARG
        assert lib.natac_last_error(), kw
    with pytest.raises(Lb.NatacError) as err:
        _ctx().region_counts(pos, tlen, [5], [4])
    assert err.value.code == -1 and "end" in str(err.value)
    with pytest.raises(ValueError):
        _ctx().region_counts(pos, tlen[:2], s, e)
