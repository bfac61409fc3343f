"""`pyatac signal` on the GPU (natac_site_signal; nucleoatac_amd/pyatac/signal_around_sites.py) against the reference's own outputs
(tests/golden/pyatac_signal.npz, made by tests/golden/make_golden_signal.py by running the reference's get_signal) and against the
NumPy restatement of tests/signal_ref.py.

Bounds, derived and not measured (u = 2^-52): a matrix entry goes through at most one exp (4 ulp allowed), one division (1 ulp) and a
divisor that is a K-term sum of non-negative terms in another order (K ulp), so it is within (K + 4) u of the reference's, relatively;
where there is no exp and no division it is the reference's bit for bit, NaN positions included.  A column of the aggregate is an
n-term sum in another order than the reference's, of entries that each carry that error: within (2n + K + 4) u times the column's sum
of absolute values.  Sums of integers are exact in any order: bit for bit."""
import ctypes as C
import gzip
import itertools

import numpy as np
import pytest

import signal_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

G = load_golden("pyatac_signal")
CASES = [str(x) for x in G["cases"]]
U = 2.0 ** -52
SG_TILE = 256                   # columns per block of natac_site_signal_rows (csrc/natac_sites.hpp)


def seg_len():
    import os
    import re
    from nucleoatac_amd import _lib
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = int(re.search(r"#define NATAC_SIGNAL_SEG (\d+)", open(os.path.join(here, "include", "natac.h")).read()).group(1))
    assert hdr == _lib.SIGNAL_SEG
    return hdr


SEG = seg_len()


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def bit_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64),
                                                                                              b[~np.isnan(b)].view(np.int64))


def case_flags(key):
    return [int(x) for x in G["args_" + key]]


def golden_tracks(key):
    return gzip.decompress(G["tracks_" + key].tobytes()).decode("ascii")


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """the golden's track bgzipped and indexed by the package's own writers, its sizes file and its two BEDs"""
    from nucleoatac_amd.writer import bgzip_file, tabix_index
    d = tmp_path_factory.mktemp("signal_inputs")
    plain = str(d / "track.bedgraph")
    with open(plain, "w") as f:
        f.write(str(G["track_text"]))
    bg = bgzip_file(plain)
    assert tabix_index(bg) == len(str(G["track_text"]).splitlines())
    sizes = str(d / "genome.sizes")
    with open(sizes, "w") as f:
        f.write(str(G["sizes_text"]))
    beds = []
    for k, key in enumerate(("bed_text", "bed_int_text")):
        beds.append(str(d / ("sites%d.bed" % k)))
        with open(beds[-1], "w") as f:
            f.write(str(G[key]))
    return d, bg, sizes, beds


def case_argv(key, bg, sizes, beds, out):
    up, down, strand, e, p, sc, al, no_agg, norm, which = case_flags(key)
    return (["signal", "--bed", beds[which], "--bg", bg, "--sizes", sizes, "--out", out, "--up", str(up), "--down", str(down)] +
            (["--strand", str(strand)] if strand else []) + (["--exp"] if e else []) + (["--positive"] if p else []) +
            (["--scale"] if sc else []) + (["--all"] if al else []) + (["--no_agg"] if no_agg else []) + (["--norm"] if norm else []))


def check_matrix(got, want, exact, K, what):
    if exact:
        assert bit_equal(got, want), what
        return
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bound = (K + 4) * U * np.abs(want[ok])
    print("%s: matrix error / bound, largest %.3g" % (what, np.max(err / np.where(bound > 0, bound, 1), initial=0)))
    assert np.all(err <= bound), what


def check_aggregate(got, want, mat_ref, n, K, exact, what, div=1):
    if exact:
        assert bit_equal(got, want), what
        return
    mag = np.nansum(np.abs(mat_ref), axis=0) / div
    bound = (2 * n + K + 4) * U * mag
    err = np.abs(got - want)
    print("%s: aggregate error / bound, largest %.3g" % (what, np.max(err / np.where(bound > 0, bound, 1), initial=0)))
    assert np.all(err <= bound), what


@pytest.mark.parametrize("key", CASES)
def test_golden_end_to_end(inputs, tmp_path, key):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    from nucleoatac_amd.pyatac.signal_around_sites import get_signal
    _, bg, sizes, beds = inputs
    up, down, strand, e, p, sc, al, no_agg, norm, which = case_flags(key)
    K = up + down + 1
    out = str(tmp_path / key)
    result, mat = get_signal(pyatac_parser().parse_args(case_argv(key, bg, sizes, beds, out)))
    exact = not (e or sc)
    assert result.shape == (K,) and result.dtype == np.float64
    if al:
        want = G["mat_" + key]
        assert mat.dtype == np.float64 and mat.shape == want.shape
        check_matrix(mat, want, exact, K, key)
        with gzip.open(out + ".tracks.txt.gz", "rb") as f:
            text = f.read().decode("ascii")
        if exact:
            assert text == golden_tracks(key), key
        else:
            assert len(text.splitlines()) == len(want) and all(len(x.split(",")) == K for x in text.splitlines()), key
    else:
        assert mat is None and not (tmp_path / (key + ".tracks.txt.gz")).exists()
    if no_agg:
        assert not (tmp_path / (key + ".agg.track.txt")).exists()
        return
    with open(out + ".agg.track.txt") as f:
        text = f.read()
    assert text == "".join("%.18e\n" % v for v in result), key             # np.savetxt's format; the file is the returned aggregate
    want = np.array([float(x) for x in str(G["agg_" + key]).split()])
    if al:
        ref_mat = G["mat_" + key]
    else:                       # no matrix from the reference without --all: the restatement's, for the magnitudes of the bound
        from nucleoatac_amd.pyatac.chunk import read_bed_columns
        records = [(f[0], int(f[1]), int(f[2]), float(f[3])) for f in (x.split("\t") for x in str(G["track_text"]).splitlines())]
        size = {f[0]: int(f[1]) for f in (x.split("\t") for x in str(G["sizes_text"]).splitlines())}
        names, chrom, start, end, minus = read_bed_columns(beds[which], strand_col=strand or None)
        sites = [(names[c], int(s), int(z), bool(m)) for c, s, z, m in zip(chrom, start, end, minus)]
        ref_mat = R.signal_ref(records, size, sites, up, down, e | 2 * p | 4 * sc)
    n = len(ref_mat)
    check_aggregate(result, want, ref_mat, n, K, bool(which), key, div=n if norm else 1)


def test_cli_writes_both_files(inputs, tmp_path, capsys):
    from nucleoatac_amd.pyatac.cli import main
    _, bg, sizes, beds = inputs
    out = str(tmp_path / "cli")
    assert main(case_argv("plain_strand", bg, sizes, beds, out)) == 0
    assert "plots are not produced" in capsys.readouterr().out
    with gzip.open(out + ".tracks.txt.gz", "rb") as f:
        assert f.read().decode("ascii") == golden_tracks("plain_strand")
    with open(out + ".agg.track.txt") as f:
        assert len(f.read().splitlines()) == 51


def test_batches_give_the_same_matrix(inputs, tmp_path, monkeypatch):
    """the batch budget lowered to 7 sites per device call: 3 batches of the 20 sites.  The rows do not depend on the batch; the aggregate is added
    in another order and stays within the bound"""
    from nucleoatac_amd.pyatac import signal_around_sites as S
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    _, bg, sizes, beds = inputs
    for key in ("plain_strand", "exp_positive_scale_strand"):
        K = 51
        argv = case_argv(key, bg, sizes, beds, str(tmp_path / "one"))
        agg1, mat1 = S.get_signal(pyatac_parser().parse_args(argv))
        calls = []
        real = type(_ctx()).site_signal
        monkeypatch.setattr(type(_ctx()), "site_signal", lambda self, *a, **k: (calls.append(len(a[1])), real(self, *a, **k))[1])
        monkeypatch.setattr(S, "BATCH_VALUES", 7 * K)
        agg2, mat2 = S.get_signal(pyatac_parser().parse_args(argv[:8] + [str(tmp_path / "many")] + argv[9:]))
        monkeypatch.undo()
        assert len(calls) >= 3 and max(calls) == 7 and sum(calls) == len(mat1), calls
        assert bit_equal(mat1, mat2), key
        check_aggregate(agg2, agg1, mat1, len(mat1), K, False, key + " in batches")
        with gzip.open(str(tmp_path / "one.tracks.txt.gz"), "rb") as f, gzip.open(str(tmp_path / "many.tracks.txt.gz"), "rb") as g:
            assert f.read() == g.read()


def synthetic(rng, n, K, n_vals=5000):
    """values with NaN stretches, negatives, zeros and -0.0; windows of every padding kind"""
    vals = np.round(rng.normal(0.3, 1.5, n_vals), 3)
    vals[rng.random(n_vals) < 0.1] = 0.0
    vals[rng.random(n_vals) < 0.02] = -0.0
    for a in rng.integers(0, n_vals, 12):
        vals[a:a + int(rng.integers(1, 2 * K + 2))] = np.nan
    vals[:K] = np.nan                                   # an all-NaN row can start at 0
    vals[K:2 * K] = 0.0                                 # and a row of zeros at K
    length = rng.integers(0, K + 1, n).astype(np.int32)
    length[rng.random(n) < 0.5] = K
    lead = (rng.random(n) * (K - length + 1)).astype(np.int32)
    lead[rng.random(n) < 0.3] = 0                       # lead + len < K: padding on the right
    src = (rng.random(n) * (n_vals - length + 1)).astype(np.int64)
    for i, (s, ln, ld) in enumerate(((0, K, 0), (K, K, 0), (7, 0, K // 2), (0, 0, K), (n_vals, 0, 0), (n_vals - K, K, 0))):
        if i < n:                                       # all NaN; all zero; all padding (len 0) twice; src == n_vals; the last values
            src[i], length[i], lead[i] = s, ln, ld
    return vals, src, length, lead


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 501, SG_TILE + 1, 3 * SG_TILE + 5])
def test_kernel_arms_against_the_restatement(K):
    ctx = _ctx()
    rng = np.random.default_rng(1000 + K)
    for n in (0, 1, SEG - 1, SEG, SEG + 1, 3 * SEG + 7):
        vals, src, length, lead = synthetic(rng, n, K)
        mixed = (rng.random(n) < 0.5).astype(np.uint8)
        plus_mats = {}
        for minus, flags in itertools.product((None, np.ones(n, np.uint8), mixed), range(8)):
            what = "K %d n %d flags %d minus %s" % (K, n, flags, "none" if minus is None else int(minus.sum()))
            kw = dict(exp=bool(flags & 1), positive=bool(flags & 2), scale=bool(flags & 4))
            agg, mat = ctx.site_signal(vals, src, length, lead, minus, K, want_matrix=True, **kw)
            agg_only, none = ctx.site_signal(vals, src, length, lead, minus, K, want_matrix=False, **kw)
            assert none is None and bit_equal(agg_only, agg), what              # mat == NULL changes nothing
            assert mat.shape == (n, K) and agg.shape == (K,)
            if n == 0:
                assert not agg.any() and not np.signbit(agg).any(), what
                continue
            want = R.rows_ref_fast(vals, src, length, lead, minus, K, flags)
            exact = not flags & 5
            if exact:
                assert bit_equal(mat, want), what
            else:
                assert np.array_equal(np.isnan(mat), np.isnan(want)), what
                ok = ~np.isnan(want)
                assert np.all(np.abs(mat[ok] - want[ok]) <= (K + 4) * U * np.abs(want[ok])), what
            if flags & 4:
                total = np.abs(mat).sum(axis=1)
                assert not np.isnan(mat).any() and np.all((total == 0) | (np.abs(total - 1) < 1e-12)), what
                if not flags & 1:
                    assert not mat[0].any() and (n < 2 or not mat[1].any()), what       # all NaN, all zero: S == 0, divided by 1
            else:
                assert np.isnan(mat[0]).all(), what
            assert bit_equal(agg, R.aggregate_in_segments(mat, SEG)), what      # the documented order, bit for bit
            mag = np.nansum(np.abs(want), axis=0)
            assert np.all(np.abs(agg - R.aggregate(want)) <= (2 * n + K + 4) * U * mag), what
            # mirror columns land exactly: a minus row is the plus row reversed (the divisor of --scale is added in another order)
            if minus is None:
                plus_mats[flags] = mat
            elif not flags & 4:
                rev = minus.astype(bool)
                assert bit_equal(mat[rev], plus_mats[flags][rev][:, ::-1]) and bit_equal(mat[~rev], plus_mats[flags][~rev]), what


def test_two_calls_give_the_same_bits():
    ctx = _ctx()
    rng = np.random.default_rng(77)
    n, K = 3 * SEG + 7, 501
    vals, src, length, lead = synthetic(rng, n, K, n_vals=40000)
    minus = (rng.random(n) < 0.5).astype(np.uint8)
    for flags in (0, 7):
        kw = dict(exp=bool(flags & 1), positive=bool(flags & 2), scale=bool(flags & 4), want_matrix=True)
        a1, m1 = ctx.site_signal(vals, src, length, lead, minus, K, **kw)
        ctx.site_signal(vals[:100], src[:3] % 50, length[:3] % 50, lead[:3] * 0, None, 50)     # another shape in between
        a2, m2 = ctx.site_signal(vals, src, length, lead, minus, K, **kw)
        assert bit_equal(a1, a2) and bit_equal(m1, m2)
        assert bit_equal(a1, R.aggregate_in_segments(m1, SEG))


def test_bad_operands_are_refused_before_any_launch():
    from nucleoatac_amd import _lib as Lb
    lib, h = Lb.load(), _ctx()._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    K = 5
    vals = np.arange(20, dtype=np.float64)
    src = np.array([0, 3, 15], np.int64)
    length = np.array([5, 2, 5], np.int32)
    lead = np.array([0, 3, 0], np.int32)
    mat = np.full((3, K), -7.0)
    agg = np.full(K, -7.0)
    ms = C.c_double(-1)

    def call(h_=h, v=vals, nv=20, ns=3, s=src, ln=length, ld=lead, k=K, flags=0, m=mat, a=agg):
        return lib.natac_site_signal(h_, None if v is None else vp(v), nv, ns, None if s is None else vp(s), None if ln is None else vp(ln),
                                     None if ld is None else vp(ld), None, k, flags, None if m is None else vp(m),
                                     None if a is None else vp(a), C.byref(ms))
    assert call() == 0 and ms.value >= 0
    assert mat.tolist() == [[0, 1, 2, 3, 4], [0, 0, 0, 3, 4], [15, 16, 17, 18, 19]] and agg.tolist() == [15, 17, 19, 24, 27]
    i32, i64 = (lambda *x: np.array(x, np.int32)), (lambda *x: np.array(x, np.int64))
    for kw, word in ((dict(s=i64(0, 3, 16)), "site 2"),                      # src + len > n_vals
                     (dict(nv=19), "site 2"),
                     (dict(ld=i32(0, 4, 0)), "site 1"),                      # lead + len > K
                     (dict(ln=i32(5, -1, 5)), "site 1"),                     # negative len
                     (dict(ld=i32(-1, 3, 0)), "site 0"),
                     (dict(s=i64(0, -1, 15)), "site 1"),
                     (dict(k=0), "K"), (dict(k=(1 << 20) + 2), "K"), (dict(flags=8), "flags"),
                     (dict(h_=None), ""), (dict(a=None), ""), (dict(v=None), ""), (dict(s=None), ""), (dict(ns=-1), ""), (dict(nv=-1), "")):
        mat[:], agg[:] = -7.0, -7.0
        ms.value = -1
        assert call(**kw) == -1, kw                                           # NATAC_E_ARG
        assert word in lib.natac_last_error().decode(), (kw, lib.natac_last_error())
        assert np.all(mat == -7.0) and np.all(agg == -7.0) and ms.value <= 0, kw      # nothing ran, nothing was written
    assert call() == 0 and agg.tolist() == [15, 17, 19, 24, 27]              # the context is as usable as before
    with pytest.raises(Lb.NatacError) as err:
        _ctx().site_signal(vals, [18], [5], [0], None, K)
    assert err.value.code == -1 and "site 0" in str(err.value)
    with pytest.raises(ValueError):
        _ctx().site_signal(vals, src, length[:2], lead, None, K)
