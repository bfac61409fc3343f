"""`pyatac signal` without a device: the parser against the reference's (pyatac/cli.py:270-308), the default output name, the host part
of nucleoatac_amd/pyatac/signal_around_sites.py (centre, window, clip, pad, span merging) through the NumPy restatement of
tests/signal_ref.py against the reference's own matrices (tests/golden/pyatac_signal.npz, made by tests/golden/make_golden_signal.py),
the two text formats against the reference's files, and every SignalError with its exit code."""
import argparse
import gzip
import os

import numpy as np
import pytest

import signal_ref as R
from conftest import load_golden
from nucleoatac_amd.pyatac.cli import main, pyatac_parser

G = load_golden("pyatac_signal")
CASES = [str(x) for x in G["cases"]]
SIZES = {f[0]: int(f[1]) for f in (x.split("\t") for x in str(G["sizes_text"]).splitlines())}
RECORDS = [(f[0], int(f[1]), int(f[2]), float(f[3])) for f in (x.split("\t") for x in str(G["track_text"]).splitlines())]


def case_args(key):
    up, down, strand, e, p, sc, al, no_agg, norm, which = [int(x) for x in G["args_" + key]]
    return argparse.Namespace(up=up, down=down, strand=strand or None, exp=bool(e), positive=bool(p), scale=bool(sc), all=bool(al),
                              no_agg=bool(no_agg), norm=bool(norm), which=which, flags=e | 2 * p | 4 * sc)


def bed_text(which):
    return str(G["bed_int_text" if which else "bed_text"])


def golden_tracks(key):
    return gzip.decompress(G["tracks_" + key].tobytes()).decode("ascii")


def write_inputs(d, which=0):
    bed = str(d / "sites.bed")
    with open(bed, "w") as f:
        f.write(bed_text(which))
    sizes = str(d / "genome.sizes")
    with open(sizes, "w") as f:
        f.write(str(G["sizes_text"]))
    return bed, sizes


def host_rows(tmp_path, a):
    """the package's host part for a case: the BED columns, the windows, the merged spans and the value buffer the device would get
    (read here by the restatement's read_track)"""
    from nucleoatac_amd.pyatac.chunk import read_bed_columns
    from nucleoatac_amd.pyatac.signal_around_sites import merge_spans, site_windows
    bed, _ = write_inputs(tmp_path, a.which)
    names, chrom, start, end, minus = read_bed_columns(bed, strand_col=a.strand)
    ws, we, lead, K = site_windows(names, chrom, start, end, minus, SIZES, a.up, a.down)
    sc, ss, se, off, src = merge_spans(chrom, ws, we)
    vals = np.concatenate([R.read_track(RECORDS, names[c], int(s), int(e)) for c, s, e in zip(sc, ss, se)])
    assert len(vals) == off[-1]
    return names, chrom, start, end, minus, ws, we, lead, K, (sc, ss, se, off, src), vals


def bit_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64),
                                                                                              b[~np.isnan(b)].view(np.int64))


def test_parser_has_the_references_flags_and_defaults():
    p = pyatac_parser()
    a = p.parse_args(["signal", "--bed", "s.bed", "--bg", "t.bedgraph.gz", "--sizes", "g.sizes"])
    assert vars(a) == dict(call="signal", bed="s.bed", bg="t.bedgraph.gz", sizes="g.sizes", out=None, cores=1, all=False, no_agg=False,
                           up=250, down=250, weight=None, strand=None, exp=False, positive=False, scale=False, norm=False)
    a = p.parse_args(["signal", "--bed", "s.bed", "--bg", "t", "--sizes", "g", "--out", "o", "--cores", "4", "--all", "--no_agg", "--up", "30",
                      "--down", "70", "--weight", "5", "--strand", "6", "--exp", "--positive", "--scale", "--norm"])
    assert (a.out, a.cores, a.all, a.no_agg, a.up, a.down, a.weight, a.strand, a.exp, a.positive, a.scale, a.norm) == (
        "o", 4, True, True, 30, 70, 5, 6, True, True, True, True)
    for bad in (["signal", "--bg", "t", "--sizes", "g"], ["signal", "--bed", "s.bed", "--sizes", "g"], ["signal", "--bed", "s.bed", "--bg", "t"],
                ["signal", "--bam", "x.bam", "--bed", "s.bed"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for tool in ("vplot", "bias_vplot"):
        with pytest.raises(SystemExit):
            p.parse_args([tool, "--bed", "s.bed", "--bg", "t", "--sizes", "g"])


def test_default_output_name_is_set_before_anything_is_read():
    from nucleoatac_amd.pyatac.signal_around_sites import get_signal
    a = pyatac_parser().parse_args(["signal", "--bed", "/no/such/dir/nucpos.bed.gz", "--bg", "/no/such/t.gz", "--sizes", "/no/such/g.sizes"])
    with pytest.raises(IOError):
        get_signal(a)
    assert a.out == "nucpos.bed"


@pytest.mark.parametrize("key", [k for k in CASES if case_args(k).all])
def test_host_windows_and_the_restatement_give_the_references_matrix(key, tmp_path):
    """site_windows + merge_spans feed the restated gather / transform: the reference's matrix.  Bit for bit where no exp or division
    is involved; with them, within 4 ulp per entry (NumPy's exp here against NumPy's exp where the golden was made)"""
    a = case_args(key)
    names, chrom, start, end, minus, ws, we, lead, K, spans, vals = host_rows(tmp_path, a)
    want = G["mat_" + key]
    assert K == a.up + a.down + 1 and want.shape == (len(start), K)
    for i in range(len(start)):            # the package's windows are the restatement's
        c, s, e, ld = R.site_window(int(start[i]), int(end[i]), bool(minus[i]), a.up, a.down, SIZES[names[chrom[i]]])
        assert (ws[i], we[i], lead[i]) == (s, e, ld), (key, i)
    src = spans[4]
    got = R.rows_ref(vals, src, (we - ws).astype(np.int32), lead, minus, K, a.flags)
    fast = R.rows_ref_fast(vals, src, (we - ws).astype(np.int32), lead, minus, K, a.flags)
    sites = [(names[c], int(s), int(e), bool(m)) for c, s, e, m in zip(chrom, start, end, minus)]
    direct = R.signal_ref(RECORDS, SIZES, sites, a.up, a.down, a.flags)
    assert bit_equal(got, direct), key
    if a.exp or a.scale:
        assert np.array_equal(np.isnan(got), np.isnan(want)), key
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 4 * 2.0 ** -52 * np.abs(want[ok])), key
        assert np.allclose(fast, want, rtol=1e-13, atol=0, equal_nan=True), key
    else:
        assert bit_equal(got, want) and bit_equal(fast, want), key


def test_the_golden_holds_the_cases_the_rule_turns_on():
    rows = [x.split("\t") for x in bed_text(0).splitlines()]
    kept = [r for r in rows if int(r[2]) - int(r[1]) >= 1]
    assert len(kept) == len(rows) - 2 == len(G["mat_plain_strand"])
    name = [r[3] for r in kept]
    m = G["mat_plain_strand"]
    assert np.isnan(m[name.index("in_gap")]).all() and np.isnan(m[name.index("not_in_track")]).all()
    assert not m[name.index("all_padding")].any()
    both, both_minus = m[name.index("clip_both")], m[name.index("clip_both_minus")]
    assert not both[:11].any() and both[11:].all()                      # padded on the left in genomic orientation ...
    assert not both_minus[-11:].any() and both_minus[:-11].all()        # ... which the minus strand turns to the right
    assert np.isnan(m[name.index("starts_at_0_exactly")][:3]).all()     # a window that starts at 0 unclipped is read, not padded
    end = m[name.index("clip_end")]
    assert not end[-16:].any() and bit_equal(end[:35], R.read_track(RECORDS, "chrA", 2965, 3000))   # centre 2990: 16 columns past chrA
    even, even_minus = m[name.index("even")], m[name.index("even_minus")]
    odd, odd_minus = m[name.index("odd")], m[name.index("odd_minus")]
    assert bit_equal(odd[::-1], odd_minus)                              # odd length: one centre for both strands
    assert bit_equal(even, odd) and not bit_equal(even[::-1], even_minus)      # even length: centres 1050 (plus) and 1049 (minus)
    assert bit_equal(even[::-1][1:], even_minus[:-1])
    s = G["mat_scale_strand"]
    assert not s[name.index("in_gap")].any()                            # S == 0: NaN became 0, divided by 1
    e = G["mat_exp_strand"]
    assert np.all(e[name.index("all_padding")] == 1) and np.isnan(e[name.index("in_gap")]).all()
    assert np.all(G["mat_positive_strand"][~np.isnan(m)] >= 0) and (m[~np.isnan(m)] < 0).any()
    assert np.array_equal(G["mat_integers_plain_strand"], np.round(G["mat_integers_plain_strand"]))
    assert G["mat_one_column"].shape[1] == 1 and G["mat_up10_down30_strand"].shape[1] == 41


@pytest.mark.parametrize("key", [k for k in CASES if case_args(k).all])
def test_tracks_text_is_the_references(key):
    from nucleoatac_amd.pyatac import signal_around_sites as S
    mat = G["mat_" + key]
    assert S.tracks_text(mat).decode("ascii") == golden_tracks(key)
    old, S.TEXT_ROWS = S.TEXT_ROWS, 3       # a block boundary inside the matrix
    try:
        assert S.tracks_text(mat).decode("ascii") == golden_tracks(key)
    finally:
        S.TEXT_ROWS = old


@pytest.mark.parametrize("key", [k for k in CASES if not case_args(k).no_agg])
def test_agg_text_is_the_references_and_the_aggregate_is_the_column_sum(key, tmp_path):
    from nucleoatac_amd.pyatac.signal_around_sites import agg_text
    a = case_args(key)
    text = str(G["agg_" + key])
    want = np.array([float(x) for x in text.split()])
    assert agg_text(want) == text                                       # '%.18e' round-trips: the text is the aggregate
    if a.all:
        mat = G["mat_" + key]
    else:
        names, chrom, start, end, minus, ws, we, lead, K, spans, vals = host_rows(tmp_path, a)
        mat = R.rows_ref(vals, spans[4], (we - ws).astype(np.int32), lead, minus, K, a.flags)
    agg = R.aggregate(mat) / (len(mat) if a.norm else 1)
    n, K = mat.shape
    mag = np.nansum(np.abs(mat), axis=0) / (n if a.norm else 1)
    assert np.all(np.abs(agg - want) <= (2 * n + K + 4) * 2.0 ** -52 * mag), key
    if a.which:
        assert np.array_equal(agg, want) and np.array_equal(R.aggregate_in_segments(mat, 3), want), key


def test_merge_spans_gives_disjoint_sorted_spans_that_hold_every_window():
    from nucleoatac_amd.pyatac.signal_around_sites import merge_spans
    rng = np.random.default_rng(11)
    chrom = rng.integers(0, 3, 200).astype(np.int32)
    ws = rng.integers(0, 5000, 200).astype(np.int64)
    we = ws + rng.integers(0, 120, 200)
    we[:5] = ws[:5]                                                     # empty windows
    sc, ss, se, off, src = merge_spans(chrom, ws, we)
    assert np.all(se >= ss) and off[0] == 0 and np.array_equal(np.diff(off), se - ss)
    for k in range(1, len(sc)):
        assert (sc[k], ss[k]) > (sc[k - 1], se[k - 1])                  # sorted, disjoint and not touching
    genome = {c: np.arange(6000) + 10000 * c for c in range(3)}
    vals = np.concatenate([genome[c][s:e] for c, s, e in zip(sc, ss, se)])
    for i in range(200):
        assert np.array_equal(vals[src[i]:src[i] + we[i] - ws[i]], genome[chrom[i]][ws[i]:we[i]]), i
    covered = sum(len(np.unique(np.concatenate([np.arange(a, b) for a, b in zip(ws[chrom == c], we[chrom == c])]))) for c in range(3))
    assert off[-1] == covered                                           # nothing is read twice
    one = merge_spans(np.zeros(1, np.int32), np.array([7]), np.array([9]))
    assert one[1].tolist() == [7] and one[2].tolist() == [9] and one[4].tolist() == [0]


def test_native_reader_gives_the_restated_track_values(tmp_path):
    """the host read of get_signal (bgzip, tabix index, natac_tbx_read_regions with NaN for uncovered bases) against read_track: gaps,
    the later of two overlapping records, reads past the last record and a chromosome that is not in the index"""
    import __graft_entry__ as g
    g.build()
    from nucleoatac_amd.tabix import NativeTabix
    from nucleoatac_amd.writer import bgzip_file, tabix_index
    plain = str(tmp_path / "track.bedgraph")
    with open(plain, "w") as f:
        f.write(str(G["track_text"]))
    bg = bgzip_file(plain)
    assert tabix_index(bg) == len(RECORDS)
    spans = [("chrA", 0, 51), ("chrA", 580, 930), ("chrA", 1190, 1310), ("chrA", 1490, 2110), ("chrA", 2965, 3000), ("chrA", 3000, 3000),
             ("chrA", 3050, 3051), ("chrB", 0, 40), ("chrN", 275, 326), ("chrA", 0, 3000)]
    tbx = NativeTabix(bg)
    vals, off = tbx.read_regions([s[0] for s in spans], [s[1] for s in spans], [s[2] for s in spans], empty=np.nan, value_col=4)
    tbx.close()
    for k, (c, s, e) in enumerate(spans):
        assert bit_equal(vals[off[k]:off[k + 1]], R.read_track(RECORDS, c, s, e)), spans[k]
    a = R.read_track(RECORDS, "chrA", 1190, 1310)
    assert np.all(a[10:50] == 1.5) and np.all(a[50:110] == -0.75) and np.isnan(R.read_track(RECORDS, "chrN", 275, 326)).all()


def run_main(argv, capsys):
    rc = main(argv)
    err = [x for x in capsys.readouterr().err.splitlines() if x.strip()]
    return rc, err


def test_every_signal_error_exits_with_1_and_writes_nothing(tmp_path, capsys):
    from nucleoatac_amd.pyatac.signal_around_sites import SignalError, site_windows
    bed, sizes = write_inputs(tmp_path)
    out = str(tmp_path / "o")
    bg = str(tmp_path / "never_opened.bedgraph.gz")

    def refused(argv, *words):
        rc, err = run_main(["signal", "--bg", bg, "--sizes", sizes, "--out", out, "--all"] + argv, capsys)
        assert rc == 1 and len(err) == 1 and err[0].startswith("pyatac signal: ") and all(w in err[0] for w in words), (argv, err)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")], argv

    for up, down in ((0, 5), (5, 0), (250, 0)):                         # exactly one flank 0: the reference's one-base broadcast
        refused(["--bed", bed, "--up", str(up), "--down", str(down)], "--up %d" % up, "--down %d" % down)
    refused(["--bed", bed, "--up", "-1", "--down", "3"], "negative")
    negative = tmp_path / "negative.bed"
    negative.write_text("chrA\t10\t20\n" + str(G["bed_negative_text"]))
    refused(["--bed", str(negative), "--up", "25", "--down", "25"], "row 2", "chrA:3100-3121", "3085")
    missing = tmp_path / "missing.bed"
    missing.write_text("chrA\t10\t20\nchrA\t7\t7\n" + str(G["bed_missing_text"]))
    refused(["--bed", str(missing), "--up", "25", "--down", "25"], "row 2", "chrQ", "--sizes")      # the dropped row is not counted
    empty = tmp_path / "empty.bed"
    empty.write_text("chrA\t7\t7\n")
    refused(["--bed", str(empty)], "no site")
    short = tmp_path / "short.bed"
    short.write_text("chrA\t10\t20\tn\t0\t+\nchrA\t30\t40\tn\n")
    refused(["--bed", str(short), "--strand", "6"], "line 2")
    # a window that ends exactly where it starts is not an error (the reference reads nothing and pads), one base further is
    names, chrom = ["chrA"], np.zeros(2, np.int32)
    ws, we, lead, K = site_windows(names, chrom, np.array([3015, 10]), np.array([3036, 20]), np.zeros(2, bool), SIZES, 25, 25)
    assert (ws[0], we[0], lead[0], K) == (3000, 3000, 0, 51)
    with pytest.raises(SignalError):
        site_windows(names, chrom, np.array([3016, 10]), np.array([3037, 20]), np.zeros(2, bool), SIZES, 25, 25)
    # one column: the centre itself, --sizes not consulted (the reference extends nothing)
    ws, we, lead, K = site_windows(["chrQ"], np.zeros(2, np.int32), np.array([10, 10]), np.array([20, 20]), np.array([False, True]), {}, 0, 0)
    assert (ws.tolist(), we.tolist(), lead.tolist(), K) == ([15, 14], [16, 15], [0, 0], 1)
