"""`pyatac peaks` on the host: the critical-value tables against scipy.stats.poisson.sf, the NumPy restatement of the rule
(tests/peaks_ref.py) on hand-computed chromosomes, the command line, the fixed-width selection and the files' text.  The device part is
tests/test_gpu_enriched_regions.py; here get_peaks runs with the restatement as its per-chromosome finder, so nothing needs a GPU."""
import os

import numpy as np
import pytest

import peaks_ref as R
from nucleoatac_amd.pyatac import get_peaks as G
from nucleoatac_amd.pyatac.cli import main, pyatac_parser


def _i64(x):
    return np.asarray(x, np.int64)


# ---- the critical-value tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,S,L,q", [(75, 500, 5000, 5), (20, 100, 1000, 3)])
def test_tables_are_the_poisson_critical_values(h, S, L, q):
    """for every k, thr[k] is the largest count T of the local window whose rate T (2h + 1) / width still leaves a pileup of k with a tail
    probability of at most P: sf(k - 1, rate(T)) <= P < sf(k - 1, rate(T + 1)).  poisson.sf does not go through gammaincinv.  With scipy
    1.15.3 the share of k that satisfies both is 1 for both geometries and both tables, so all of them are asserted."""
    from scipy.stats import poisson
    lam, ts, tl = G.critical_tables(h, S, L, q)
    assert ts.dtype == tl.dtype == np.int32 and len(lam) == len(ts) == len(tl) == 65536
    assert lam[0] == 0 and ts[0] == 0 and tl[0] == 0 and np.all(np.diff(lam) > 0)
    ref = R.tables(h, S, L, q)
    assert all(np.array_equal(a, b) for a, b in zip((lam, ts, tl), ref))
    k = np.arange(1, 65536)
    P = 10.0 ** -q
    for T, width in ((ts, 2 * S + 1), (tl, 2 * L + 1)):
        T = T[1:].astype(np.float64)
        at, above = poisson.sf(k - 1, T * (2 * h + 1) / width), poisson.sf(k - 1, (T + 1) * (2 * h + 1) / width)
        bad = np.flatnonzero(~((at <= P) & (P < above)))
        assert not len(bad), "k = %s" % (bad[:10] + 1)


def test_table_entries_are_clipped_to_int32():
    _, ts, tl = G.critical_tables(1, 1, 50000, 0.5)          # Lam[65535] * 100001 / 3 is far past 2^31
    assert tl.max() == 2 ** 31 - 1 and np.all(np.diff(tl.astype(np.int64)) >= 0) and ts.max() < 2 ** 31 - 1


def test_min_pileup():
    lam = R.critical_rates(5)
    assert G.min_pileup_for(lam, 0.0) == 1 == R.min_pileup(lam, 0.0)                  # Lam[0] = 0 >= 0, raised to 1
    k = G.min_pileup_for(lam, 3.7)
    assert lam[k] >= 3.7 > lam[k - 1] and k == R.min_pileup(lam, 3.7)
    assert G.min_pileup_for(lam, lam[40]) == 40
    with pytest.raises(G.PeaksError):
        G.min_pileup_for(lam, lam[-1] * 1.01)
    assert R.min_pileup(lam, lam[-1] * 1.01) is None


# ---- hand-computed chromosomes (h = 2, S = 5, L = 20) -------------------------------------------------------------------------------
# a table made by hand so that the verdicts can be worked out on paper: thr_small[k] = 2k, thr_large[k] = 4k, min_pileup 3
HAND_S, HAND_L = np.arange(16, dtype=np.int32) * 2, np.arange(16, dtype=np.int32) * 4
# insertions: 4 at base 100, 1 at 110 (the r of the first record), 3 at 200, 4 at 204; every other r lies past the chromosome
HAND_POS, HAND_TLEN = _i64([96, 96, 96, 96, 196, 196, 196, 200, 200, 200, 200]), _i64([19, 400, 400, 400, 400, 400, 400, 400, 400, 400, 400])


def _hand(max_gap, min_length, n=300):
    return R.enriched_regions(HAND_POS, HAND_TLEN, n, 2, 5, 20, max_gap, min_length, 3, HAND_S, HAND_L, counts=True)


def test_hand_computed_regions():
    """p = 4 on 98..102 (s = 4 <= 8, g = 5 <= 16: significant).  Around 200: p = 3 on 198..201, 7 at 202, 4 on 203..206; s = 3 at 198,
    7 on 199..205, 4 on 206..209; g = 7.  So 198 is significant (3 <= 6), 199..201 are not (7 > 6), 202 is (7 <= 14), 203..206 are (<= 8)."""
    out = _hand(0, 1)
    assert [a.tolist() for a in out[:6]] == [[98, 198, 202], [103, 199, 207], [100, 198, 202], [4, 3, 7], [4, 3, 7], [5, 7, 7]]
    assert out[6:] == (3, 11)
    assert [a.dtype for a in out[:6]] == [np.int64] * 3 + [np.int32] * 3


def test_hand_computed_gap_and_length_rules():
    out = _hand(3, 1)            # exactly three non-significant bases between 198 and 202: joined
    assert [a.tolist() for a in out[:6]] == [[98, 198], [103, 207], [100, 202], [4, 7], [4, 7], [5, 7]] and out[6:] == (2, 11)
    out = _hand(2, 1)            # one more than the gap allows
    assert out[0].tolist() == [98, 198, 202] and out[6] == 3
    out = _hand(0, 2)            # the one-base region is dropped, and still counted as found
    assert out[0].tolist() == [98, 202] and out[1].tolist() == [103, 207] and out[6:] == (3, 11)
    out = _hand(0, 5)
    assert out[0].tolist() == [98, 202] and _hand(0, 6)[0].tolist() == []


def test_hand_computed_chromosome_ends():
    """three insertions at base 0 (l of records at pos -4) and three at base 49 = n - 1 (r of records at pos -30, whose l = -26 is dropped
    on its own); windows are clipped: p = 3 on 0..2 and on 47..49"""
    pos, tlen = _i64([-30] * 3 + [-4] * 3), _i64([84] * 3 + [400] * 3)
    assert np.sort(R.insertions(pos, tlen, 50)).tolist() == [0, 0, 0, 49, 49, 49]
    out = R.enriched_regions(pos, tlen, 50, 2, 5, 20, 0, 1, 3, HAND_S, HAND_L, counts=True)
    assert [a.tolist() for a in out[:6]] == [[0, 47], [3, 50], [1, 48], [3, 3], [3, 3], [3, 3]] and out[6:] == (2, 6)


def test_hand_computed_plateau_summit_and_table_cap():
    """two separate maximal stretches in one region: 5 insertions at 100 and 5 at 111 -> p = 5 on 98..102 and on 109..113, nothing
    between, joined by max_gap 6: a = 98, b = 113, summit 105 (an odd a + b rounds down), where p = 0.  With a table of 4 entries k is 3."""
    pos, tlen = _i64([96] * 5 + [107] * 5), _i64([400] * 10)
    out = R.enriched_regions(pos, tlen, 300, 2, 5, 20, 6, 1, 3, HAND_S, HAND_L)
    assert [a.tolist() for a in out] == [[98], [114], [105], [0], [5], [10]]
    out = R.enriched_regions(pos, tlen, 300, 2, 5, 20, 6, 1, 3, HAND_S[:4], HAND_L[:4])     # k = 3: s = 5 <= 6, g = 10 <= 12
    assert out[0].tolist() == [98]
    out = R.enriched_regions(pos, tlen, 300, 2, 5, 20, 6, 1, 3, HAND_S[:3], HAND_L[:3])     # k = 2: s = 5 > 4
    assert out[0].tolist() == []


def test_the_issue_sketch():
    """3,000 uniform and 5 x 400 planted fragments on 60 kb: five regions, the outer two touch the chromosome's ends"""
    pos, tlen = R.hotspot_chromosome(1)
    lam, ts, tl = R.tables(75, 500, 5000, 5)
    n = 60000
    mp = R.min_pileup(lam, 151.0 * len(R.insertions(pos, tlen, n)) / n)
    out = R.enriched_regions(pos, tlen, n, 75, 500, 5000, 75, 150, mp, ts, tl)
    assert len(out[0]) == 5 and out[0][0] == 0 and out[1][-1] == n and np.all(out[0][1:] >= out[1][:-1])


# ---- the fixed-width set ----------------------------------------------------------------------------------------------------------------
def test_fixed_width_selection():
    lengths = [1000, 500]
    #        region:  0     1     2     3     4     5     6
    chrom = _i64([0, 0, 0, 0, 1, 1, 0])
    summit = _i64([100, 150, 400, 30, 470, 100, 975])
    m = np.array([5.0, 9.0, 9.0, 50.0, 50.0, np.inf, 7.0])
    p = _i64([10, 10, 12, 99, 99, 3, 9])
    # W = 100: starts 50, 100, 350, -20 (leaves the chromosome), 420 (ends at 520 > 500: dropped), 50, 925 (ends at 1025: dropped)
    fc, fs = G.fixed_width_set(chrom, summit, m, p, lengths, 100)
    # rank: 5 (inf), then 2 (9.0, p 12) before 1 (9.0, p 10), then 0 (5.0), which overlaps 1 ([50, 150) against [100, 200)) and goes
    assert list(zip(fc.tolist(), fs.tolist())) == [(0, 100), (0, 350), (1, 50)]
    # intervals that only touch are both kept; an odd width centres with W // 2 before the summit
    fc, fs = G.fixed_width_set(_i64([0, 0]), _i64([100, 151]), np.array([3.0, 4.0]), _i64([5, 5]), lengths, 51)
    assert fs.tolist() == [75, 126]
    # a full tie in mlog10p and p: chromosome index, then start
    fc, fs = G.fixed_width_set(_i64([1, 0, 0]), _i64([100, 140, 100]), np.array([2.0] * 3), _i64([4] * 3), lengths, 100)
    assert list(zip(fc.tolist(), fs.tolist())) == [(0, 50), (1, 50)]
    # exactly against both ends is inside
    fc, fs = G.fixed_width_set(_i64([0, 0]), _i64([50, 950]), np.array([1.0, 1.0]), _i64([1, 1]), lengths, 100)
    assert fs.tolist() == [0, 900]
    fc, fs = G.fixed_width_set(_i64([]), _i64([]), np.zeros(0), _i64([]), lengths, 100)
    assert len(fc) == 0 and len(fs) == 0


def test_score():
    from scipy.stats import poisson
    m, fold = G.score([30, 12, 100000], [33, 0, 10], [153, 0, 10], 2, 5, 20, 0.5)
    lam = [5 * max(0.5, 33 / 11.0, 153 / 41.0), 5 * 0.5, 2.5]
    assert np.allclose(fold[:2], [30 / lam[0], 12 / lam[1]], rtol=1e-15)
    assert np.allclose(m[:2], [-np.log10(poisson.sf(29, lam[0])), -np.log10(poisson.sf(11, lam[1]))], rtol=1e-12)
    assert np.isinf(m[2]) and m[2] > 0


# ---- the command --------------------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_required_arguments(capsys):
    a = pyatac_parser().parse_args(["peaks", "--bam", "x.npz"])
    assert (a.half_width, a.small, a.large, a.mlog10p, a.max_gap, a.min_length, a.fixed_width) == (75, 500, 5000, 5.0, 75, 150, None)
    assert a.fasta is None and a.sizes is None and a.out is None and a.call == "peaks"
    with pytest.raises(SystemExit):
        pyatac_parser().parse_args(["peaks"])
    assert "--bam" in capsys.readouterr().err


def _store(tmp_path, name="sample.frags.npz", empty=False):
    from nucleoatac_amd.pyatac.fragments import FragmentStore
    if empty:
        st = FragmentStore(["chr1"], [3000], {"chr1": _i64([])}, {"chr1": _i64([])})
    else:
        # chr1: 60 records with l = 1000 and r = 1041 .. 1100; chr2: five scattered records; chr3: none
        st = FragmentStore(["chr1", "chr2", "chr3"], [3000, 1000, 500],
                           {"chr1": _i64([996] * 60), "chr2": _i64([-6, 100, 300, 500, 990]), "chr3": _i64([])},
                           {"chr1": _i64(np.arange(50, 110)), "chr2": _i64([40, 50, 60, 70, 80]), "chr3": _i64([])})
    path = str(tmp_path / name)
    st.save_npz(path)
    return path


SMALL = ["--half_width", "2", "--small", "5", "--large", "20", "--mlog10p", "2", "--max_gap", "3", "--min_length", "1"]


def _args(argv):
    return pyatac_parser().parse_args(["peaks"] + argv)


def _ref_regions(*a):
    return R.enriched_regions(*a, counts=True)


@pytest.mark.parametrize("extra,message", [
    (["--half_width", "0"], "1 <= --half_width (0) <= --small (500) <= --large (5000) <= 50000 must hold"),
    (["--small", "74"], "1 <= --half_width (75) <= --small (74) <= --large (5000) <= 50000 must hold"),
    (["--large", "499"], "1 <= --half_width (75) <= --small (500) <= --large (499) <= 50000 must hold"),
    (["--large", "50001"], "1 <= --half_width (75) <= --small (500) <= --large (50001) <= 50000 must hold"),
    (["--mlog10p", "0"], "--mlog10p (0.0) must be positive"),
    (["--mlog10p", "-1"], "--mlog10p (-1.0) must be positive"),
    (["--max_gap", "-1"], "--max_gap (-1) must not be negative"),
    (["--min_length", "0"], "--min_length (0) must be at least 1"),
    (["--fixed_width", "0"], "--fixed_width (0) must be at least 1"),
    (["--sizes", "MISSING"], "MISSING: no such file"),
    (["--fasta", "MISSING"], "MISSING: no such file"),
])
def test_refusals_write_nothing(tmp_path, capsys, extra, message):
    bam = _store(tmp_path)
    missing = str(tmp_path / "missing.sizes")
    before = sorted(os.listdir(tmp_path))
    rc = main(["peaks", "--bam", bam, "--out", str(tmp_path / "o")] + [missing if x == "MISSING" else x for x in extra])
    assert rc == 1 and capsys.readouterr().err == "pyatac peaks: %s\n" % message.replace("MISSING", missing)
    assert sorted(os.listdir(tmp_path)) == before


def test_missing_input_and_empty_store_write_nothing(tmp_path, capsys):
    rc = main(["peaks", "--bam", str(tmp_path / "none.npz"), "--out", str(tmp_path / "o")])
    assert rc == 1 and "no such file" in capsys.readouterr().err and os.listdir(tmp_path) == []
    bam = _store(tmp_path, empty=True)
    rc = main(["peaks", "--bam", bam, "--out", str(tmp_path / "o")])
    assert rc == 1 and capsys.readouterr().err == "pyatac peaks: the store holds no records\n" and os.listdir(tmp_path) == [os.path.basename(bam)]


def test_a_chromosome_without_a_length_is_refused(tmp_path):
    bam = _store(tmp_path)
    sizes = tmp_path / "g.sizes"
    sizes.write_text("chr1\t3000\n")
    with pytest.raises(G.PeaksError, match="chr2 has records but no length"):
        G.get_peaks(_args(["--bam", bam, "--sizes", str(sizes), "--out", str(tmp_path / "o")] + SMALL), regions=_ref_regions)
    assert sorted(os.listdir(tmp_path)) == ["g.sizes", "sample.frags.npz"]


NARROWPEAK = "chr1\t998\t1003\tsample.frags_peak_1\t%d\t.\t%s\t%s\t-1\t2\n"


def test_files_exact_text_and_default_output_name(tmp_path, monkeypatch):
    """the small store: 60 insertions at chr1:1000 (p = 60 on 998..1002), their partners one per base on 1041..1100 (p = 5 there, below
    min_pileup or not improbable against s = 11), 125 insertions kept over 4,500 bases"""
    from scipy.stats import poisson
    bam = _store(tmp_path)
    monkeypatch.chdir(tmp_path)
    res, texts = G.get_peaks(_args(["--bam", bam, "--fixed_width", "20"] + SMALL), regions=_ref_regions)
    assert sorted(os.listdir(tmp_path)) == ["sample.frags.npz", "sample.frags.peaks.fixed.bed", "sample.frags.peaks.narrowPeak",
                                            "sample.frags.peaks.txt"]
    # chr2's record at pos -6 loses its l = -2, the one at 990 its r = 1065: 2 * 65 - 2 = 128 kept
    lam_g = 5 * 128 / 4500.0
    assert res["min_pileup"] == R.min_pileup(R.critical_rates(2), lam_g)
    assert [res[k].tolist() for k in ("chrom", "start", "end", "summit", "pileup", "n_small", "n_large")] == [[0], [998], [1003], [1000], [60], [60], [60]]
    lam = 5 * max(128 / 4500.0, 60 / 11.0, 60 / 41.0)
    m = -poisson.logsf(59, lam) / np.log(10)
    want = NARROWPEAK % (min(1000, int(10 * m)), "%.4f" % (60 / lam), "%.2f" % m)
    assert open("sample.frags.peaks.narrowPeak").read() == want == "chr1\t998\t1003\tsample.frags_peak_1\t73\t.\t2.2000\t7.37\t-1\t2\n"
    assert open("sample.frags.peaks.fixed.bed").read() == "chr1\t990\t1010\n"
    assert open("sample.frags.peaks.txt").read() == (
        "records\t65\ninsertions_kept\t128\ninsertions_dropped\t2\ngenome_length\t4500\nlam_g\t0.142222\nmin_pileup\t%d\n"
        "significant_bases\t5\nregions_found\t1\nregions_kept\t1\nfixed_width_kept\t1\n" % res["min_pileup"])
    assert texts[".peaks.narrowPeak"] == want.encode()


def test_sizes_file_sets_the_lengths_and_no_fixed_width_no_bed(tmp_path):
    bam = _store(tmp_path)
    sizes = tmp_path / "g.sizes"
    sizes.write_text("chr1\t1001\nchr2\t1000\nchr3\t500\nchrX\t7499\n")       # chr1 ends right behind the hotspot: its partners are dropped
    res, _ = G.get_peaks(_args(["--bam", bam, "--sizes", str(sizes), "--out", str(tmp_path / "o")] + SMALL), regions=_ref_regions)
    assert res["genome_length"] == 10000 and res["insertions_kept"] == 68 and res["end"].tolist() == [1001]
    assert sorted(os.listdir(tmp_path)) == ["g.sizes", "o.peaks.narrowPeak", "o.peaks.txt", "sample.frags.npz"]
    assert open(str(tmp_path / "o.peaks.txt")).read().endswith("fixed_width_kept\tNA\n")


def test_no_region_is_not_an_error(tmp_path):
    bam = _store(tmp_path)
    res, _ = G.get_peaks(_args(["--bam", bam, "--out", str(tmp_path / "o"), "--fixed_width", "200", "--mlog10p", "200"]), regions=_ref_regions)
    assert res["regions_kept"] == 0
    assert open(str(tmp_path / "o.peaks.narrowPeak")).read() == "" and open(str(tmp_path / "o.peaks.fixed.bed")).read() == ""
    text = open(str(tmp_path / "o.peaks.txt")).read()
    assert "regions_found\t0\nregions_kept\t0\nfixed_width_kept\t0\n" in text and "records\t65\n" in text


def test_an_infinite_score_is_written_finite():
    res = dict(chrom=_i64([0]), start=_i64([5]), end=_i64([9]), summit=_i64([7]), pileup=_i64([9]), n_small=_i64([1]), n_large=_i64([1]),
               mlog10p=np.array([np.inf]), fold=np.array([3.0]), records=1, insertions_kept=2, insertions_dropped=0, genome_length=10,
               lam_g=1.0, min_pileup=1, significant_bases=4, regions_found=1, regions_kept=1)
    assert G.texts(res, ["c"], "b")[".peaks.narrowPeak"] == b"c\t5\t9\tb_peak_1\t1000\t.\t3.0000\t1000.00\t-1\t2\n"


def test_downstream_bed_readers_take_both_files(tmp_path):
    """read_bed_columns is the reader of `counts`, `cellqc --peaks` and `cellcounts --bed`; ChunkList.read that of `nucleoatac run --bed`"""
    from nucleoatac_amd.pyatac.chunk import ChunkList, read_bed_columns
    bam = _store(tmp_path)
    G.get_peaks(_args(["--bam", bam, "--out", str(tmp_path / "o"), "--fixed_width", "20"] + SMALL), regions=_ref_regions)
    for name, row in (("o.peaks.narrowPeak", (998, 1003)), ("o.peaks.fixed.bed", (990, 1010))):
        names, chrom, start, end, _ = read_bed_columns(str(tmp_path / name))
        assert list(names) == ["chr1"] and chrom.tolist() == [0] and (start.tolist(), end.tolist()) == ([row[0]], [row[1]])
        chunks = ChunkList.read(str(tmp_path / name))
        assert [(c.chrom, c.start, c.end) for c in chunks] == [("chr1",) + row]


# ---- the constructed cases of the device tests reach what they are built for (the restatement alone) ---------------------------------
def _pairs(ans):
    return list(zip(ans[0].tolist(), ans[1].tolist()))


def test_scan_borders_of_the_default_segment():
    hist, verdict, segment = R.scan_borders()
    assert R.SEGMENT == 2 * R.SCAN_TRIP and R.BORDERS_N > 2 * R.SEGMENT           # three segments; the last has one trip
    assert segment == [4194304, 8388608] and verdict == [2097152, 6291456]
    assert hist == [2097152, 4194304, 6291455, 8388607]       # two more trips of the histogram's scan in each full segment


@pytest.mark.parametrize("max_gap,kind", R.BORDER_CASES)
def test_border_cases_lie_across_their_borders(max_gap, kind):
    case, spots, ans = R.border_case_with_answer(max_gap, kind)
    hist, verdict, segment = R.scan_borders()
    regions, ins = set(_pairs(ans)), R.insertions(case[0], case[1], case[2])
    assert len(regions) == ans[6] > R.FIRST_CAPACITY                             # the first sweep's buffer overflows
    assert [B for B, _, _ in spots] == sorted(verdict + segment)
    for B, what, want in spots:
        assert all(w in regions for w in want), (B, what)
        lo, hi = want[0][0], want[-1][1] - 1                  # the construction's first and last significant base
        assert not np.any((ins >= lo - 100) & (ins <= lo)) and not np.any((ins >= hi) & (ins <= hi + 100))       # nothing else near it
        if what in ("joined", "split"):
            x = want[-1][0] if what == "split" else want[0][0] + 31 + max_gap   # the later run's first base
            between = max_gap + (what == "split")
            assert not np.any((ins >= x - between - 1) & (ins <= x - 1)) and np.any(ins == x + 1) and np.any(ins == x - between - 2)
            assert len(want) == (2 if what == "split" else 1)
            assert x - max_gap - 1 < B <= x                   # the bases that decide whether x starts a region: both sides of B
        elif what == "dense":
            assert lo < B - 1 and B + 1 < hi and (lo + hi) // 2 > B + 2           # across B - 1 | B, the summit not beside it
        elif what == "ends":
            assert hi == B - 1 and B == segment[0]            # ends on the last base of a segment
        else:
            assert what == "starts" and lo == B and B == segment[1]
        assert all(lo < b < hi for b in hist if abs(b - B) <= 1) or what in ("ends", "starts")
    assert all(any(0 <= B - b <= 1 for B, _, _ in spots) for b in hist)
    if (max_gap, kind) in ((0, "joined"), (7, "dense")):      # a run across every border of the histogram's scan, between them
        dense = [(B, want[0]) for B, what, want in spots if what in ("joined", "dense")]
        if max_gap == 0:
            assert len(dense) == 4 and all(a < b - 1 and b + 1 < e for b in hist for B, (a, e) in dense if abs(b - B) <= 1)
        else:
            assert [B for B, _ in dense] == verdict


def test_long_piece_cases_have_the_pieces_they_are_made_for():
    cases, summits = R.long_piece_cases()
    for k, (case, (top_a, top_b)) in enumerate(zip(cases, summits)):
        ans = R.regions_of(case, counts=False)
        assert _pairs(ans) == [(999, 1002), (2500, 14300), (14699, 14702), (15099, 15102), (15500, 21500), (21999, 22002)]
        per_segment = R.pieces(ans[0], ans[1], case[2], 3000)
        assert per_segment == [[3, 500], [3000], [3000], [3000], [2300, 3], [3, 2500], [3000], [500, 3]]
        long_ = [[p for p in seg if p > R.SHORT_MAX] for seg in per_segment]
        assert [len(s) for s in long_] == [0, 1, 1, 1, 1, 1, 1, 0]             # the long list's offset grows from segment to segment
        assert sum(1 for seg, l in zip(per_segment, long_) if seg == l) == 4 and sum(1 for seg, l in zip(per_segment, long_) if l and seg != l) == 2
        assert max(max(seg, default=0) for seg in R.pieces(ans[0], ans[1], case[2], 2048)) <= R.SHORT_MAX
        assert ans[2][1] == top_a and ans[2][4] == top_b and ans[3].tolist() == [1, 2 if k == 2 else 5, 1, 1, 5, 1]
    assert summits == [(2700, 16000), (7000, 19000), (6350, 21200)]
    assert 2500 < 2700 < 3000 < 6000 < 7000 < 9000 < 10000 < 12000 and 15500 < 16000 < 18000 < 19000 < 21000 < 21200 < 21500


def test_piece_limit_case_has_regions_of_exactly_the_limit():
    case, want = R.piece_limit_case()
    ans = R.regions_of(case, counts=False)
    assert list(zip(*(a.tolist() for a in ans[:3]))) == want
    assert sorted(set((ans[1] - ans[0]).tolist())) == [R.SHORT_MAX - 1, R.SHORT_MAX, R.SHORT_MAX + 1] and len(want) == 15
    assert ans[3].tolist() == [12, 12, 12, 12, 3] * 3         # one highest base, or two equal ones around a summit that is none
    cum = np.concatenate([[0], np.cumsum(np.bincount(R.insertions(case[0], case[1], case[2]), minlength=case[2]))])
    p = R.window_counts(cum, case[2], 1)
    for (a, e, c), place in zip(want, ["first", "last", 63, 64, "both"] * 3):
        top = a + np.flatnonzero(p[a:e] == 12)
        assert top.tolist() == {"first": [a], "last": [e - 1], "both": [a, e - 1]}.get(place, [c]) and p[a:e].max() == 12
    assert case[2] < R.SEGMENT                                # one segment: a region is one piece


def test_reach_case_is_decided_by_its_far_records():
    case = R.reach_case()
    pos, tlen, n, geom = case[:4]
    L, seg = geom[2], R.REACH_SEGMENT
    assert pos[0] == -15 < pos[1] and tlen[0] == 5000 == tlen.max() and pos[0] + 4 < 0 and pos[0] + tlen[0] - 5 == 5 * seg - L
    assert pos[-1] == 6024 > pos[-2] and tlen[-1] == -3000 == tlen.min() and pos[-1] + 4 >= n and pos[-1] + tlen[-1] - 5 == 3 * seg + L - 1
    assert np.sum(tlen == 0) == 1 and np.sum((tlen >= 30) & (tlen <= 220)) > 0.8 * len(pos)
    ins = R.insertions(pos, tlen, n)
    assert np.sum(ins == 5 * seg - L) == 1 and np.sum(ins == 3 * seg + L - 1) == 1
    full = R.regions_of(case)
    at = {(a, e): (c, g) for a, e, c, g in zip(full[0].tolist(), full[1].tolist(), full[2].tolist(), full[5].tolist())}
    assert at[(2997, 2999)] == (2997, 5) and at[(5001, 5003)] == (5001, 5)
    assert at[(3037, 3042)] == (3039, 8) and at[(4958, 4963)] == (4960, 8)      # the far insertions at exactly large of the summits
    assert not any(a < 4003 and e > 3998 for a, e in at)
    for name, gone, there in (("far+", (5001, 5003), (4998, 5003)), ("far-", (2997, 2999), (2997, 3002)), ("zero", None, (3998, 4003))):
        less = R.regions_of(R.reach_case(drop=(name,)))
        assert there in _pairs(less) and gone not in _pairs(less) and there not in at
    less = R.regions_of(R.reach_case(drop=("far+", "far-")))
    assert less[5][_pairs(less).index((3037, 3042))] == 7 and less[5][_pairs(less).index((4958, 4963))] == 7


def test_grid_stride_case_keeps_a_region_of_the_records_past_the_grid():
    case = R.grid_stride_case()
    assert len(case[0]) == R.GRID_RECORDS + 1000 and np.all(np.diff(case[0]) >= 0) and case[1].max() <= 220
    ans = R.regions_of(case)
    tail = ans[0] >= 99_000
    assert tail.sum() == 1 and (~tail).sum() >= 6 and case[4] > 1000
    less = R.regions_of(R.grid_stride_case(tail=False))       # the same tables without the last 1000 records
    assert all(np.array_equal(a[~tail], b) for a, b in zip(ans[:6], less[:6]))


def test_far_end_case_moves_with_a_shift():
    case = R.far_end_case()
    ans = R.regions_of(case)
    assert len(ans[0]) >= 3 and ans[1][-1] == case[2] and (case[0] + 4).min() > case[3][2]
    d = 3_000_000
    moved = R.regions_of(R.shifted(case, d))
    want = R.shift_answer(ans, d)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(moved[:6], want[:6])) and moved[6:] == want[6:]
    assert R.shifted(case, 2 ** 31 - 1 - case[2])[2] == 2 ** 31 - 1


def test_wide_window_cases_keep_regions_the_large_window_decides():
    cases = R.wide_window_cases()
    assert all(c[3][2] == R.MAX_WINDOW and c[2] == 120_000 < R.SEGMENT for c in cases)      # every dense range is the whole chromosome
    assert [len(c[5]) for c in cases] == [64, 2, 2] and cases[2][3][0] == R.MAX_WINDOW
    answers = [R.regions_of(c) for c in cases]
    assert all(len(a[0]) >= 1 for a in answers)
    assert all(np.array_equal(a, b) for a, b in zip(answers[0], answers[1]))
    opened = R.regions_of(cases[0][:6] + (R.OPEN,))
    assert opened[7] > answers[0][7]                          # thr_large takes significant bases away
    assert (answers[2][1] - answers[2][0]).max() > R.SHORT_MAX
