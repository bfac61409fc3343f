"""`pyatac motifs` end to end on the GPU (nucleoatac_amd/pyatac/get_motifs.py): a synthetic FASTA of three chromosomes with a strong
12-column motif planted at 40 known positions and strands, the sites file, both matrix formats, the summary, --only, --bg regions, and
`pyatac nucleotide` reading the sites file.  The matrix and the sites are compared with the NumPy restatement of tests/motifs_ref.py."""
import gzip
import os

import numpy as np
import pytest

import motifs_ref as R

pytestmark = pytest.mark.gpu

WORD = "CCGATTAGCTGA"
NAMES = ["chrA", "chrB", "chrC"]
N = 30000


def revcomp(word):
    return word[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def run(argv):
    from nucleoatac_amd.pyatac.cli import main
    return main(argv)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("motifs_cli")
    rng = np.random.default_rng(77)
    seqs, plants = {}, []
    for k, c in enumerate(NAMES):
        s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, N)].tobytes())
        pos = (1500 + 2000 * np.arange(13) + rng.integers(0, 300, 13)).tolist()
        if k == 0:
            pos.append(4995)                                  # across the border of the windows [4500, 5000) and [5000, 5500)
        for i, x in enumerate(pos):
            minus = bool(rng.integers(0, 2))
            w = revcomp(WORD) if minus else WORD
            if i % 4 == 1:
                w = w.lower()
            if i % 4 == 2:
                w = w[:5] + w[5:].lower()
            s[x:x + 12] = w.encode()
            if i == 3:
                s[x - 1:x] = b"N"                             # an N next to the site, not inside it
            plants.append((c, x, "-" if minus else "+"))
        s[100:110] = b"NNNNNNNNNN"
        seqs[c] = bytes(s)
    assert len(plants) == 40
    fasta = str(d / "genome.fa")
    with open(fasta, "w") as f:
        for c in NAMES:
            f.write(">%s\n" % c)
            for i in range(0, N, 60):
                f.write(seqs[c][i:i + 60].decode() + "\n")
    # abutting windows of 500 over [1000, 29000) of every chromosome, in a shuffled order, some overlapping ones and a zero-length row
    rows = [(c, a, a + 500) for c in NAMES for a in range(1000, 29000, 500)]
    rows += [("chrB", 1400, 2600), ("chrB", 1400, 2600), ("chrC", 0, 700), ("chrA", 29500, 30000), ("chrA", 7, 7)]
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    bed = str(d / "windows.bed")
    with open(bed, "w") as f:
        f.write("".join("%s\t%d\t%d\n" % r for r in rows))
    rows = [r for r in rows if r[2] > r[1]]
    second = R.random_counts(np.random.default_rng(5), 9, nsites=40)
    motifs = {"PLANT": ("planted factor", np.array([[50.0 if b == ch else 0.0 for b in "ACGT"] for ch in WORD])), "RND.2": ("", second)}
    mfile = str(d / "motifs.jaspar")
    with open(mfile, "w") as f:
        f.write(R.jaspar_text(motifs))
    return dict(dir=d, fasta=fasta, bed=bed, motifs=mfile, seqs=seqs, plants=plants, rows=rows, counts=motifs)


def expected(world, bg, p, ids):
    """the restatement's sites (rows of the file) and dense matrix"""
    S_list = [R.scores(world["counts"][i][1], bg) for i in ids]
    thr = [R.threshold(S, bg, p) for S in S_list]
    widths = np.array([len(S) for S in S_list], np.int32)
    S = np.concatenate(S_list)
    T = np.array([t[0] for t in thr], np.int32)
    rows = world["rows"]
    dense = np.zeros((len(rows), len(ids)), np.int32)
    per = {}
    for c in NAMES:
        idx = [i for i, r in enumerate(rows) if r[0] == c]
        hm, hs, hst, hsc, cnt = R.scan(world["seqs"][c], [rows[i][1] for i in idx], [rows[i][2] for i in idx], widths, S, T)
        dense[idx] = cnt
        per[c] = (hm, hs, hst, hsc)
    sites = []
    for m, mid in enumerate(ids):
        for c in NAMES:
            hm, hs, hst, hsc = per[c]
            for j in np.flatnonzero(hm == m):
                sites.append("%s\t%d\t%d\t%s\t%.2f\t%s" % (c, hs[j], hs[j] + widths[m], mid, hsc[j] / 100.0, "+-"[hst[j]]))
    return sites, dense, thr


def read_sites(path):
    with gzip.open(path, "rt") as f:
        return f.read().splitlines()


def read_summary(path):
    lines = open(path).read().splitlines()
    head = {l.split("\t")[0]: l.split("\t")[1:] for l in lines[:3]}
    k = lines.index("id\talt\twidth\tmax_score\tthreshold\ttail_p\thits_plus\thits_minus\twindows_hit")
    motifs = [l.split("\t") for l in lines[k + 1:-4]]
    totals = {l.split("\t")[0]: int(l.split("\t")[1]) for l in lines[-4:]}
    return head, motifs, totals


@pytest.fixture(scope="module")
def mtx_run(world):
    base = str(world["dir"] / "mtx")
    assert run(["motifs", "--fasta", world["fasta"], "--motifs", world["motifs"], "--bed", world["bed"], "--pvalue", "1e-5", "--out", base]) == 0
    return base


def test_planted_sites_are_found(world, mtx_run):
    rows = read_sites(mtx_run + ".motifs.sites.bed.gz")
    want, _, thr = expected(world, [0.25] * 4, 1e-5, ["PLANT", "RND.2"])
    assert rows == want                                       # order: motif, chromosome (FASTA order), start, + before -
    assert thr[0][0] < 12 * 198 and thr[0][1] is not None
    found = {tuple(r.split("\t")[i] for i in (0, 1, 5)) for r in rows if r.split("\t")[3] == "PLANT"}
    for c, x, strand in world["plants"]:
        assert (c, str(x), strand) in found, (c, x, strand)
    top = [r for r in rows if r.split("\t")[3] == "PLANT" and r.split("\t")[4] == "%.2f" % (12 * 1.98)]
    assert len(top) == 40


def test_matrix_equals_the_restatement_in_both_formats(world, mtx_run):
    _, dense, _ = expected(world, [0.25] * 4, 1e-5, ["PLANT", "RND.2"])
    base = str(world["dir"] / "npz")
    assert run(["motifs", "--fasta", world["fasta"], "--motifs", world["motifs"], "--bed", world["bed"], "--pvalue", "1e-5", "--format", "npz",
                "--out", base]) == 0
    for suffix in (".motifs.sites.bed.gz", ".motifs.txt"):
        assert open(mtx_run + suffix, "rb").read() == open(base + suffix, "rb").read(), suffix
    assert sorted(os.listdir(str(world["dir"]))).count("npz.motifs.npz") == 1 and not os.path.exists(base + ".motifs.mtx.gz")
    z = np.load(base + ".motifs.npz")
    assert z["shape"].tolist() == list(dense.shape) and [m.decode() for m in z["motifs"]] == ["PLANT", "RND.2"]
    got = np.zeros(dense.shape, np.int32)
    for i in range(dense.shape[0]):
        sl = slice(z["indptr"][i], z["indptr"][i + 1])
        assert np.all(np.diff(z["indices"][sl]) > 0)
        got[i, z["indices"][sl]] = z["data"][sl]
    assert np.array_equal(got, dense) and z["data"].dtype == np.int32 and np.all(z["data"] > 0)
    rows = world["rows"]
    assert z["region_chrom"].tolist() == [r[0] for r in rows] and z["region_start"].tolist() == [r[1] for r in rows]
    assert z["region_end"].tolist() == [r[2] for r in rows]
    # the MatrixMarket text, the names and the regions
    lines = gzip.open(mtx_run + ".motifs.mtx.gz", "rt").read().splitlines()
    assert lines[0].startswith("%%MatrixMarket") and lines[1] == "%d %d %d" % (dense.shape[0], dense.shape[1], np.count_nonzero(dense))
    got = np.zeros(dense.shape, np.int32)
    for l in lines[2:]:
        i, j, v = (int(x) for x in l.split())
        got[i - 1, j - 1] = v
    assert np.array_equal(got, dense)
    assert open(mtx_run + ".motifs.names.tsv").read() == "PLANT\tplanted factor\nRND.2\t\n"
    assert open(mtx_run + ".motifs.regions.bed").read() == "".join("%s\t%d\t%d\n" % r for r in rows)
    # the site across the border of two abutting windows is a site and counts in neither
    i0, i1 = rows.index(("chrA", 4500, 5000)), rows.index(("chrA", 5000, 5500))
    assert dense[i0, 0] == 0 and dense[i1, 0] == 0
    assert dense[rows.index(("chrB", 1400, 2600)), 0] >= 1 and dense[:, 0].sum() > 40 - 1      # overlapping windows count a site twice


def test_summary_adds_up(world, mtx_run):
    sites, dense, thr = expected(world, [0.25] * 4, 1e-5, ["PLANT", "RND.2"])
    head, motifs, totals = read_summary(mtx_run + ".motifs.txt")
    assert head["background"] == ["uniform"] + ["0.250000"] * 4 and float(head["pvalue"][0]) == 1e-5 and float(head["pseudocount"][0]) == 0.8
    assert [m[0] for m in motifs] == ["PLANT", "RND.2"] and motifs[0][1] == "planted factor" and [int(m[2]) for m in motifs] == [12, 9]
    for k, m in enumerate(motifs):
        mine = [s.split("\t") for s in sites if s.split("\t")[3] == m[0]]
        assert int(m[6]) == sum(r[5] == "+" for r in mine) and int(m[7]) == sum(r[5] == "-" for r in mine)
        assert int(m[8]) == np.count_nonzero(dense[:, k])
        assert m[3] == "%.2f" % (thr[k][2] / 100.0)
        if thr[k][1] is None:
            assert m[4] == "NA" and m[5] == "NA" and int(m[6]) == int(m[7]) == 0
        else:
            assert m[4] == "%.2f" % (thr[k][0] / 100.0) and abs(float(m[5]) - thr[k][1]) <= 1e-5 * thr[k][1] and float(m[5]) <= 1e-5
    merged = {c: R.merged([r[1] for r in world["rows"] if r[0] == c], [r[2] for r in world["rows"] if r[0] == c]) for c in NAMES}
    assert totals == dict(bases_scanned=sum(e - s for c in NAMES for s, e in merged[c]), scan_intervals=sum(len(v) for v in merged.values()),
                          windows=len(world["rows"]), hits=len(sites))
    assert totals["hits"] == sum(int(m[6]) + int(m[7]) for m in motifs)


def test_only_restricts_every_output(world):
    base = str(world["dir"] / "only")
    assert run(["motifs", "--fasta", world["fasta"], "--motifs", world["motifs"], "--bed", world["bed"], "--pvalue", "1e-5", "--only", "RND.2",
                "--out", base]) == 0
    sites, dense, _ = expected(world, [0.25] * 4, 1e-5, ["RND.2"])
    assert read_sites(base + ".motifs.sites.bed.gz") == sites
    assert open(base + ".motifs.names.tsv").read() == "RND.2\t\n"
    lines = gzip.open(base + ".motifs.mtx.gz", "rt").read().splitlines()
    assert lines[1] == "%d 1 %d" % (dense.shape[0], np.count_nonzero(dense))
    _, motifs, totals = read_summary(base + ".motifs.txt")
    assert [m[0] for m in motifs] == ["RND.2"] and totals["hits"] == len(sites)


def test_bg_regions_and_no_sites(world):
    base = str(world["dir"] / "regions")
    assert run(["motifs", "--fasta", world["fasta"], "--motifs", world["motifs"], "--bed", world["bed"], "--pvalue", "1e-4", "--bg", "regions",
                "--no_sites", "--format", "npz", "--out", base]) == 0
    assert not os.path.exists(base + ".motifs.sites.bed.gz")
    acgt = np.zeros(4, np.int64)
    for c in NAMES:
        seq = np.frombuffer(world["seqs"][c], np.uint8)
        for s, e in R.merged([r[1] for r in world["rows"] if r[0] == c], [r[2] for r in world["rows"] if r[0] == c]):
            code = R.CODE[seq[s:e]]
            acgt += np.bincount(code, minlength=5)[:4]
    at, cg = (acgt[0] + acgt[3]) / (2.0 * acgt.sum()), (acgt[1] + acgt[2]) / (2.0 * acgt.sum())
    bg = [at, cg, cg, at]
    head, motifs, _ = read_summary(base + ".motifs.txt")
    assert head["background"] == ["regions"] + ["%.6f" % x for x in bg]
    _, dense, thr = expected(world, bg, 1e-4, ["PLANT", "RND.2"])
    assert [m[4] for m in motifs] == ["%.2f" % (t[0] / 100.0) for t in thr]
    z = np.load(base + ".motifs.npz")
    got = np.zeros(dense.shape, np.int32)
    got[np.repeat(np.arange(dense.shape[0]), np.diff(z["indptr"])), z["indices"]] = z["data"]
    assert np.array_equal(got, dense)


def test_whole_genome_without_a_bed(world):
    base = str(world["dir"] / "whole")
    assert run(["motifs", "--fasta", world["fasta"], "--motifs", world["motifs"], "--only", "PLANT", "--pvalue", "1e-5", "--format", "npz",
                "--out", base]) == 0
    rows = read_sites(base + ".motifs.sites.bed.gz")
    found = {tuple(r.split("\t")[i] for i in (0, 1, 5)) for r in rows}
    assert all((c, str(x), s) in found for c, x, s in world["plants"])
    z = np.load(base + ".motifs.npz")
    assert z["shape"].tolist() == [3, 1] and z["region_end"].tolist() == [N] * 3 and int(z["data"].sum()) == len(rows)


def test_nucleotide_reads_the_sites_file(world):
    base = str(world["dir"] / "plant")
    assert run(["motifs", "--fasta", world["fasta"], "--motifs", world["motifs"], "--bed", world["bed"], "--pvalue", "1e-5", "--only", "PLANT",
                "--out", base]) == 0
    out = str(world["dir"] / "plantnuc")
    assert run(["nucleotide", "--fasta", world["fasta"], "--bed", base + ".motifs.sites.bed.gz", "--strand", "6", "--up", "10", "--down", "10",
                "--out", out]) == 0
    table = {l.split("\t")[0]: [float(x) for x in l.split("\t")[1:]] for l in open(out + ".nucfreq.txt").read().splitlines()}
    assert sorted(table) == ["A", "C", "G", "T"] and all(len(v) == 21 for v in table.values())
    # a site's centre is its 7th base on either strand (minus sites are read as their reverse complement): columns 4 .. 15 hold the motif
    best = "".join(max("ACGT", key=lambda b: table[b][col]) for col in range(4, 16))
    assert best == WORD
    # (`nucleotide` keeps the reference's rule for soft-masked minus-strand windows, so the lower-case plants dilute the share)
    assert min(table[ch][4 + j] for j, ch in enumerate(WORD)) > 0.5
