"""`pyatac genescores` on the host: the window rule and the weight table against numbers written out here, the gene reader's errors, every
parameter rule, the command with the device call replaced by the NumPy restatement of tests/genescores_ref.py (the device call itself is
tests/test_gpu_genescores.py), the launch plan of the device call, and the gene names carried through `pyatac markers`.  No GPU."""
import gzip
import os

import numpy as np
import pytest

import genescores_ref as R
import markers_ref as MR
from helpers import bgzf_bytes
from nucleoatac_amd.pyatac import get_genescores as GG
from nucleoatac_amd.pyatac import get_markers as GM


def _args(argv, call="genescores"):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    return pyatac_parser().parse_args([call] + argv)


# ---- the window rule and the weights ---------------------------------------------------------------------------------------------------
def _both_rules(chrom, start, end, minus, *par, **kw):
    a = [np.asarray(v).tolist() for v in GG.gene_windows(np.array(chrom), np.array(start), np.array(end), np.array(minus, bool), *par, **kw)]
    b = [list(v) for v in R.gene_windows(chrom, start, end, minus, *par, **kw)]
    assert a == b
    return a


def test_window_rule_on_hand_made_genes():
    chrom = [0, 0, 0, 0, 1]
    start = [20000, 21500, 27000, 27500, 3000]
    end = [21000, 22000, 28000, 29000, 4000]
    bs, be, wl, wh = _both_rules(chrom, start, end, [False] * 5, 0, 1000, 10000)
    assert bs == start and be == end
    # gene 0: no gene before it, the next 500 bases on: closer than e_min, so the window still reaches e_min
    # gene 1: the one before ends 500 bases off (e_min wins), the next starts 5,000 bases on: between e_min and e_max, the window stops there
    # gene 2: stops at gene 1's end on the left; gene 3 overlaps it and limits nothing, so e_max on the right
    # gene 3: gene 2 overlaps it: the nearest gene wholly before is gene 1
    # gene 4: alone on its chromosome, clipped at 0
    assert wl == [10000, 20500, 22000, 22000, 0]
    assert wh == [22000, 27000, 38000, 39000, 14000]
    _, _, wl, wh = _both_rules(chrom, start, end, [False] * 5, 0, 1000, 10000, boundaries=False)
    assert wl == [10000, 11500, 17000, 17500, 0] and wh == [31000, 32000, 38000, 39000, 14000]
    # upstream: before the start of a plus gene (clipped at 0), behind the end of a minus gene; the bodies then bound each other
    bs, be, wl, wh = _both_rules([0, 0, 0], [200, 5000, 9000], [900, 6000, 9500], [False, True, False], 500, 100, 2000)
    assert bs == [0, 5000, 8500] and be == [900, 6500, 9500]
    assert wl == [0, 3000, 6500] and wh == [2900, 8500, 11500]
    # identical genes do not bound each other
    _, _, wl, wh = _both_rules([0, 0], [5000, 5000], [6000, 6000], [False, False], 0, 10, 100)
    assert wl == [4900, 4900] and wh == [6100, 6100]
    # e_min == e_max == 0: the body itself
    _, _, wl, wh = _both_rules([0], [50], [60], [True], 7, 0, 0)
    assert (wl, wh) == ([50], [67])


def test_weight_table_at_written_points():
    for (unit, decay, e_max), want in (((256, 5000, 100000), {0: 350, 5000: 188, 100000: 94}), ((4, 1, 10), {0: 5, 1: 3, 10: 1})):
        w = GG.weight_table(e_max, decay, unit)
        assert w.dtype == np.int32 and len(w) == e_max + 1 and np.array_equal(w, R.weight_table(e_max, decay, unit))
        assert {d: int(w[d]) for d in want} == want and w.min() >= 1 and np.all(np.diff(w) <= 0)
    assert GG.weight_table(1 << 20, 1, 4).min() == 1 and GG.weight_table(0, 10 ** 7, 65536).tolist() == [89645]


# ---- the gene reader and the parameters ------------------------------------------------------------------------------------------------
def test_gene_reader_and_its_errors(tmp_path):
    path = str(tmp_path / "genes.bed")
    good = "# a comment\nchr2\t100\t200\tB\t0\t-\textra\n\nchr1\t5\t6\tA\t.\t+\nchr2\t100\t200\tB\t0\t.\n"
    open(path, "w").write(good)
    names, chrom, start, end, gene, minus = GG.read_genes(path)
    assert names == ["chr2", "chr1"] and chrom.tolist() == [0, 1, 0] and start.tolist() == [100, 5, 100] and end.tolist() == [200, 6, 200]
    assert gene == ["B", "A", "B"] and minus.tolist() == [True, False, False]
    names, chrom, start, end, gene, minus = GG.read_genes(path, name_col=6, strand_col=4)
    assert gene == ["-", "+", "."] and not minus.any()
    for bad, why in (("chr1\t5\t6\tA\t.\n", "line 6: 5 fields, at least 6 are needed"), ("chr1\t5\t5\tA\t.\t+\n", "line 6: end - start is 0, less than 1"),
                     ("chr1\t9\t5\tA\t.\t+\n", "line 6: end - start is -4, less than 1"), ("chr1\t5\t6\t\t.\t+\n", "line 6: the name in column 4 is empty"),
                     ("chr1\t5\t6\t%s\t.\t+\n" % ("N" * 256), "line 6: the name in column 4 has 256 bytes, more than 255"),
                     ("chr1\tx\t6\tA\t.\t+\n", "line 6: start and end must be integers")):
        open(path, "w").write(good + bad)
        with pytest.raises(GG.GenescoresError) as e:
            GG.read_genes(path)
        assert str(e.value) == "%s: %s" % (path, why)
    open(path, "w").write(good + "chr1\t5\t6\t%s\t.\t+\n" % ("N" * 255))
    assert GG.read_genes(path)[4][-1] == "N" * 255
    open(path, "w").write("")
    assert len(GG.read_genes(path)[2]) == 0


def test_every_parameter_rule():
    ok = dict(upstream=5000, min_extend=1000, max_extend=100000, decay=5000, unit=256, lower=0, upper=1000)
    GG.check_params(**ok)
    GG.check_params(upstream=0, min_extend=0, max_extend=0, decay=1, unit=4, lower=0, upper=1)
    GG.check_params(upstream=1 << 20, min_extend=1 << 20, max_extend=1 << 20, decay=10 ** 7, unit=65536, lower=49999, upper=50000)
    for change, text in ((dict(upstream=-1), "--upstream"), (dict(upstream=(1 << 20) + 1), "--upstream"), (dict(min_extend=-1), "--min_extend"),
                         (dict(min_extend=100001), "--min_extend"), (dict(max_extend=(1 << 20) + 1), "--max_extend"), (dict(decay=0), "--decay"),
                         (dict(decay=10 ** 7 + 1), "--decay"), (dict(unit=3), "--unit"), (dict(unit=65537), "--unit"), (dict(lower=-1), "--lower"),
                         (dict(lower=1000), "--lower"), (dict(upper=50001), "--upper"), (dict(name_col=3), "--name"), (dict(strand_col=4), "--strand")):
        with pytest.raises(GG.GenescoresError) as e:
            GG.check_params(**dict(ok, **change))
        assert text in str(e.value) and "\n" not in str(e.value)


# ---- the command -------------------------------------------------------------------------------------------------------------------------
GENES = ("#name\n"
         "chr1\t20000\t21000\tAlpha\t0\t+\n"
         "chr1\t21500\t22000\tBeta\t0\t-\n"
         "\n"
         "chr2\t3000\t9000\tGamma\t0\t+\n"
         "chr1\t27000\t28000\tDelta\t0\t+\n"
         "chr9\t100\t200\tNowhere\t0\t+\n"
         "chr1\t27500\t29000\tDelta\t0\t-\n"
         "chr2\t30000\t30001\tTiny\t0\t.\n")
PARAMS = ["--upstream", "300", "--min_extend", "500", "--max_extend", "4000", "--decay", "700", "--unit", "50", "--lower", "1", "--upper", "600"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("genescores_host")
    rng = np.random.default_rng(11)
    barcodes = [b"CELL%03d" % i for i in range(30)]
    lines, recs = [], {"chr1": [], "chr2": []}
    for _ in range(4000):
        c = "chr1" if rng.random() < 0.6 else "chr2"
        s = int(rng.integers(0, 45000))
        e = s + int(rng.choice([0, 1, 40, 150, 320, 599, 600, 900]))
        k = int(rng.integers(0, 33))
        if k < 29:                                                     # CELL029 has no line; 29 .. 32 are barcodes the table does not list
            recs[c].append((s - 4, e - s + 8, k))
        lines.append("%s\t%d\t%d\t%s\t1\n" % (c, s, e, barcodes[k].decode() if k < 29 else "OTHER%d" % k))
    frag, genes, cells = str(d / "frags.tsv.gz"), str(d / "my.genes.bed"), str(d / "cells.tsv")
    open(frag, "wb").write(bgzf_bytes("".join(lines).encode(), blk=5000))
    open(genes, "w").write(GENES)
    open(cells, "wb").write(b"barcode\tcluster\n" + b"".join(b + b"\tc1\n" for b in barcodes))
    # the expectation, gene by gene, from the lines themselves
    chrom = ["chr1", "chr1", "chr2", "chr1", "chr9", "chr1", "chr2"]
    start, end = [20000, 21500, 3000, 27000, 100, 27500, 30000], [21000, 22000, 9000, 28000, 200, 29000, 30001]
    minus = [False, True, False, False, False, True, False]
    bs, be, wl, wh = R.gene_windows(chrom, start, end, minus, 300, 500, 4000)
    weight = R.weight_table(4000, 700, 50)
    dense, hits = np.zeros((7, 30), np.int64), np.zeros(7, np.int64)
    for g in range(7):
        if chrom[g] in recs:
            a = np.array(sorted(recs[chrom[g]]), np.int64)
            x, c = R.insertions(a[:, 0], a[:, 1], a[:, 2], 1, 600)
            dense[g], hits[g] = R.gene_row(x, c, 30, wl[g], wh[g], bs[g], be[g], weight)
    n_rec = sum(len(v) for v in recs.values())
    n_sized = sum(1 for v in recs.values() for r in v if 1 <= r[1] - 8 < 600)
    return dict(d=d, frag=frag, genes=genes, cells=cells, barcodes=barcodes, dense=dense, hits=hits, bs=bs, be=be, wl=wl, wh=wh, chrom=chrom,
                start=start, end=end, minus=minus, n_lines=len(lines), n_rec=n_rec, n_sized=n_sized)


def _cmd(world, out, extra=()):
    return ["--fragments", world["frag"], "--cells", world["cells"], "--header", "--genes", world["genes"], "--out", out] + PARAMS + list(extra)


def test_command_writes_every_file(world):
    from nucleoatac_amd.pyatac.get_cluster import read_counts
    from nucleoatac_amd.pyatac.get_deviations import read_regions
    d, dense = world["d"], world["dense"]
    mats, files = {}, {}
    for fmt in ("npz", "mtx"):
        for run in ("a", "b"):
            base = str(d / ("%s_%s" % (fmt, run)))
            ip, ix, da = GG.get_genescores(_args(_cmd(world, base, ["--format", fmt])), score=R.gene_cell_scores)
            got = np.zeros_like(dense)
            got[np.repeat(np.arange(7), np.diff(ip)), ix] = da
            assert np.array_equal(got, dense) and da.dtype == np.int32 and ix.dtype == np.int32
            names = sorted(f for f in os.listdir(str(d)) if f.startswith("%s_%s." % (fmt, run)))
            files[fmt, run] = [open(str(d / f), "rb").read() for f in names]
            tails = ["genes.tsv", "npz", "txt"] if fmt == "npz" else ["barcodes.tsv", "genes.tsv", "mtx.gz", "regions.bed", "txt"]
            assert names == ["%s_%s.genescores.%s" % (fmt, run, t) for t in tails]
        assert files[fmt, "a"] == files[fmt, "b"]                      # byte-identical reruns
        path = str(d / (fmt + "_a.genescores." + ("npz" if fmt == "npz" else "mtx.gz")))
        ip, ix, da, bcs = read_counts(path)
        assert bcs == world["barcodes"]
        mats[fmt] = (ip.tolist(), ix.tolist(), da.tolist())
        chrom, start, end = read_regions(path)
        assert chrom == world["chrom"] and start.tolist() == world["start"] and end.tolist() == world["end"]
    assert mats["npz"] == mats["mtx"] and dense.sum() > 0 and dense[4].sum() == 0 and np.count_nonzero(dense[[0, 1, 2, 3, 5]].sum(axis=1)) == 5
    assert files["npz", "a"][0] == files["mtx", "a"][1] and files["npz", "a"][2] == files["mtx", "a"][4]      # genes.tsv and txt
    z = np.load(str(d / "npz_a.genescores.npz"))
    assert z["region_name"].tolist() == ["Alpha", "Beta", "Gamma", "Delta", "Nowhere", "Delta", "Tiny"] and z["region_minus"].tolist() == world["minus"]
    for k, want in (("window_start", "wl"), ("window_end", "wh"), ("body_start", "bs"), ("body_end", "be")):
        assert z[k].tolist() == world[want] and z[k].dtype == np.int64
    assert z["params"].tolist() == [300, 500, 4000, 700, 50, 1, 600, 1] and z["shape"].tolist() == [7, 30] and z["data"].dtype == np.int32
    rows = files["npz", "a"][0].decode().split("\n")
    assert rows[0] == "#name\tchrom\tstart\tend\tstrand\tbody_start\tbody_end\twindow_start\twindow_end\thits\tcells\ttotal" and rows[-1] == ""
    for g, ln in enumerate(rows[1:-1]):
        assert ln == "%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (
            z["region_name"][g], world["chrom"][g], world["start"][g], world["end"][g], "-" if world["minus"][g] else "+", world["bs"][g], world["be"][g],
            world["wl"][g], world["wh"][g], world["hits"][g], np.count_nonzero(dense[g]), dense[g].sum())
    summary = dict(x.split("\t") for x in files["npz", "a"][2].decode().splitlines())
    h = world["hits"]
    assert summary == dict(barcodes_listed="30", barcodes_seen="29", data_lines=str(world["n_lines"]), unassigned_lines=str(world["n_lines"] - world["n_rec"]),
                           records_counted=str(world["n_sized"]), records_filtered_by_size=str(world["n_rec"] - world["n_sized"]), genes="7",
                           genes_with_hit=str(np.count_nonzero(h)), hits=str(h.sum()), entries=str(np.count_nonzero(dense)),
                           largest_entry=str(dense.max()), largest_column_sum=str(dense.sum(axis=0).max()),
                           rows_short=str(np.count_nonzero((h > 0) & (h <= 64))), rows_table=str(np.count_nonzero(h > 64)))
    assert 0 < world["n_sized"] < world["n_rec"] < world["n_lines"] and np.count_nonzero(h > 64)
    # --no_boundaries changes the windows and the stated parameter, and the default base is the gene file's name
    GG.get_genescores(_args(_cmd(world, str(d / "nb"), ["--no_boundaries"])), score=R.gene_cell_scores)
    z2 = np.load(str(d / "nb.genescores.npz"))
    assert z2["params"].tolist()[-1] == 0 and z2["window_start"].tolist() != world["wl"] and z2["body_start"].tolist() == world["bs"]


def test_default_base_and_mtx_layout(world, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    argv = _cmd(world, "x", ["--format", "mtx"])
    del argv[argv.index("--out"):argv.index("--out") + 2]
    GG.get_genescores(_args(argv), score=R.gene_cell_scores)
    assert sorted(os.listdir(".")) == ["my.genes.genescores." + t for t in ("barcodes.tsv", "genes.tsv", "mtx.gz", "regions.bed", "txt")]
    assert open("my.genes.genescores.regions.bed").read() == "".join("%s\t%d\t%d\n" % r for r in zip(world["chrom"], world["start"], world["end"]))
    text = gzip.open("my.genes.genescores.mtx.gz").read().decode().splitlines()
    assert text[0] == "%%MatrixMarket matrix coordinate integer general" and text[1] == "7 30 %d" % np.count_nonzero(world["dense"])


def test_refusals_write_nothing(world, capsys):
    from nucleoatac_amd._lib import NatacError
    from nucleoatac_amd.pyatac.cli import pyatac_main
    d = world["d"]
    base = str(d / "bad")

    def refused(argv, text, score=None):
        if score is None:
            assert pyatac_main(_args(argv)) == 1
            err = capsys.readouterr().err
            assert err.startswith("pyatac genescores: ") and err.endswith("\n") and err.count("\n") == 1 and text in err
        else:
            with pytest.raises(GG.GenescoresError) as e:
                GG.get_genescores(_args(argv), score=score)
            assert text in str(e.value) and "\n" not in str(e.value)
        assert not [f for f in os.listdir(str(d)) if f.startswith("bad.")]

    ok = _cmd(world, base)
    refused(ok + ["--unit", "3"], "--unit must be in [4, 65536] (got 3)")
    refused(ok + ["--decay", "0"], "--decay must be in [1, 10000000] (got 0)")
    refused(ok + ["--upstream", "-1"], "--upstream must be in")
    refused(ok + ["--min_extend", "5000"], "--min_extend <= --max_extend")
    refused(ok + ["--upper", "1"], "--lower < --upper")
    refused(ok + ["--name", "6"], "--name and --strand")
    for flag in ("--fragments", "--cells", "--genes"):
        argv = list(ok)
        argv[argv.index(flag) + 1] = str(d / "nope")
        refused(argv, "nope: no such file")
    short = str(d / "short.bed")
    open(short, "w").write(GENES + "chr1\t1\t2\tX\n")
    argv = list(ok)
    argv[argv.index("--genes") + 1] = short
    refused(argv, "short.bed: line 10: 4 fields, at least 6 are needed")

    # the device's refusal of an entry that could pass 2^31, and the host's of a column sum that does
    def device_refuses(*a, **kw):
        raise NatacError(-1, "gene 3: 30000 insertions count and the largest weight is 89645: an entry could reach 2^31")

    def huge_column(*a, **kw):
        res = list(R.gene_cell_scores(*a, **kw))
        res[2] = np.full(len(res[2]), 1 << 30, np.int32)
        return tuple(res)

    refused(ok, "gene 3: 30000 insertions count and the largest weight is 89645: an entry could reach 2^31: lower --unit (now 50)", score=device_refuses)
    refused(ok, "2^31 or more, and `markers` needs less: lower --unit (now 50)", score=huge_column)


# ---- the launch plan -----------------------------------------------------------------------------------------------------------------------
def test_plan_pins_the_arms_and_the_forced_values(monkeypatch):
    from nucleoatac_amd import _lib as L
    from nucleoatac_amd.device import gene_cell_scores_plan as plan
    for name in ("NATAC_GENESCORES_SHORT_MAX", "NATAC_GENESCORES_TILE"):
        monkeypatch.delenv(name, raising=False)
    assert (L.GENESCORES_SHORT_CAP, L.GENESCORES_TILE_CAP, L.GENESCORES_MAX_WEIGHT) == (64, 16384, 1 << 20)
    assert plan(5000, 10000, 4000) == dict(short_max=64, tile=16384, n_tiles=1, wg=256, lds_bytes=65536, grid=2048)
    assert plan(120, 200, 10) == dict(short_max=64, tile=256, n_tiles=1, wg=256, lds_bytes=1024, grid=10)
    assert plan(40, 20000, 5) == dict(short_max=64, tile=16384, n_tiles=2, wg=256, lds_bytes=65536, grid=10)
    assert [plan(10, n, 0)["tile"] for n in (1, 63, 256, 257, 512, 513, 16384, 16385, 1 << 23)] == [256, 256, 256, 512, 512, 1024, 16384, 16384, 16384]
    assert plan(10, 1 << 23, 10, n_cu=4) == dict(short_max=64, tile=16384, n_tiles=512, wg=256, lds_bytes=65536, grid=32)
    assert plan(10, 100, 0)["grid"] == 0
    monkeypatch.setenv("NATAC_GENESCORES_SHORT_MAX", "1")
    monkeypatch.setenv("NATAC_GENESCORES_TILE", "64")
    assert plan(120, 200, 100) == dict(short_max=1, tile=64, n_tiles=4, wg=256, lds_bytes=256, grid=400)
    assert plan(120, 65, 100)["n_tiles"] == 2 and plan(120, 64, 100)["n_tiles"] == 1
    monkeypatch.setenv("NATAC_GENESCORES_TILE", "16")
    assert (plan(120, 63, 1)["tile"], plan(120, 63, 1)["n_tiles"], plan(120, 63, 1)["lds_bytes"]) == (16, 4, 64)
    monkeypatch.setenv("NATAC_GENESCORES_SHORT_MAX", "64")
    monkeypatch.setenv("NATAC_GENESCORES_TILE", "16384")
    assert plan(120, 200, 100)["tile"] == 16384 and plan(120, 200, 100)["short_max"] == 64
    for sm, tile in (("0", "8"), ("65", "32768"), ("-3", "48"), ("x", "100"), ("", "")):       # outside their rules: ignored
        monkeypatch.setenv("NATAC_GENESCORES_SHORT_MAX", sm)
        monkeypatch.setenv("NATAC_GENESCORES_TILE", tile)
        assert plan(120, 200, 10) == dict(short_max=64, tile=256, n_tiles=1, wg=256, lds_bytes=1024, grid=10)
    for bad in ((0, 100, 0), (10, 0, 0), (10, (1 << 23) + 1, 0), (10, 100, -1), (10, 100, 11)):
        with pytest.raises(L.NatacError) as e:
            plan(*bad)
        assert "natac_gene_cell_scores_plan" in str(e.value)
    with pytest.raises(L.NatacError):
        plan(10, 100, 5, n_cu=0)


# ---- the cases of tests/test_gpu_genescores_launch_edges.py: sized for the grid before they reach a GPU ---------------------------------------
@pytest.mark.parametrize("n_cu", [256, 304])
def test_table_stride_case_exceeds_the_grid(n_cu, monkeypatch):
    from nucleoatac_amd.device import gene_cell_scores_plan as plan
    monkeypatch.setenv("NATAC_GENESCORES_SHORT_MAX", "1")
    monkeypatch.setenv("NATAC_GENESCORES_TILE", "16")
    most = plan(1 << 20, 200, 1 << 20, n_cu=n_cu)
    assert (most["tile"], most["n_tiles"], most["grid"]) == (16, 13, 8 * n_cu)
    n_genes = max(400, (most["grid"] + 500) // 13 + 60)
    case = R.make_case(seed=200, n_frags=6000, n_cells=200, n_genes=n_genes)
    ptr, col, val, hits = R.gene_cell_scores(*R.case_args(case), with_hits=True)
    assert np.array_equal(hits, R.window_hits(case))
    rows = np.flatnonzero(hits > 1)
    p = plan(n_genes, 200, len(rows), n_cu=n_cu)
    assert p == dict(short_max=1, tile=16, n_tiles=13, wg=256, lds_bytes=64, grid=8 * n_cu) and len(rows) * p["n_tiles"] > p["grid"] + 500
    pairs = R.tile_pairs(ptr, col, rows, 16, 13)
    assert pairs.sum() == sum(ptr[g + 1] - ptr[g] for g in rows) and pairs.max() == 16
    a, b = pairs[:len(pairs) - p["grid"]], pairs[p["grid"]:]            # the items a workgroup serves one after the other
    assert ((a >= 8) & (b == 0)).sum() >= 40 and ((a == 0) & (b >= 8)).sum() >= 30 and ((a > 0) & (b > 0) & (a != b)).sum() >= 500
    assert (hits == 1).sum() >= 1
    monkeypatch.setenv("NATAC_GENESCORES_TILE", "64")
    assert plan(n_genes, 200, len(rows), n_cu=n_cu)["n_tiles"] == 4
    monkeypatch.delenv("NATAC_GENESCORES_TILE")
    assert (plan(n_genes, 200, len(rows), n_cu=n_cu)["tile"], plan(n_genes, 200, len(rows), n_cu=n_cu)["n_tiles"]) == (256, 1)


def test_wave_stride_case_gives_waves_a_second_row(monkeypatch):
    """the wave kernels' grid does not follow the CU count: min(ceil(n_genes / 4), 16384) workgroups of 4 waves"""
    from nucleoatac_amd.device import gene_cell_scores_plan as plan
    waves = 4 * 16384
    case = R.make_case(seed=50, n_frags=1500, n_cells=50, n_genes=66000)
    hits = R.window_hits(case)
    assert len(hits) > waves + 400
    a, b = hits[:len(hits) - waves], hits[waves:]
    both = (a >= 1) & (a <= 64) & (b >= 1) & (b <= 64)
    assert both.sum() >= 100 and (both & (a != b)).sum() >= 50 and (b == 0).sum() >= 5 and (b > 64).sum() >= 5 and ((b == 1) & (a > 1)).sum() >= 3
    assert ((hits > 0) & (hits <= 64)).sum() >= 1000 and (hits == 1).sum() >= 1000
    monkeypatch.setenv("NATAC_GENESCORES_SHORT_MAX", "1")
    monkeypatch.delenv("NATAC_GENESCORES_TILE", raising=False)
    for n_cu in (256, 304):
        p = plan(66000, 50, int((hits > 1).sum()), n_cu=n_cu)
        assert (p["tile"], p["n_tiles"], p["grid"]) == (256, 1, 8 * n_cu) and (hits > 1).sum() > p["grid"] + 500


# ---- gene names through `pyatac markers` ---------------------------------------------------------------------------------------------------
def test_markers_carries_region_names(tmp_path):
    X, barcodes, grp = MR.planted_case(seed=5, n_groups=3, per_group=30, n_windows=90, planted=15)
    groups = str(tmp_path / "groups.tsv")
    open(groups, "w").write("".join("%s\tc%d\n" % (b.decode(), g + 1) for b, g in zip(barcodes, grp)))
    plain = MR.write_counts(str(tmp_path / "plain"), X, barcodes, "npz")
    names = ["GENE%d" % (i % 80) for i in range(90)]                   # not unique
    with np.load(plain) as z:
        arrays = {k: z[k] for k in z.files}
    named = str(tmp_path / "named.cellcounts.npz")
    np.savez_compressed(named, region_name=np.array(names, dtype="U"), **arrays)
    out = {}
    for key, cx in (("plain", plain), ("named", named)):
        paths = GM.get_markers(_args(["--counts", cx, "--groups", groups, "--min_cells", "5", "--out", str(tmp_path / ("out_" + key))], "markers"),
                               rank=MR.device_stand_in)
        out[key] = paths
    old_header = "group\tchrom\tstart\tend\tlog2fc\tauc\tpct_in\tpct_rest\tz\tp\tq"
    plain_rows = open(out["plain"][1]).read().split("\n")
    named_rows = open(out["named"][1]).read().split("\n")
    assert plain_rows[0] == old_header and named_rows[0] == old_header + "\tname" and len(plain_rows) == len(named_rows) > 20
    chrom, start, _ = MR.regions(90)
    where = {(c, int(s)): i for i, (c, s) in enumerate(zip(chrom, start))}
    for a, b in zip(plain_rows[1:-1], named_rows[1:-1]):
        f = b.split("\t")
        assert "\t".join(f[:-1]) == a and f[-1] == names[where[f[1], int(f[2])]]
    for a, b in zip(out["plain"][2:], out["named"][2:]):               # the summary and the BED files are unchanged
        assert open(a, "rb").read() == open(b, "rb").read()
    zp, zn = np.load(out["plain"][0]), np.load(out["named"][0])
    assert "region_name" not in zp.files and zn["region_name"].tolist() == names and sorted(zn.files) == sorted(zp.files + ["region_name"])
    for k in zp.files:
        assert np.array_equal(zp[k], zn[k], equal_nan=zp[k].dtype.kind == "f")
    # an input without the array gives the bytes of a run that never looked for it: the table through output_texts' default, and the
    # archive through the same writer without the extra member
    again = GM.get_markers(_args(["--counts", plain, "--groups", groups, "--min_cells", "5", "--out", str(tmp_path / "out_again")], "markers"),
                           rank=MR.device_stand_in)
    for a, b in zip(out["plain"], again):
        assert open(a, "rb").read() == open(b, "rb").read()


# ---- genescores -> markers on planted groups, with both device calls restated ----------------------------------------------------------------
def test_planted_groups_name_their_genes_on_the_cpu(tmp_path):
    w, _, found = R.planted_chain(tmp_path, R.gene_cell_scores, MR.device_stand_in)
    assert found == {"g%d" % k: {"GENE%d" % i for i in w["sets"][k]} for k in range(3)}
