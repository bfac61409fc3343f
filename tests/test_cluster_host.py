"""CPU: the host part of `pyatac cluster` (nucleoatac_amd/pyatac/get_cluster.py) -- reading either output of `cellcounts`, the TF-IDF
weights, the depth rule, k-means with its fixed rules, the files and the error paths -- against hand-computed values and against the
restatement of tests/lsi_ref.py, whose SVD stands in for Context.sparse_lsi here (the device call is tests/test_gpu_lsi.py)."""
import gzip
import os

import numpy as np
import pytest

import lsi_ref as R
from nucleoatac_amd.pyatac import get_cluster as GC

# windows x cells: cell 3 has no count, window 3 has none, window 1 is seen in one cell
SMALL = np.array([[2, 0, 1, 0, 0],
                  [0, 3, 0, 0, 0],
                  [1, 1, 0, 0, 2],
                  [0, 0, 0, 0, 0]])


def _args(argv):
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    return pyatac_parser().parse_args(["cluster"] + argv)


def _write_counts(base, indptr, indices, data, barcodes, fmt):
    """what `pyatac cellcounts --format fmt` writes, as far as `cluster` reads it"""
    from nucleoatac_amd.pyatac.get_cellcounts import mtx_text
    if fmt == "npz":
        np.savez_compressed(base + ".cellcounts.npz", indptr=indptr, indices=indices, data=data,
                            shape=np.array([len(indptr) - 1, len(barcodes)], np.int64), barcodes=np.array(barcodes, dtype="S"))
        return base + ".cellcounts.npz"
    with gzip.open(base + ".cellcounts.mtx.gz", "wb") as f:
        f.write(mtx_text(indptr, indices, data, len(barcodes)))
    with open(base + ".cellcounts.barcodes.tsv", "wb") as f:
        f.write(b"".join(b + b"\n" for b in barcodes))
    return base + ".cellcounts.mtx.gz"


def test_weights_by_hand():
    ip, ix, da = R.csr_of(SMALL)
    total, rw, cs = GC.tfidf_weights(ip, ix, da, 5)
    assert total.tolist() == [3, 4, 1, 0, 2]
    assert np.array_equal(cs, [1 / 3, 1 / 4, 1.0, 0.0, 1 / 2]) and np.array_equal(rw, [4 / 3, 4 / 3, 4 / 4, 0.0])       # N = 4 cells kept
    total, rw, cs = GC.tfidf_weights(ip, ix, da, 5, binarize=True)
    assert total.tolist() == [2, 2, 1, 0, 1]
    assert np.array_equal(cs, [0.5, 0.5, 1.0, 0.0, 1.0]) and np.array_equal(rw, [4 / 2, 4 / 1, 4 / 3, 0.0])
    total, rw, cs = GC.tfidf_weights(ip, ix, da, 5, min_cells=2)
    assert total.tolist() == [3, 4, 1, 0, 2] and np.array_equal(rw, [4 / 3, 0.0, 1.0, 0.0])                            # window 1: one cell
    for kw in (dict(), dict(binarize=True), dict(min_cells=2), dict(binarize=True, min_cells=3)):
        for a, b in zip(GC.tfidf_weights(ip, ix, da, 5, **kw), R.weights(ip, ix, da, 5, **kw)):
            assert np.array_equal(a, b)
    # the weighted entry itself: window 2, cell 4 holds 2 -> 2 / 2 * 4 / 4
    X = R.weighted_matrix(ip, ix, da, 5, *GC.tfidf_weights(ip, ix, da, 5)[1:], transform="linear").toarray()
    assert X.shape == (5, 4) and X[4, 2] == 1.0 and X[0, 0] == 2 / 3 * 4 / 3 and not X[3].any() and not X[:, 3].any()


def test_depth_correlation_rule():
    rng = np.random.default_rng(3)
    total = rng.integers(10, 1000, 50)
    d = np.log10(total)
    E = np.stack([3 * d + 1, -d, rng.standard_normal(50), np.ones(50), d + 2.0 * rng.standard_normal(50)], axis=1)
    cor = GC.depth_correlation(E, total)
    assert abs(cor[0] - 1) < 1e-12 and abs(cor[1] + 1) < 1e-12 and cor[3] == 0.0
    assert np.allclose(cor[[0, 1, 2, 4]], [np.corrcoef(E[:, j], d)[0, 1] for j in (0, 1, 2, 4)], rtol=0, atol=1e-12)
    # through the command's computation: U carries E, sigma is 1; components 1 and 2 go, whatever their sign; cells without counts do not count
    A = np.zeros((8, 52), np.int64)
    A[0, :50] = total - 7
    A[1:, :50] = 1                         # the column sums are `total`; cells 50 and 51 have no count
    ip, ix, da = R.csr_of(A)
    U = np.zeros((52, 8))
    U[:50, :5] = E
    U[50:, :5] = 1e6                       # dropped cells: never looked at

    def svd(*a, **k):
        return np.ones(8), U, np.zeros((8, 8))
    res = GC.cluster_cells(ip, ix, da, 52, 2, components=5, oversample=3, max_depth_cor=0.75, svd=svd)
    want = [j for j in range(5) if not abs(cor[j]) > 0.75]
    assert want[:2] == [2, 3] and np.array_equal(res["total"][:50], total) and np.allclose(res["depth_cor"], cor, rtol=0, atol=1e-12)
    assert res["components_kept"].tolist() == want and res["cell_keep"].sum() == 50 and res["embedding"].shape == (50, len(want))
    assert np.allclose(np.linalg.norm(res["embedding"], axis=1), 1.0, rtol=0, atol=1e-14)
    emb, cor2, comp = R.embedding(np.ones(8), U, res["total"], 5, 0.75)
    assert comp == want and np.allclose(emb, res["embedding"], rtol=0, atol=1e-14) and np.allclose(cor2, res["depth_cor"], rtol=0, atol=1e-12)
    # a zero row stays zero
    assert np.array_equal(GC.unit_rows(np.array([[0.0, 0.0], [3.0, 4.0]])), [[0.0, 0.0], [0.6, 0.8]])


def test_kmeans_rules():
    # every row is as far from the mean as every other: the first centre is row 0; rows 1 and 3 are as far from it: the second is row 1
    X = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 0.0], [2.0, 0.0]])
    raw, it = GC.kmeans(X, 2)
    assert raw.tolist() == [0, 1, 0, 1] and it == 2
    rank, sizes = GC.name_clusters(raw, 2)
    assert rank[raw].tolist() == [0, 1, 0, 1] and sizes.tolist() == [2, 2]                 # equal sizes: the lowest cell index names
    # a row as near to two centres goes to the lower one
    raw, it = GC.kmeans(np.array([[0.0], [2.0], [1.0]]), 2)
    assert raw.tolist() == [0, 1, 0]
    # more clusters than distinct rows: the third centre repeats row 0, loses every row to the second, keeps its place; named last
    X = np.array([[0.0], [0.0], [1.0]])
    raw, it = GC.kmeans(X, 3)
    assert raw.tolist() == [1, 1, 0]
    rank, sizes = GC.name_clusters(raw, 3)
    assert rank[raw].tolist() == [0, 0, 1] and sizes.tolist() == [2, 1, 0] and rank.tolist() == [1, 0, 2]
    # naming by size: the big cluster is c1 wherever its centre came from
    X = np.array([[5.0], [0.0], [0.1], [0.2], [5.1]])
    raw, it = GC.kmeans(X, 2)
    rank, sizes = GC.name_clusters(raw, 2)
    assert rank[raw].tolist() == [1, 0, 0, 0, 1] and sizes.tolist() == [3, 2]
    # --max_iter stops the steps
    rng = np.random.default_rng(0)
    X = rng.standard_normal((300, 4))
    assert GC.kmeans(X, 5, max_iter=1)[1] == 1 and GC.kmeans(X, 5, max_iter=2)[1] == 2
    for k in (1, 3, 7):
        raw, it = GC.kmeans(X, k)
        rank, sizes = GC.name_clusters(raw, k)
        names, sizes_ref, steps = R.kmeans(X, k)
        assert np.array_equal(rank[raw], names) and sizes.tolist() == sizes_ref and it == steps and sizes.sum() == 300
        assert np.all(np.diff(sizes) <= 0)


def test_parser_defaults():
    a = _args(["--counts", "x.cellcounts.npz", "--clusters", "7"])
    assert (a.counts, a.clusters, a.components, a.oversample, a.iterations, a.method, a.binarize, a.min_cells, a.max_depth_cor, a.max_iter,
            a.seed, a.out) == ("x.cellcounts.npz", 7, 30, 10, 4, "log", False, 1, 0.75, 100, 1, None)
    a = _args(["--counts", "x", "--clusters", "2", "--method", "linear", "--binarize", "--out", "o"])
    assert a.method == "linear" and a.binarize and a.out == "o"
    with pytest.raises(SystemExit):
        _args(["--counts", "x"])
    with pytest.raises(SystemExit):
        _args(["--clusters", "3"])
    assert GC.default_base("/a/b/run1.cellcounts.mtx.gz") == "run1" and GC.default_base("r.cellcounts.npz") == "r" and GC.default_base("m.npz") == "m"


@pytest.fixture(scope="module")
def planted():
    A, group = R.planted()
    return R.csr_of(A) + (A.shape[1], group)


@pytest.fixture(scope="module")
def planted_files(planted, tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_host")
    ip, ix, da, n, group = planted
    barcodes = [b"CELL%04d-1" % k for k in range(n)]
    paths = {fmt: _write_counts(str(d / "pl"), ip, ix, da, barcodes, fmt) for fmt in ("npz", "mtx")}
    return dict(d=d, paths=paths, barcodes=barcodes, group=group)


def test_planted_groups_are_recovered(planted):
    """400 cells in 4 groups of 100, 3,000 windows, depths 300 to 3,000, each group 6x enriched in its own 600 windows"""
    ip, ix, da, n, group = planted
    res = GC.cluster_cells(ip, ix, da, n, 4, components=10, svd=R.sparse_lsi)
    table = np.zeros((4, 4), np.int64)
    np.add.at(table, (group, res["labels"]), 1)
    assert np.array_equal(np.sort(table.ravel())[-4:], [100] * 4) and (table > 0).sum() == 4                  # a permutation matrix x 100
    assert abs(res["depth_cor"][0]) > 0.75 and 0 not in res["components_kept"].tolist()
    assert np.all(np.abs(res["depth_cor"][1:]) < 0.75) and res["components_kept"].tolist() == list(range(1, 10))
    assert res["sizes"].tolist() == [100] * 4 and res["labels"][0] == 0                                      # equal sizes: cell 0 is in c1
    # the restated post-processing agrees
    tot, rw, cs = R.weights(ip, ix, da, n)
    q0 = np.random.default_rng(1).standard_normal((len(ip) - 1, 20))
    sigma, U, V = R.sparse_lsi(ip, ix, da, n, rw, cs, 20, 4, q0)
    emb, cor, comp = R.embedding(sigma, U, tot, 10, 0.75)
    assert np.array_equal(R.kmeans(emb, 4)[0], res["labels"]) and np.array_equal(sigma, res["sigma"])


def test_both_inputs_give_the_same_files(planted_files, tmp_path, monkeypatch):
    from nucleoatac_amd.pyatac.cellgroups import read_groups
    monkeypatch.chdir(tmp_path)
    out = {}
    for fmt in ("npz", "mtx"):
        a = _args(["--counts", planted_files["paths"][fmt], "--clusters", "4", "--components", "10", "--out", fmt])
        paths = GC.get_cluster(a, svd=R.sparse_lsi)
        assert paths == [fmt + x for x in (".clusters.tsv", ".lsi.npz", ".cluster.txt")]
        out[fmt] = [open(p, "rb").read() for p in paths]
    assert out["npz"] == out["mtx"]
    assert sorted(os.listdir(".")) == sorted(f + x for f in ("npz", "mtx") for x in (".clusters.tsv", ".lsi.npz", ".cluster.txt"))
    a, b = (GC.read_counts(planted_files["paths"][f]) for f in ("npz", "mtx"))
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[:3], b[:3])) and a[3] == b[3] == planted_files["barcodes"]
    # the table is what `split --groups` reads, in matrix column order
    g = read_groups("npz.clusters.tsv")
    assert g.barcodes == planted_files["barcodes"] and sorted(g.names) == ["c1", "c2", "c3", "c4"]
    group = planted_files["group"]
    for k in range(4):
        assert len({g.group_of[c] for c in np.flatnonzero(group == k)}) == 1
    z = np.load("npz.lsi.npz")
    assert sorted(z.files) == ["barcodes", "components", "depth_cor", "embedding", "kept", "labels", "sigma"]
    assert z["embedding"].shape == (400, 9) and z["sigma"].shape == (20,) and z["depth_cor"].shape == (10,) and z["kept"].all()
    assert z["components"].tolist() == list(range(1, 10)) and [b"c%d" % (l + 1) for l in z["labels"]] == \
        [line.split(b"\t")[1] for line in out["npz"][0].splitlines()]
    summary = dict(x.split("\t") for x in out["npz"][2].decode().splitlines())
    assert summary == dict(cells_listed="400", cells_kept="400", cells_dropped="0", windows_kept=str(int((np.diff(a[0]) > 0).sum())),
                           windows_dropped=str(int((np.diff(a[0]) == 0).sum())), nnz=str(len(a[1])), r="20", iterations="4",
                           components_removed="1", kmeans_iterations=summary["kmeans_iterations"], c1="100", c2="100", c3="100", c4="100")


def test_dropped_cells_are_counted_and_absent(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(9)
    A = rng.poisson(0.6, (40, 14))
    A[:, 5] = 0
    A[7] = 0
    ip, ix, da = R.csr_of(A)
    barcodes = [b"B%02d" % k for k in range(14)]
    a = _args(["--counts", _write_counts("d", ip, ix, da, barcodes, "npz"), "--clusters", "2", "--components", "3", "--oversample", "2",
               "--max_depth_cor", "1.0"])
    GC.get_cluster(a, svd=R.sparse_lsi)
    rows = open("d.clusters.tsv", "rb").read().splitlines()
    assert [r.split(b"\t")[0] for r in rows] == [b for k, b in enumerate(barcodes) if k != 5]
    summary = dict(x.split("\t") for x in open("d.cluster.txt").read().splitlines())
    assert (summary["cells_listed"], summary["cells_kept"], summary["cells_dropped"]) == ("14", "13", "1")
    assert int(summary["windows_dropped"]) >= 1 and summary["components_removed"] == "none"
    z = np.load("d.lsi.npz")
    assert z["kept"].tolist() == [k != 5 for k in range(14)] and len(z["labels"]) == 13


def test_every_error_leaves_nothing(planted_files, tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac.cli import main
    monkeypatch.chdir(tmp_path)
    good = planted_files["paths"]["npz"]
    ip, ix, da = R.csr_of(np.outer([1, 2, 1, 3, 1, 1, 2, 1], [1, 1, 2, 1, 3, 1, 1]) + np.outer([0, 1, 0, 0, 2, 0, 1, 0], [0, 2, 0, 1, 0, 0, 1]))
    low = _write_counts("low", ip, ix, da, [b"L%d" % k for k in range(7)], "npz")                  # rank 2
    lone = str(tmp_path / "lone.cellcounts.mtx.gz")
    with gzip.open(lone, "wb") as f:
        f.write(b"%%MatrixMarket matrix coordinate integer general\n1 1 1\n1 1 1\n")
    open("junk.cellcounts.npz", "wb").write(b"")
    np.savez("other.npz", x=np.zeros(3))
    before = sorted(os.listdir("."))
    # through the command line: everything that is decided before the SVD
    for argv, message in ((["--counts", good, "--clusters", "0"], "--clusters must be at least 1"),
                          (["--counts", good, "--clusters", "3", "--components", "60"], "their sum at most 64"),
                          (["--counts", good, "--clusters", "3", "--components", "0"], "--components must be at least 1"),
                          (["--counts", good, "--clusters", "3", "--oversample", "-1"], "--oversample at least 0"),
                          (["--counts", good, "--clusters", "3", "--iterations", "0"], "must be at least 1"),
                          (["--counts", good, "--clusters", "3", "--max_iter", "0"], "must be at least 1"),
                          (["--counts", good, "--clusters", "3", "--min_cells", "0"], "must be at least 1"),
                          (["--counts", good, "--clusters", "3", "--max_depth_cor", "1.5"], "--max_depth_cor must be in [0, 1]"),
                          (["--counts", str(tmp_path / "missing.cellcounts.npz"), "--clusters", "3"], "missing.cellcounts.npz: no such file"),
                          (["--counts", lone, "--clusters", "3"], "lone.cellcounts.barcodes.tsv: no such file"),
                          (["--counts", "other.npz", "--clusters", "3"], "not a cellcounts .npz"),
                          (["--counts", "junk.cellcounts.npz", "--clusters", "3"], "not a cellcounts .npz"),
                          (["--counts", good, "--clusters", "401"], "400 cells kept, fewer than the 401 clusters"),
                          (["--counts", low, "--clusters", "2", "--components", "6", "--oversample", "2"], "lower --components")):
        assert main(["cluster"] + argv) == 1
        err = capsys.readouterr().err
        assert err.startswith("pyatac cluster: ") and message in err and err.count("\n") == 1
        assert sorted(os.listdir(".")) == before
    # behind the SVD: lost rank, and no component left
    with pytest.raises(GC.ClusterError, match="fewer than 4 independent directions: lower --components"):
        GC.get_cluster(_args(["--counts", low, "--clusters", "2", "--components", "3", "--oversample", "1", "--method", "linear"]),
                       svd=R.sparse_lsi)
    with pytest.raises(GC.ClusterError, match="none is left"):
        GC.get_cluster(_args(["--counts", good, "--clusters", "4", "--components", "5", "--max_depth_cor", "0"]), svd=R.sparse_lsi)

    def broken(*a, **k):
        raise ValueError("something else")
    with pytest.raises(ValueError, match="something else"):
        GC.get_cluster(_args(["--counts", good, "--clusters", "4"]), svd=broken)
    assert sorted(os.listdir(".")) == before
