"""`pyatac doublets` end to end on the GPU on the planted case of tests/knn_ref.py: the written neighbour lists are the restatement's on the
written points (the device LSI differs from NumPy's in the last bits, so the check is self-consistency, not a comparison with a host
run), the planted doublets are recovered, and two runs write the same bytes."""
import gzip

import numpy as np
import pytest

import knn_ref as K

pytestmark = pytest.mark.gpu

FILES = (".doublets.tsv", ".doublets.cells.tsv", ".doublets.npz", ".doublets.txt")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    from nucleoatac_amd.pyatac.cli import main
    from nucleoatac_amd.pyatac.get_cellcounts import mtx_text
    d = tmp_path_factory.mktemp("doublets_gpu")
    ip, ix, da, n, group, pa, pb = K.planted_doublets(seed=1)
    barcodes = [b"CELL%04d-1" % k for k in range(n)]
    counts = str(d / "pl.cellcounts.mtx.gz")
    with gzip.open(counts, "wb") as f:
        f.write(mtx_text(ip, ix, da, n))
    with open(str(d / "pl.cellcounts.barcodes.tsv"), "wb") as f:
        f.write(b"".join(b + b"\n" for b in barcodes))
    out = []
    for name in ("a", "b"):
        assert main(["doublets", "--counts", counts, "--components", "10", "--out", str(d / name)]) == 0
        out.append([open(str(d / name) + x, "rb").read() for x in FILES])
    return dict(out=out, z=np.load(str(d / "a.doublets.npz")), group=group, pa=pa, pb=pb, barcodes=barcodes, d=d)


def test_the_written_neighbours_are_the_restatements_on_the_written_points(runs):
    z = runs["z"]
    P = z["points"]
    assert P.shape == (1320, 9) and z["knn_index"].shape == (440, 30) and z["knn_index"].dtype == np.int32
    assert K.same((z["knn_index"], z["knn_dist2"]), K.knn(P, 30, queries=P[:440], self_offset=0))
    assert np.array_equal(z["synthetic_neighbors"], (z["knn_index"] >= 440).sum(axis=1))
    g = np.random.default_rng(1)
    g.standard_normal((3000, 20))
    assert np.array_equal(z["pair_a"], g.integers(0, 440, 880)) and np.array_equal(z["pair_b"], g.integers(0, 440, 880))
    summary = dict(x.split("\t") for x in runs["out"][0][3].decode().splitlines())
    assert (summary["arm"], summary["k"], summary["k_adj"], summary["simulated"], summary["dimensions"]) == ("wave", "10", "30", "880", "9")


def test_planted_doublets_are_recovered(runs):
    """the condition of tests/test_doublets_host.py: at least 26 of the 33 heterotypic planted doublets among the 40 highest scores"""
    z = runs["z"]
    found, het = K.recovered(z["score"], runs["group"], runs["pa"], runs["pb"])
    print("heterotypic planted doublets among the 40 highest scores: %d of %d" % (found, het))
    assert het == 33 and found >= 26
    top = int(np.lexsort((np.arange(440), -z["score"]))[0])
    assert np.flatnonzero(z["flagged"]).tolist() == [top]
    assert runs["out"][0][1].splitlines() == [b for k, b in enumerate(runs["barcodes"]) if k != top]


def test_two_runs_write_the_same_bytes(runs):
    assert runs["out"][0] == runs["out"][1] and all(len(b) > 0 for b in runs["out"][0])
