"""`pyatac cluster` end to end on the GPU, between the commands it links: a synthetic single-cell fragment file with three planted groups
goes through `cellcounts`, `cluster --clusters 3` and `split --groups BASE.clusters.tsv`.  The labels are the planted groups up to naming,
the stores come out one per cluster, and the .mtx.gz route gives the same bytes as the .npz route."""
import os

import numpy as np
import pytest

from helpers import bgzf_bytes

pytestmark = pytest.mark.gpu

N_GROUPS, PER_GROUP, N_WINDOWS, SLOT, WIDTH = 3, 20, 60, 2000, 500


def synthetic_cells(seed=3):
    """(fragment file text, barcodes in order of first appearance in the table, group of every barcode, BED text): 60 cells of 60 to 140
    fragments; four fragments in five start in one of the 20 windows of the cell's group, the rest in any window"""
    rng = np.random.default_rng(seed)
    n = N_GROUPS * PER_GROUP
    group = np.arange(n) % N_GROUPS                          # interleaved: the table's order says nothing
    barcodes = [b"ACGT%04dTTGA-1" % k for k in range(n)]
    own = N_WINDOWS // N_GROUPS
    rows = []
    for c in range(n):
        depth = int(rng.integers(60, 141))
        inside = rng.random(depth) < 0.8
        w = np.where(inside, group[c] * own + rng.integers(0, own, depth), rng.integers(0, N_WINDOWS, depth))
        start = w * SLOT + 700 + rng.integers(0, WIDTH - 100, depth)
        length = rng.integers(40, 200, depth)
        rows += [(int(x) // (SLOT * N_WINDOWS // 2), int(x) % (SLOT * N_WINDOWS // 2), int(l), c) for x, l in zip(start, length)]
    rows.sort()
    text = b"".join(b"chr%d\t%d\t%d\t%s\t1\n" % (k + 1, s, s + l, barcodes[c]) for k, s, l, c in rows)
    half = N_WINDOWS // 2
    bed = b"".join(b"chr%d\t%d\t%d\n" % (w // half + 1, (w % half) * SLOT + 700, (w % half) * SLOT + 700 + WIDTH) for w in range(N_WINDOWS))
    return text, barcodes, group, bed


def test_cellcounts_cluster_split(tmp_path, monkeypatch, capsys):
    from nucleoatac_amd.pyatac.cli import main
    monkeypatch.chdir(tmp_path)
    text, barcodes, group, bed = synthetic_cells()
    assert 3000 < text.count(b"\n") < 9000
    open("cells.tsv.gz", "wb").write(bgzf_bytes(text, blk=4000))
    open("windows.bed", "wb").write(bed)
    open("cells.txt", "wb").write(b"".join(b + b"\n" for b in barcodes))
    base = ["cellcounts", "--fragments", "cells.tsv.gz", "--bed", "windows.bed", "--cells", "cells.txt"]
    assert main(base + ["--format", "npz", "--out", "a"]) == 0 and main(base + ["--out", "b"]) == 0
    cl = ["--clusters", "3", "--components", "5", "--oversample", "5"]
    assert main(["cluster", "--counts", "a.cellcounts.npz"] + cl) == 0
    assert main(["cluster", "--counts", "b.cellcounts.mtx.gz"] + cl) == 0
    for x in (".clusters.tsv", ".lsi.npz", ".cluster.txt"):
        assert open("a" + x, "rb").read() == open("b" + x, "rb").read(), x
    # the labels are the planted groups up to naming
    rows = [line.split(b"\t") for line in open("a.clusters.tsv", "rb").read().splitlines()]
    assert [r[0] for r in rows] == barcodes
    table = np.zeros((N_GROUPS, N_GROUPS), np.int64)
    for g, r in zip(group, rows):
        table[g, int(r[1][1:]) - 1] += 1
    assert np.array_equal(np.sort(table.ravel())[-N_GROUPS:], [PER_GROUP] * N_GROUPS) and (table > 0).sum() == N_GROUPS
    summary = dict(x.split("\t") for x in open("a.cluster.txt").read().splitlines())
    assert (summary["cells_kept"], summary["cells_dropped"], summary["r"], summary["c1"], summary["c2"], summary["c3"]) == \
        ("60", "0", "10", "20", "20", "20")
    # the table goes into `split` unchanged: one store per cluster
    assert main(["split", "--fragments", "cells.tsv.gz", "--groups", "a.clusters.tsv", "--out", "s"]) == 0
    assert sorted(f for f in os.listdir(".") if f.startswith("s.")) == ["s.c1.npz", "s.c2.npz", "s.c3.npz", "s.split.txt"]
    lines = [x.split("\t") for x in open("s.split.txt").read().splitlines()]
    assert lines[0][0] == "group" and sorted(x[0] for x in lines[1:4]) == ["c1", "c2", "c3"]      # in order of first appearance in the table
    assert all(x[1] == "20" and x[2] == "20" for x in lines[1:4]) and lines[4] == ["unassigned", "0"]
    assert sum(int(x[3]) for x in lines[1:4]) == text.count(b"\n")
    per_cluster = {x[0]: int(x[3]) for x in lines[1:4]}
    cell_lines = np.bincount([barcodes.index(f.split(b"\t")[3]) for f in text.splitlines()], minlength=len(barcodes))
    for g in range(N_GROUPS):
        name = "c%d" % (int(np.argmax(table[g])) + 1)
        assert per_cluster[name] == int(cell_lines[group == g].sum())
    capsys.readouterr()
