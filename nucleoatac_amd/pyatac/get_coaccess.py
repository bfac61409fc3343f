"""`pyatac coaccess`: the windows that open and close together -- the Pearson correlation over the cells of every two windows of one
chromosome that lie within a genomic distance of each other, with a t-test, Benjamini-Hochberg q-values and a BEDPE file of links -- from
the cell-by-window count matrix of `pyatac cellcounts` and, for metacells, the table `pyatac cluster` writes.  This command is this
package's own, like `cluster`, `deviations` and `markers`: the reference has no such tool.  It answers which distal window goes with
which promoter (Cicero's co-accessibility, ArchR's getCoAccessibility), with fixed rules so that the result is a function of the inputs.

Cells.  X is the windows x cells count matrix (get_cluster.read_counts).  A cell is kept when its column sum is positive.  With
--aggregate TABLE [--header] the columns are first summed per group on the host (TABLE is read by cellgroups.read_groups, so it holds at
most 255 groups): the "cells" are then the groups that have a count, and unlisted barcodes are dropped.  This is the metacell form; a
user makes metacells with `cluster --clusters 200`.  With --binarize every entry counts as 1, before the aggregation.  N cells stay,
3 <= N <= 2^20.

Windows.  Window p has entries a[p, c] >= 1 and det[p] = their number, S1[p] = sum a, S2[p] = sum a^2, all int64.  A window is tested when
det[p] >= --min_cells; its centre is (start + end) // 2.

Pairs.  Per chromosome the tested windows are ranked by (centre, index).  A pair is two tested windows of one chromosome whose centres
differ by at most --max_distance (in [0, 10^8]); it is listed once, under the member that ranks first (its owner), in rank order of the
partner; the chromosomes go in order of first appearance in the region list.

Device (Context.window_pair_sums, csrc/natac_coaccess.hpp; include/natac.h states it), exact integers per pair (p, q): sxy int64 = the sum
over the cells of a[p, c] * a[q, c]; both int32 = the number of cells with an entry in both.  That is the hot path: a sparse-sparse
intersection for every pair.  With a_max the largest count and L_max the longest tested row the call needs N * a_max^2 * L_max < 2^62;
then every sxy, N * sxy, S1[p] * S1[q] and N * S2 - S1^2 fit in int64.  The command refuses a matrix past the bound and says to use
--binarize.

Host, fp64, one pair at a time:  num = N * sxy - S1[p] * S1[q] and D[p] = N * S2[p] - S1[p]^2 in int64;
r = float(num) / sqrt(float(D[p]) * float(D[q])), clipped to [-1, 1], NaN where a D is 0;  t = r * sqrt((N - 2) / ((1 - r) * (1 + r)));
p = 2 * scipy.stats.t.sf(|t|, N - 2), and 0 where |r| == 1;  q is Benjamini-Hochberg over all pairs with a finite p
(get_markers.benjamini_hochberg).  A link has r >= --min_cor (in [-1, 1]) and q <= --fdr (in (0, 1]).

Not done here: kNN metacells picked by the command itself, a depth or GC covariate, graphical-lasso regularisation as in Cicero, a
cross-chromosome background, a peak-to-gene step (`genescores` has the genes, but the package has no expression input).

Files.  BASE.coaccess.npz (fixed timestamps: both forms of the matrix give the same bytes): region_chrom / _start / _end, tested, detected,
s1, s2, n_cells, pair_a and pair_b (window indices in file order, the owner first), sxy, both, r, p, q.  BASE.coaccess.bedpe: the links
only, `chrom start1 end1 chrom start2 end2 name score . . r both p q` with name <BASE's file name>_link_<i>, score
min(1000, int(1000 * r)), r as %.4f, p and q as %.3e, the member with the smaller start first, sorted by q, then r descending, then pair
index.  BASE.coaccess.txt: cells listed / kept / dropped, windows and tested windows, pairs, pairs with a finite r, links, N, a_max,
L_max and the arm the device took.  No pair at all is not an error: the files are empty and the summary says 0.

Measured on the MI355X box (tools/bench_coaccess.py, one box, one process, three runs after a warm-up: 10,000 cells x 100,000 windows,
8.07 M entries, 4 chromosomes at 2 kb spacing, 12,468,500 pairs within 250 kb): the device call 64 to 79 ms (the host's checks, the
uploads and 150 MB of results included; 4.7 ms in the table arm's kernel, 15.3 ms in the search arm's on the same matrix); the
scipy.sparse restatement of tests/coaccess_ref.py on the first 2,000 owners (250,000 pairs) 3.44 s on that box, both arrays equal.
"""
import os

import numpy as np

from .get_cluster import ClusterError, _savez_fixed, default_base, read_counts
from .get_markers import benjamini_hochberg

MAX_CELLS = 1 << 20         # NATAC_COACCESS_MAX_CELLS
MAX_DISTANCE = 10 ** 8


class CoaccessError(ValueError):
    """an input or a parameter `pyatac coaccess` cannot use; one line"""


def check_params(min_cells, max_distance, min_cor, fdr):
    if min_cells < 1:
        raise CoaccessError("--min_cells must be at least 1 (got %d)" % min_cells)
    if not 0 <= max_distance <= MAX_DISTANCE:
        raise CoaccessError("--max_distance must be in [0, %d] (got %d)" % (MAX_DISTANCE, max_distance))
    if not -1.0 <= min_cor <= 1.0:
        raise CoaccessError("--min_cor must be in [-1, 1] (got %r)" % (min_cor,))
    if not 0.0 < fdr <= 1.0:
        raise CoaccessError("--fdr must be in (0, 1] (got %r)" % (fdr,))


def _device_pair_sums(*args, **kw):
    from .. import get_context
    return get_context().window_pair_sums(*args, **kw)


def pair_lists(chrom, start, end, tested, max_distance):
    """(order int32[k], hi int64[k]) as Context.window_pair_sums takes them: the tested windows per chromosome (in order of first
    appearance) ranked by (centre, index); owner i is paired with order[i + 1 .. hi[i]), the later windows of its chromosome whose
    centre is at most max_distance past its own"""
    start, end = np.asarray(start, np.int64), np.asarray(end, np.int64)
    tested = np.asarray(tested, bool)
    names, first, code = np.unique(np.asarray(chrom, dtype="U"), return_index=True, return_inverse=True)
    by_first = np.empty(len(names), np.int64)
    by_first[np.argsort(first, kind="stable")] = np.arange(len(names))
    code = by_first[code]                                  # the chromosomes numbered in order of first appearance
    idx = np.flatnonzero(tested)
    centre = (start + end) // 2
    order = idx[np.lexsort((idx, centre[idx], code[idx]))]
    hi = np.zeros(len(order), np.int64)
    edges = np.flatnonzero(np.diff(code[order])) + 1
    for a, b in zip(np.concatenate([[0], edges]).tolist(), np.concatenate([edges, [len(order)]]).tolist()):
        c = centre[order[a:b]]
        hi[a:b] = a + np.searchsorted(c, c + int(max_distance), side="right")
    return order.astype(np.int32), hi


def cell_matrix(indptr, indices, data, barcodes, groups=None, binarize=False):
    """the matrix of the kept cells -> (indptr int64, indices int32, data int64, N, n_listed): zero entries go; with binarize every entry
    becomes 1; with groups (a cellgroups.CellGroups) the columns are summed per group and unlisted barcodes are dropped; then the
    columns without a count go and the rest are renumbered in their order.  n_listed: the columns before that last step."""
    import scipy.sparse as sp
    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(data, np.int64)
    n_win = len(indptr) - 1
    row = np.repeat(np.arange(n_win, dtype=np.int64), np.diff(indptr))
    keep = data > 0
    col, n_col = indices, len(barcodes)
    if groups is not None:
        where = {bc: k for k, bc in enumerate(barcodes)}
        group_of = np.full(len(barcodes), -1, np.int64)
        for bc, g in zip(groups.barcodes, groups.group_of):
            if bc in where:
                group_of[where[bc]] = g
        col, n_col = group_of[indices], len(groups.names)
        keep &= col >= 0
    val = np.ones(int(keep.sum()), np.int64) if binarize else data[keep]
    X = sp.coo_matrix((val, (row[keep], col[keep])), shape=(n_win, n_col)).tocsr()      # duplicates summed, in int64
    X.sort_indices()
    has = np.bincount(X.indices, minlength=n_col) > 0
    new = np.cumsum(has) - 1
    return X.indptr.astype(np.int64), new[X.indices].astype(np.int32), X.data.astype(np.int64), int(has.sum()), n_col


def correlations(sxy, pair_a, pair_b, s1, s2, N):
    """(r, p) float64 per pair from the exact integers, every element through the operations of the module docstring in that order"""
    from scipy.stats import t as student
    num = N * np.asarray(sxy, np.int64) - s1[pair_a] * s1[pair_b]
    D = N * s2 - s1 * s1
    Da, Db = D[pair_a], D[pair_b]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = num.astype(np.float64) / np.sqrt(Da.astype(np.float64) * Db.astype(np.float64))
        r = np.where((Da == 0) | (Db == 0), np.nan, np.clip(r, -1.0, 1.0))
        t = r * np.sqrt((N - 2.0) / ((1.0 - r) * (1.0 + r)))
        p = 2.0 * student.sf(np.abs(t), N - 2)
    p = np.where(np.abs(r) == 1.0, 0.0, p)
    return r, np.where(np.isnan(r), np.nan, p)


def coaccess(indptr, indices, data, n_cells, chrom, start, end, min_cells=10, max_distance=250000, min_cor=0.5, fdr=0.05, pairs=None):
    """the computation of `pyatac coaccess` on the kept cells' CSR arrays (cell_matrix) -> dict.  pairs(indptr, indices, data, n_cells,
    order, hi) -> (sxy, both) defaults to Context.window_pair_sums."""
    check_params(min_cells, max_distance, min_cor, fdr)
    indptr, data, N = np.asarray(indptr, np.int64), np.asarray(data, np.int64), int(n_cells)
    if N < 3:
        raise CoaccessError("fewer than 3 cells have a count (%d): a correlation needs three" % N)
    if N > MAX_CELLS:
        raise CoaccessError("%d cells are kept, more than %d" % (N, MAX_CELLS))
    n_win = len(indptr) - 1
    row = np.repeat(np.arange(n_win, dtype=np.int64), np.diff(indptr))
    detected = np.diff(indptr)
    s1, s2 = np.zeros(n_win, np.int64), np.zeros(n_win, np.int64)
    np.add.at(s1, row, data)
    a_max = int(data.max()) if len(data) else 0
    if a_max >= 1 << 31:
        raise CoaccessError("a count of %d, 2^31 or more: use --binarize" % a_max)
    np.add.at(s2, row, data * data)
    tested = detected >= min_cells
    if not tested.any():
        raise CoaccessError("no window has an entry in %d cells or more (--min_cells)" % min_cells)
    l_max = int(detected[tested].max())
    if N * a_max * a_max * l_max >= 1 << 62:
        raise CoaccessError("N * a_max^2 * L_max = %d * %d^2 * %d is 2^62 or more, the sums would leave 64 bits: use --binarize" % (N, a_max, l_max))
    order, hi = pair_lists(chrom, start, end, tested, max_distance)
    k = len(order)
    n_part = hi - np.arange(k, dtype=np.int64) - 1
    pair_a = np.repeat(order.astype(np.int64), n_part)
    ptr = np.zeros(k + 1, np.int64)
    np.cumsum(n_part, out=ptr[1:])
    # partner e of owner i is order[i + 1 + e]
    pair_b = order.astype(np.int64)[np.arange(int(ptr[-1]), dtype=np.int64) - np.repeat(ptr[:-1], n_part) + np.repeat(np.arange(k, dtype=np.int64), n_part) + 1]
    sxy, both = (pairs or _device_pair_sums)(indptr, np.asarray(indices, np.int32), data.astype(np.int32), N, order, hi)
    sxy, both = np.asarray(sxy, np.int64), np.asarray(both, np.int32)
    r, p = correlations(sxy, pair_a, pair_b, s1, s2, N)
    q = benjamini_hochberg(p)
    with np.errstate(invalid="ignore"):
        w = np.flatnonzero((r >= min_cor) & (q <= fdr))
    links = w[np.lexsort((w, -r[w], q[w]))]
    arm = "none"
    if len(pair_a):
        from ..device import window_pair_sums_plan
        arm = window_pair_sums_plan(n_win, N, len(data), k, int(detected[order].sum()))["arm"]
    return dict(N=N, a_max=a_max, l_max=l_max, tested=tested, detected=detected.astype(np.int64), s1=s1, s2=s2, pair_a=pair_a, pair_b=pair_b,
                sxy=sxy, both=both, r=r, p=p, q=q, links=links, arm=arm)


def output_texts(res, chrom, start, end, name, n_listed):
    """(coaccess.bedpe, summary) as text; name: the links are <name>_link_<i>"""
    rows = []
    for i, e in enumerate(res["links"].tolist(), 1):
        a, b = int(res["pair_a"][e]), int(res["pair_b"][e])
        if start[b] < start[a]:
            a, b = b, a
        r = res["r"][e]
        rows.append("%s\t%d\t%d\t%s\t%d\t%d\t%s_link_%d\t%d\t.\t.\t%.4f\t%d\t%.3e\t%.3e\n"
                    % (chrom[a], start[a], end[a], chrom[b], start[b], end[b], name, i, min(1000, int(1000 * r)), r, res["both"][e],
                       res["p"][e], res["q"][e]))
    tested = res["tested"]
    summary = ("cells_listed\t%d\ncells_kept\t%d\ncells_dropped\t%d\nwindows\t%d\nwindows_tested\t%d\npairs\t%d\npairs_finite\t%d\nlinks\t%d\n"
               "N\t%d\na_max\t%d\nL_max\t%d\narm\t%s\n"
               % (n_listed, res["N"], n_listed - res["N"], len(tested), int(tested.sum()), len(res["pair_a"]), int(np.isfinite(res["r"]).sum()),
                  len(res["links"]), res["N"], res["a_max"], res["l_max"], res["arm"]))
    return "".join(rows), summary


def get_coaccess(args, pairs=None):
    """`pyatac coaccess`: writes BASE.coaccess.npz, .bedpe and .txt; returns their paths.  Everything is computed before the first file
    is written, so an error leaves nothing behind.  pairs: the device call (coaccess), for the tests."""
    from .cellgroups import read_groups
    from .get_deviations import DeviationsError, read_regions
    check_params(args.min_cells, args.max_distance, args.min_cor, args.fdr)
    for path in (args.counts,) + ((args.aggregate,) if args.aggregate else ()):
        if not os.path.exists(path):
            raise CoaccessError("%s: no such file" % path)
    try:
        indptr, indices, data, barcodes = read_counts(args.counts)
        chrom, start, end = read_regions(args.counts)
    except (ClusterError, DeviationsError) as e:
        raise CoaccessError(str(e))
    if len(start) != len(indptr) - 1:
        raise CoaccessError("%s: %d regions for %d rows" % (args.counts, len(start), len(indptr) - 1))
    groups = read_groups(args.aggregate, header=args.header) if args.aggregate else None
    ptr, col, cnt, N, n_listed = cell_matrix(indptr, indices, data, barcodes, groups, args.binarize)
    res = coaccess(ptr, col, cnt, N, chrom, start, end, args.min_cells, args.max_distance, args.min_cor, args.fdr, pairs=pairs)
    base = (args.out if args.out else default_base(args.counts)) + ".coaccess"
    bedpe, summary = output_texts(res, chrom, start, end, os.path.basename(base[:-len(".coaccess")]), n_listed)
    paths = [base + ".npz", base + ".bedpe", base + ".txt"]
    _savez_fixed(paths[0], region_chrom=np.array(chrom), region_start=start, region_end=end, tested=res["tested"], detected=res["detected"],
                 s1=res["s1"], s2=res["s2"], n_cells=np.int64(res["N"]), pair_a=res["pair_a"], pair_b=res["pair_b"], sxy=res["sxy"],
                 both=res["both"], r=res["r"], p=res["p"], q=res["q"])
    for path, text in zip(paths[1:], [bedpe, summary]):
        with open(path, "w") as f:
            f.write(text)
    return paths
