"""`pyatac markers`: the windows that distinguish every cell group from the rest, by a Wilcoxon rank-sum test of depth-normalised
accessibility, one group against all other kept cells, for every window and every group -- from the cell-by-window count matrix of
`pyatac cellcounts` and the table `pyatac cluster` writes.  This command is this package's own, like `cluster` and `deviations`: the
reference has no such tool.  It answers, after clustering, which windows are more open in cluster c3 than elsewhere (the test ArchR's
getMarkerFeatures and Seurat's FindAllMarkers made usual), with fixed rules so that the result is a function of the inputs.

Cells and groups.  X is the windows x cells count matrix (get_cluster.read_counts).  A cell is kept when the group table lists its
barcode and its column sum is positive; unlisted cells are in no group and not in "the rest" either.  N cells stay, 2 <= N <= 2^20.
d[c] is the kept cell's column sum over all windows, 1 <= d[c] < 2^31; grp[c] is in [0, G), at most 255 groups in order of first
appearance, and n_g is the group's number of kept cells.  A group with n_g = 0 or n_g = N gets NA everywhere.

Values and ranks.  Window p has L entries (c, a) among the kept cells and z0 = N - L cells at value 0.  The value of an entry is the exact
rational a / d[c]; order and ties are decided by comparing a_i * d_j with a_j * d_i in 64-bit integers (both factors are below 2^31, so
no product overflows).  Midranks, with less_i / eq_i counted among the window's entries and eq_i including i itself: a zero cell has
2 * rank = z0 + 1, an entry has 2 * rank_i = 2 z0 + 2 less_i + eq_i + 1.

Device (Context.group_rank_sums, csrc/natac_markers.hpp; include/natac.h states it), exact integers: detected[p, g] int32, the entries of
group g; total[p, g] int64, the sum of their counts; rank2[p, g] int64 = (n_g - detected)(z0 + 1) + the sum over the group's entries of
2 rank_i; ties[p] int64 = (z0^3 - z0) + the sum over the entries of (eq_i^2 - 1), which is the sum over tie groups of (t^3 - t) without a
sort.  An empty row is legal: rank2 = n_g (N + 1), ties = N^3 - N.  That is the hot path: a ranking of every row of X.

Host, fp64, one window and group at a time, with n_r = N - n_g:  U = rank2 / 2 - n_g (n_g + 1) / 2,  mu = n_g n_r / 2,
var = n_g n_r / 12 * ((N + 1) - ties / (N (N - 1))),  z = (U - mu - 0.5 sign(U - mu)) / sqrt(var), NaN where var == 0,
p = min(1, 2 * norm.sf(|z|)) (scipy's asymptotic two-sided test with tie and continuity correction),  auc = U / (n_g n_r),
pct_in = detected / n_g,  pct_rest = (row detected - detected) / n_r,
log2fc = log2(((total + 1) / D_g) / ((row total - total + 1) / D_r)) with D_g the sum of d over the group's cells and D_r the sum over the
rest: a pseudo-bulk ratio, integers in, no order-dependent float sum.

A window is tested when at least --min_cells kept cells have an entry; untested windows are NA and do not enter the correction.  q is
Benjamini-Hochberg per group over that group's tested windows with finite p; ties in p keep index order, and there is a running minimum
from the largest down.  A marker of g has q <= --fdr, log2fc >= --min_log2fc and auc > 0.5.

Not done here: bias-matched background cells as ArchR picks them, a logistic-regression or negative-binomial test, pairwise group
contrasts, a test of motif deviations.

Files.  BASE.markers.npz (fixed timestamps: both forms of the matrix give the same bytes): groups, n_cells, region_chrom / _start /
_end, tested, the [windows x groups] arrays detected, total, rank2, z, p, q, log2fc, auc, and ties.  BASE.markers.tsv: the markers only,
`group chrom start end log2fc auc pct_in pct_rest z p q`, ratios %.4f, p and q %.3e, per group by q, then auc descending, then window
index.  BASE.markers.<group>.bed, one per group: that group's markers in that order, cut at --top when given, `chrom start end name
score` with name <group>_marker_<i> and score min(1000, int(-10 log10 q)) -- `motifs --bed`, `counts --bed`, `cellcounts --bed` and
`run --bed` take it unchanged; a group without markers gets an empty file.  BASE.markers.txt: cells listed / kept / dropped, windows,
tested windows, and per group its cells, tested windows and markers.  When the --counts .npz holds region_name (`pyatac genescores` writes
it: the rows are genes) that array is written into BASE.markers.npz and the table gets a last column `name`; every other input gives the
files as they always were.

Measured on the MI355X box (tools/bench_markers.py, one box, one process, three runs after a warm-up: 10,000 cells x 100,000 windows,
8.07 M entries, 1,000 of the windows open in every second cell): the device call 7.5 to 36 ms with 8 groups and 45 to 69 ms with 64 (the
host's checks and row lists, the uploads and up to 128 MB of results included; 0.76 ms in the kernels); the exact restatement of
tests/markers_ref.py on 2,020 of those rows (251,531 entries) 1.30 s on that box, the four arrays equal.
"""
import os

import numpy as np

from .get_cluster import ClusterError, _savez_fixed, default_base, read_counts

MAX_CELLS = 1 << 20         # NATAC_MARKERS_MAX_CELLS


class MarkersError(ValueError):
    """an input or a parameter `pyatac markers` cannot use; one line"""


def check_params(min_cells, fdr, min_log2fc, top):
    if min_cells < 1:
        raise MarkersError("--min_cells must be at least 1 (got %d)" % min_cells)
    if not 0.0 < fdr <= 1.0:
        raise MarkersError("--fdr must be in (0, 1] (got %r)" % (fdr,))
    if not np.isfinite(min_log2fc):
        raise MarkersError("--min_log2fc must be finite (got %r)" % (min_log2fc,))
    if top is not None and top < 1:
        raise MarkersError("--top must be at least 1 (got %d)" % top)


def _device_rank_sums(*args, **kw):
    from .. import get_context
    return get_context().group_rank_sums(*args, **kw)


def statistics(detected, total, rank2, ties, depth, group, n_groups, min_cells):
    """the host part on the device's integers -> dict of tested bool[m], n_in_group int64[G] and float64[m, G] z, p, auc, pct_in, pct_rest,
    log2fc: NaN where the window is untested or the group has no cell or every cell.  Every element goes through the operations of the
    module docstring in that order."""
    from scipy.special import ndtr
    m, G, N = detected.shape[0], int(n_groups), len(depth)
    group = np.asarray(group, np.int64)
    n_g = np.bincount(group, minlength=G).astype(np.int64)
    D_g = np.zeros(G, np.int64)
    np.add.at(D_g, group, np.asarray(depth, np.int64))
    n_r, D_r = N - n_g, int(np.sum(np.asarray(depth, np.int64))) - D_g
    row_det, row_tot = detected.sum(axis=1, dtype=np.int64), total.sum(axis=1, dtype=np.int64)
    tested = row_det >= min_cells
    live = (n_g > 0) & (n_r > 0)
    ng, nr = n_g.astype(np.float64)[None, :], n_r.astype(np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        U = rank2.astype(np.float64) / 2.0 - ng * (ng + 1.0) / 2.0
        mu = ng * nr / 2.0
        var = ng * nr / 12.0 * ((N + 1.0) - ties.astype(np.float64)[:, None] / (N * (N - 1.0)))
        z = np.where(var == 0, np.nan, (U - mu - 0.5 * np.sign(U - mu)) / np.sqrt(var))
        p = np.minimum(1.0, 2.0 * ndtr(-np.abs(z)))
        auc = U / (ng * nr)
        pct_in = detected.astype(np.float64) / ng
        pct_rest = (row_det[:, None] - detected).astype(np.float64) / nr
        log2fc = np.log2(((total + 1).astype(np.float64) / D_g.astype(np.float64)[None, :]) /
                         ((row_tot[:, None] - total + 1).astype(np.float64) / D_r.astype(np.float64)[None, :]))
    out = dict(z=z, p=p, auc=auc, pct_in=pct_in, pct_rest=pct_rest, log2fc=log2fc)
    na = ~(tested[:, None] & live[None, :])
    for k in out:
        out[k] = np.where(na, np.nan, out[k])
    out["tested"], out["n_in_group"] = tested, n_g
    return out


def benjamini_hochberg(p):
    """q of the finite values of p (the others NaN): ranks by (p, index), q = p n / rank, a running minimum from the largest rank down"""
    p = np.asarray(p, np.float64)
    q = np.full(p.shape, np.nan)
    idx = np.flatnonzero(np.isfinite(p))
    if len(idx):
        order = idx[np.lexsort((idx, p[idx]))]
        n = len(order)
        raw = p[order] * float(n) / np.arange(1, n + 1, dtype=np.float64)
        q[order] = np.minimum.accumulate(raw[::-1])[::-1]
    return q


def rank_sum_markers(indptr, indices, data, barcodes, groups, min_cells=10, fdr=0.05, min_log2fc=0.5, rank=None):
    """the computation of `pyatac markers` on CSR arrays -> dict.  groups: a cellgroups.CellGroups.  rank(indptr, indices, data, n_cells,
    depth, group, n_groups) -> (detected, total, rank2, ties) defaults to Context.group_rank_sums."""
    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(data, np.int64)
    n_win, n_all, G = len(indptr) - 1, len(barcodes), len(groups.names)
    d_all = np.zeros(n_all, np.int64)
    np.add.at(d_all, indices, data)
    group_all = np.full(n_all, -1, np.int64)
    where = {bc: k for k, bc in enumerate(barcodes)}
    for bc, g in zip(groups.barcodes, groups.group_of):
        if bc in where:
            group_all[where[bc]] = g
    cell_keep = (group_all >= 0) & (d_all > 0)
    cells = np.flatnonzero(cell_keep)
    N = len(cells)
    depth, group = d_all[cells], group_all[cells]
    if N < 2 or len(np.unique(group)) < 2:
        raise MarkersError("fewer than two groups have a cell with a count: %d cells of the table are in the matrix with one" % N)
    if N > MAX_CELLS:
        raise MarkersError("%d cells are kept, more than %d" % (N, MAX_CELLS))
    if depth.max() >= 1 << 31:
        raise MarkersError("cell %s has %d counts, 2^31 or more" % (barcodes[cells[int(np.argmax(depth))]].decode("latin-1"), depth.max()))
    # the kept cells' matrix: zero entries and dropped cells go, the cells are renumbered; empty rows stay
    row_of = np.repeat(np.arange(n_win, dtype=np.int64), np.diff(indptr))
    keep = (data > 0) & cell_keep[indices]
    ptr = np.zeros(n_win + 1, np.int64)
    np.cumsum(np.bincount(row_of[keep], minlength=n_win), out=ptr[1:])
    new_cell = np.cumsum(cell_keep) - 1
    detected, total, rank2, ties = (rank or _device_rank_sums)(ptr, new_cell[indices[keep]].astype(np.int32), data[keep].astype(np.int32), N,
                                                               depth, group.astype(np.int32), G)
    st = statistics(detected, total, rank2, ties, depth, group, G, min_cells)
    q = np.full((n_win, G), np.nan)
    for g in range(G):
        q[:, g] = benjamini_hochberg(st["p"][:, g])
    with np.errstate(invalid="ignore"):
        is_marker = (q <= fdr) & (st["log2fc"] >= min_log2fc) & (st["auc"] > 0.5)
    markers = []
    for g in range(G):
        w = np.flatnonzero(is_marker[:, g])
        markers.append(w[np.lexsort((w, -st["auc"][w, g], q[w, g]))])
    st.update(cell_keep=cell_keep, N=N, detected=detected, total=total, rank2=rank2, ties=ties, q=q, markers=markers)
    return st


def output_texts(res, names, chrom, start, end, n_listed, n_all, top=None, region_name=None):
    """(markers.tsv, [one BED text per group], summary) as text.  region_name (one per window, or None): a last column `name` of the
    table"""
    named = region_name is not None
    rows = ["group\tchrom\tstart\tend\tlog2fc\tauc\tpct_in\tpct_rest\tz\tp\tq%s\n" % ("\tname" if named else "")]
    beds = []
    for g, name in enumerate(names):
        bed = []
        for i, w in enumerate(res["markers"][g].tolist(), 1):
            q = res["q"][w, g]
            rows.append("%s\t%s\t%d\t%d\t%.4f\t%.4f\t%.4f\t%.4f\t%.4f\t%.3e\t%.3e%s\n"
                        % (name, chrom[w], start[w], end[w], res["log2fc"][w, g], res["auc"][w, g], res["pct_in"][w, g], res["pct_rest"][w, g],
                           res["z"][w, g], res["p"][w, g], q, "\t%s" % region_name[w] if named else ""))
            if top is None or i <= top:
                score = 1000 if q <= 1e-100 else min(1000, int(-10.0 * np.log10(q)))
                bed.append("%s\t%d\t%d\t%s_marker_%d\t%d\n" % (chrom[w], start[w], end[w], name, i, score))
        beds.append("".join(bed))
    tested = res["tested"]
    summary = ("cells_listed\t%d\ncells_in_matrix\t%d\ncells_kept\t%d\ncells_dropped\t%d\nwindows\t%d\nwindows_tested\t%d\n"
               % (n_listed, n_all, res["N"], n_listed - res["N"], len(tested), int(tested.sum())))
    summary += "group\tcells\ttested\tmarkers\n"
    for g, name in enumerate(names):
        summary += "%s\t%d\t%d\t%d\n" % (name, res["n_in_group"][g], int(np.isfinite(res["p"][:, g]).sum()), len(res["markers"][g]))
    return "".join(rows), beds, summary


def read_region_names(path, n_rows):
    """the region_name array of a count matrix .npz (`pyatac genescores` writes one) as a list of str, or None where the file has none"""
    if not path.endswith(".npz"):
        return None
    with np.load(path, allow_pickle=False) as z:
        if "region_name" not in z.files:
            return None
        names = [n.decode("latin-1") if isinstance(n, bytes) else str(n) for n in z["region_name"].tolist()]
    if len(names) != n_rows:
        raise MarkersError("%s: %d region names for %d rows" % (path, len(names), n_rows))
    return names


def get_markers(args, rank=None):
    """`pyatac markers`: writes BASE.markers.npz, .tsv, .txt and one BASE.markers.<group>.bed per group; returns their paths.  Everything
    is computed before the first file is written, so an error leaves nothing behind.  rank: the device call (rank_sum_markers), for the
    tests."""
    from .cellgroups import read_groups
    from .get_deviations import DeviationsError, read_regions
    check_params(args.min_cells, args.fdr, args.min_log2fc, args.top)
    for path in (args.counts, args.groups):
        if not os.path.exists(path):
            raise MarkersError("%s: no such file" % path)
    try:
        indptr, indices, data, barcodes = read_counts(args.counts)
        chrom, start, end = read_regions(args.counts)
    except (ClusterError, DeviationsError) as e:
        raise MarkersError(str(e))
    if len(start) != len(indptr) - 1:
        raise MarkersError("%s: %d regions for %d rows" % (args.counts, len(start), len(indptr) - 1))
    region_name = read_region_names(args.counts, len(start))
    groups = read_groups(args.groups, header=args.header)
    res = rank_sum_markers(indptr, indices, data, barcodes, groups, args.min_cells, args.fdr, args.min_log2fc, rank=rank)
    table, beds, summary = output_texts(res, groups.names, chrom, start, end, len(groups.barcodes), len(barcodes), args.top, region_name=region_name)
    extra = {} if region_name is None else dict(region_name=np.array(region_name, dtype="U"))
    base = (args.out if args.out else default_base(args.counts)) + ".markers"
    paths = [base + ".npz", base + ".tsv", base + ".txt"] + [base + ".%s.bed" % name for name in groups.names]
    _savez_fixed(paths[0], groups=np.array([n.encode("latin-1") for n in groups.names], dtype="S"), n_cells=res["n_in_group"],
                 region_chrom=np.array(chrom), region_start=start, region_end=end, tested=res["tested"], detected=res["detected"],
                 total=res["total"], rank2=res["rank2"], z=res["z"], p=res["p"], q=res["q"], log2fc=res["log2fc"], auc=res["auc"],
                 ties=res["ties"], **extra)
    for path, text in zip(paths[1:], [table, summary] + beds):
        with open(path, "w") as f:
            f.write(text)
    return paths
