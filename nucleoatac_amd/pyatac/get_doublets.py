"""`pyatac doublets`: a doublet score per cell of the cell-by-window count matrix that `pyatac cellcounts` wrote, and the table of the
cells that are kept.  This command is this package's own, like `cluster`: the reference has no such tool.  Its place in the chain is
`cellcounts` -> `doublets` -> `cellcounts --cells BASE.doublets.cells.tsv` -> `cluster`.

The method is the usual one (Scrublet, ArchR's addDoubletScores / filterDoublets) with fixed rules; include/natac.h states them in full.

Space.  Everything up to V is `cluster`'s, with the same flags and the same checks: tfidf_weights, r = --components + --oversample <= 64,
the same Context.sparse_lsi call.  g = numpy.random.default_rng(seed) and q0 = g.standard_normal((windows, r)) is drawn first, so the LSI is
bit for bit `cluster`'s for that seed.  N cells are kept (total > 0); N >= 2.

Simulated doublets.  S = int(rint(--ratio * N)), ratio in (0, 8], S >= 1; a = g.integers(0, N, S) and b = g.integers(0, N, S), in that
order, index the kept cells (a[i] == b[i] is allowed).  Doublet i has the counts x[a] + x[b] and the total total[a] + total[b]; with
--binarize every window in the union counts 1.

Projection, on the host in fp64.  Every column, real and simulated alike, goes through one function: the weighted entry is
t = a' * (1 / total) * row_weight[w], or log1p(10000 t) with --method log, the row weights those of the real cells, and
E = A V[:, :components] is one scipy.sparse CSR-times-dense product with sorted indices.  The real cells are projected this way too, not
taken from U sigma (the two differ by how far the subspace iteration has converged).  depth_correlation of the real rows against their
totals decides the components kept, as in `cluster`, and P = unit_rows of the kept components has N + S rows, the real cells first.

Neighbours.  k = --neighbors in [1, 1024] if given, else max(1, int(rint(0.5 sqrt(N)))); k_adj = int(rint(k (1 + S / N))) clipped to
[1, min(1024, N + S - 1)].  For every real cell its k_adj nearest rows of P, itself excluded, come from Context.knn: the exact search on
the device (csrc/natac_knn.hpp), the hot path.

Score, on the host in fp64 in this order: n_syn = the neighbours with index >= N, q = (n_syn + 1) / (k_adj + 2), rr = S / N,
rho = --expected_rate in (0, 0.5], score = q * rho / rr / (1 - rho - q * (1 - rho - rho / rr)) -- Scrublet's likelihood.

Flag.  With --max_score X a cell is flagged when score > X.  Otherwise ArchR's rule with F = --filter_ratio in [0, 100] (default 1.0):
n_remove = min(N - 1, int(F * N * N / 100000)) and the first n_remove cells by (score descending, index ascending) are flagged.  The two
switches exclude each other.  No knee or histogram threshold is searched for.

Not done: approximate search, ArchR's down-sampling of the simulated counts, an automatic threshold, UMAP or graph clustering on the
graph, writing V into `cluster`'s BASE.lsi.npz.
"""
import numpy as np

from .get_cluster import SCALE, ClusterError, _device_svd, _savez_fixed, default_base, depth_correlation, read_counts, tfidf_weights, unit_rows

MAX_K = 1024        # NATAC_KNN_MAX_K
MAX_RATIO = 8.0


class DoubletsError(ClusterError):
    """an input or a parameter `pyatac doublets` cannot use; one line"""


def _device_knn(points, k, queries, self_offset):
    from .. import get_context
    return get_context().knn(points, k, queries=queries, self_offset=self_offset, with_arm_queries=True)


def neighbour_counts(n_kept, n_sim, neighbors=None):
    """(k, k_adj, capped) by the rule of the module docstring"""
    if neighbors is None:
        k = max(1, int(np.rint(0.5 * np.sqrt(n_kept))))
    else:
        k = int(neighbors)
        if not 1 <= k <= MAX_K:
            raise DoubletsError("--neighbors must be in [1, %d] (got %d)" % (MAX_K, k))
    want = int(np.rint(k * (1.0 + float(n_sim) / n_kept)))
    k_adj = max(1, min(want, MAX_K, n_kept + n_sim - 1))
    return k, k_adj, want > MAX_K


def likelihood(n_syn, k_adj, rr, rho):
    """Scrublet's likelihood of a doublet given n_syn simulated doublets among k_adj neighbours, fp64 in the rule's operation order"""
    q = (np.asarray(n_syn, np.float64) + 1.0) / (k_adj + 2.0)
    return q * rho / rr / (1.0 - rho - q * (1.0 - rho - rho / rr))


def flag_cells(score, filter_ratio=None, max_score=None):
    """(flagged bool[N], n_remove or None) by the rule of the module docstring"""
    n = len(score)
    if max_score is not None:
        return score > max_score, None
    f = 1.0 if filter_ratio is None else float(filter_ratio)
    n_remove = min(n - 1, int(f * n * n / 100000.0))
    order = np.lexsort((np.arange(n), -score))
    flagged = np.zeros(n, bool)
    flagged[order[:n_remove]] = True
    return flagged, n_remove


def project(counts, totals, row_weight, V, method):
    """E = A V for the columns of counts (scipy CSC, windows x columns, integer counts): the weighted entry of count a in window w and
    column c is t = a * (1 / totals[c]) * row_weight[w], or log1p(SCALE * t) with method "log"; A is cells x windows CSR with sorted
    indices and the product is scipy's"""
    M = counts.tocoo()
    t = M.data.astype(np.float64) * (1.0 / np.asarray(totals, np.float64))[M.col] * row_weight[M.row]
    v = np.log1p(t * SCALE) if method == "log" else t
    import scipy.sparse as sp
    A = sp.csr_matrix((v, (M.col, M.row)), shape=(counts.shape[1], counts.shape[0]))
    A.sort_indices()
    return A.dot(np.ascontiguousarray(V))


def doublet_scores(indptr, indices, data, n_cells, components=30, oversample=10, iterations=4, method="log", binarize=False, min_cells=1,
                   max_depth_cor=0.75, seed=1, ratio=2.0, neighbors=None, expected_rate=0.06, filter_ratio=None, max_score=None, svd=None,
                   knn=None):
    """the computation of `pyatac doublets` on CSR arrays -> dict(total, cell_keep, win_keep, depth_cor, components_kept, points, pair_a,
    pair_b, k, k_adj, capped, knn_index, knn_dist2, synthetic_neighbors, score, flagged, n_remove, arm, r).  svd: see
    get_cluster.cluster_cells.  knn(points, k, queries, self_offset) -> (idx, dist2[, arm_queries]) defaults to Context.knn."""
    import scipy.sparse as sp
    if components < 1 or oversample < 0 or components + oversample > 64:
        raise DoubletsError("--components must be at least 1, --oversample at least 0 and their sum at most 64 (got %d + %d)" % (components, oversample))
    if iterations < 1 or min_cells < 1:
        raise DoubletsError("--iterations and --min_cells must be at least 1")
    if method not in ("log", "linear"):
        raise DoubletsError("--method must be log or linear (got %s)" % method)
    if not 0.0 <= max_depth_cor <= 1.0:
        raise DoubletsError("--max_depth_cor must be in [0, 1] (got %g)" % max_depth_cor)
    if not 0.0 < ratio <= MAX_RATIO:
        raise DoubletsError("--ratio must be in (0, %g] (got %g)" % (MAX_RATIO, ratio))
    if not 0.0 < expected_rate <= 0.5:
        raise DoubletsError("--expected_rate must be in (0, 0.5] (got %g)" % expected_rate)
    if filter_ratio is not None and max_score is not None:
        raise DoubletsError("--filter_ratio and --max_score exclude each other")
    if filter_ratio is not None and not 0.0 <= filter_ratio <= 100.0:
        raise DoubletsError("--filter_ratio must be in [0, 100] (got %g)" % filter_ratio)
    if max_score is not None and not np.isfinite(max_score):
        raise DoubletsError("--max_score must be a finite number")
    if neighbors is not None and not 1 <= neighbors <= MAX_K:
        raise DoubletsError("--neighbors must be in [1, %d] (got %d)" % (MAX_K, neighbors))
    r = components + oversample
    total, row_weight, col_scale = tfidf_weights(indptr, indices, data, n_cells, binarize, min_cells)
    cell_keep, win_keep = col_scale > 0, row_weight > 0
    kept = np.flatnonzero(cell_keep)
    N = len(kept)
    if N < 2:
        raise DoubletsError("%d cells kept, fewer than 2" % N)
    if r > N or r > int(win_keep.sum()):
        raise DoubletsError("%d cells and %d windows kept, fewer than --components + --oversample = %d: lower --components"
                            % (N, int(win_keep.sum()), r))
    S = int(np.rint(ratio * N))
    if S < 1:
        raise DoubletsError("--ratio %g of %d cells simulates no doublet" % (ratio, N))
    n_windows = len(indptr) - 1
    g = np.random.default_rng(seed)
    q0 = g.standard_normal((n_windows, r))
    try:
        _, _, V = (svd or _device_svd)(indptr, indices, data, n_cells, row_weight, col_scale, r, iterations, q0, scale=SCALE, transform=method,
                                       binarize=binarize)
    except ValueError as e:
        if str(e) != "rank":
            raise
        raise DoubletsError("the weighted matrix has fewer than %d independent directions: lower --components" % r)
    pair_a = g.integers(0, N, S)
    pair_b = g.integers(0, N, S)
    a = np.ones(len(indices), np.int64) if binarize else np.asarray(data, np.int64)
    X = sp.csr_matrix((a, np.asarray(indices, np.int64), np.asarray(indptr, np.int64)), shape=(n_windows, n_cells)).tocsc()[:, kept]
    D = (X[:, pair_a] + X[:, pair_b]).tocsc()
    if binarize:
        D.data[:] = 1
    tot = total[kept]
    E = project(sp.hstack([X, D]).tocsc(), np.concatenate([tot, tot[pair_a] + tot[pair_b]]), row_weight, V[:, :components], method)
    depth_cor = depth_correlation(E[:N], tot)
    comp_keep = np.flatnonzero(~(np.abs(depth_cor) > max_depth_cor))
    if len(comp_keep) < 1:
        raise DoubletsError("every component tracks sequencing depth (|correlation| > %g): none is left" % max_depth_cor)
    P = np.ascontiguousarray(unit_rows(E[:, comp_keep]))
    k, k_adj, capped = neighbour_counts(N, S, neighbors)
    got = (knn or _device_knn)(P, k_adj, P[:N], 0)
    idx, d2 = np.asarray(got[0], np.int32), np.asarray(got[1], np.float64)
    arm = "host" if len(got) < 3 else ("wave" if got[2][0] else "lds")
    n_syn = (idx >= N).sum(axis=1).astype(np.int64)
    score = likelihood(n_syn, k_adj, float(S) / N, float(expected_rate))
    flagged, n_remove = flag_cells(score, filter_ratio, max_score)
    return dict(total=total, cell_keep=cell_keep, win_keep=win_keep, depth_cor=depth_cor, components_kept=comp_keep, points=P, pair_a=pair_a,
                pair_b=pair_b, k=k, k_adj=k_adj, capped=capped, knn_index=idx, knn_dist2=d2, synthetic_neighbors=n_syn, score=score,
                flagged=flagged, n_remove=n_remove, arm=arm, r=r)


def get_doublets(args, svd=None, knn=None):
    """`pyatac doublets`: writes BASE.doublets.tsv, BASE.doublets.cells.tsv, BASE.doublets.npz and BASE.doublets.txt and returns their
    paths.  Everything is computed before the first file is written, so an error leaves nothing behind.  svd, knn: see doublet_scores."""
    indptr, indices, data, barcodes = read_counts(args.counts)
    res = doublet_scores(indptr, indices, data, len(barcodes), args.components, args.oversample, args.iterations, args.method, args.binarize,
                         args.min_cells, args.max_depth_cor, args.seed, args.ratio, args.neighbors, args.expected_rate, args.filter_ratio,
                         args.max_score, svd=svd, knn=knn)
    base = args.out if args.out else default_base(args.counts)
    kept = np.flatnonzero(res["cell_keep"])
    N, S = len(kept), len(res["pair_a"])
    place = np.full(len(barcodes), -1, np.int64)
    place[kept] = np.arange(N)
    score, flagged, n_syn, total = res["score"], res["flagged"], res["synthetic_neighbors"], res["total"]
    rows = [b"#barcode\ttotal\tsynthetic_neighbors\tscore\tflagged\n"]
    for c, b in enumerate(barcodes):
        i = int(place[c])
        if i < 0:
            rows.append(b + b"\t%d\tNA\tNA\t0\n" % total[c])
        else:
            rows.append(b + b"\t%d\t%d\t%s\t%d\n" % (total[c], n_syn[i], ("%.4f" % score[i]).encode(), 1 if flagged[i] else 0))
    cells = b"".join(barcodes[c] + b"\n" for i, c in enumerate(kept.tolist()) if not flagged[i])
    removed = [j + 1 for j in range(args.components) if j not in set(res["components_kept"].tolist())]
    n_flag = int(flagged.sum())

    def _fmt(v):
        return "%.4f" % v if v is not None else "NA"

    summary = ("cells_listed\t%d\ncells_kept\t%d\ncells_dropped\t%d\nsimulated\t%d\nk\t%d\nk_adj\t%d\nk_adj_capped\t%s\ndimensions\t%d\n"
               "components_removed\t%s\nflagged\t%d\nsmallest_flagged_score\t%s\nlargest_unflagged_score\t%s\narm\t%s\n"
               % (len(barcodes), N, len(barcodes) - N, S, res["k"], res["k_adj"], "yes" if res["capped"] else "no", res["points"].shape[1],
                  ",".join("%d" % j for j in removed) if removed else "none", n_flag,
                  _fmt(float(score[flagged].min()) if n_flag else None), _fmt(float(score[~flagged].max()) if n_flag < N else None),
                  res["arm"]))
    params = np.array([("components", "%d" % args.components), ("oversample", "%d" % args.oversample), ("iterations", "%d" % args.iterations),
                       ("method", args.method), ("binarize", "%d" % (1 if args.binarize else 0)), ("min_cells", "%d" % args.min_cells),
                       ("max_depth_cor", repr(float(args.max_depth_cor))), ("seed", "%d" % args.seed), ("ratio", repr(float(args.ratio))),
                       ("neighbors", "default" if args.neighbors is None else "%d" % args.neighbors),
                       ("expected_rate", repr(float(args.expected_rate))),
                       ("filter_ratio", "none" if args.max_score is not None else repr(1.0 if args.filter_ratio is None else float(args.filter_ratio))),
                       ("max_score", "none" if args.max_score is None else repr(float(args.max_score)))], dtype="S")
    paths = [base + ".doublets.tsv", base + ".doublets.cells.tsv", base + ".doublets.npz", base + ".doublets.txt"]
    with open(paths[0], "wb") as f:
        f.write(b"".join(rows))
    with open(paths[1], "wb") as f:
        f.write(cells)
    _savez_fixed(paths[2], barcodes=np.array(barcodes, dtype="S"), kept=res["cell_keep"], components=res["components_kept"].astype(np.int64),
                 depth_cor=res["depth_cor"], points=res["points"], pair_a=res["pair_a"].astype(np.int64), pair_b=res["pair_b"].astype(np.int64),
                 knn_index=res["knn_index"], knn_dist2=res["knn_dist2"], synthetic_neighbors=n_syn, score=score, flagged=flagged, params=params)
    with open(paths[3], "w") as f:
        f.write(summary)
    return paths
