"""`pyatac cluster`: cluster the cells of the cell-by-window count matrix that `pyatac cellcounts` wrote.  This command is this package's
own, like `cellcounts`: the reference has no such tool.

It is the usual scATAC recipe with fixed rules -- TF-IDF weighting, latent semantic indexing (a truncated SVD of the weighted matrix),
removal of the components that track sequencing depth, k-means on what is left with the number of clusters given by the user -- and its
output is the `barcode<TAB>group` table `split --groups` takes unchanged.  No knee, no graph clustering, no UMAP, no search for K.

Weighting.  a' is the count, or 1 with --binarize.  total[c] is the column sum of a' and t_w the row sum.  Cells with total 0 are dropped
(counted in the summary, absent from the table), windows seen in fewer than --min_cells cells are dropped.  With N the number of cells
kept, the entry of window w and cell c is a' / total[c] * N / t_w -- term frequency times inverse document frequency -- and, with --method
log (the default), log1p of 10,000 times that.

LSI.  r = --components + --oversample singular triplets of the weighted matrix (cells x windows) come from Context.sparse_lsi: --iterations
rounds of subspace iteration from q0 = numpy.random.default_rng(seed).standard_normal((windows, r)), fp64 on the device
(csrc/natac_lsi.hpp).  That is the hot path: products of the sparse matrix with a block of r columns in both orientations.  The embedding
is E = U[:, :components] * sigma[:components]; component j is removed when |pearson(E[:, j], log10(total))| exceeds --max_depth_cor (the
first one usually is: it tracks depth, not biology), and every row of what is left is scaled to unit length (a zero row stays zero).

k-means runs in NumPy on the host, like everything else behind the SVD: it is O(cells x components) work per step -- 10^5 cells x 50
clusters x 50 dimensions per iteration is milliseconds of BLAS -- and has nothing for the device to win.  The rules are fixed so that the
result is a function of the input: the first centre is the row farthest from the mean row, each next centre the row farthest from its
nearest centre (ties go to the lowest index), Lloyd steps run until no label changes or --max_iter is reached, an emptied cluster keeps
its centre, and the clusters are named c1 .. cK by size descending, then by their lowest cell index.

Measured on the MI355X box (tools/bench_lsi.py, one box, one run: 10,000 cells x 100,000 windows, 3.08 M entries, r = 40, 4 rounds): the
device call 0.044 s (operand checks, the host's counting sort, uploads and downloads included; 6.5 ms, 15 %, between its first and last
kernel); the same algorithm with scipy.sparse products, numpy.linalg.qr and eigh on that box 0.97 s, the singular values equal to 3e-15
of the largest.
"""
import gzip
import io
import os
import zipfile

import numpy as np

SCALE = 1e4


class ClusterError(ValueError):
    """an input or a parameter `pyatac cluster` cannot use; one line"""


def read_counts(path):
    """either output of `pyatac cellcounts` -> (indptr int64, indices int32, data int32, barcodes list of bytes): CSR with one row per
    window, the cells ascending within a row.  BASE.cellcounts.mtx.gz comes with BASE.cellcounts.barcodes.tsv beside it."""
    if not os.path.exists(path):
        raise ClusterError("%s: no such file" % path)
    if path.endswith(".npz"):
        try:
            z = np.load(path, allow_pickle=False)
        except (ValueError, OSError, EOFError, zipfile.BadZipFile):
            raise ClusterError("%s: not a cellcounts .npz" % path)
        with z:
            for k in ("indptr", "indices", "data", "shape", "barcodes"):
                if k not in z.files:
                    raise ClusterError("%s: no array %r: not a cellcounts .npz" % (path, k))
            indptr, indices, data = z["indptr"].astype(np.int64), z["indices"].astype(np.int32), z["data"].astype(np.int32)
            barcodes = [bytes(b) for b in z["barcodes"].tolist()]
            n_rows, n_cols = (int(v) for v in z["shape"])
        if len(indptr) != n_rows + 1 or len(barcodes) != n_cols:
            raise ClusterError("%s: the arrays do not have the shape the file states" % path)
        return indptr, indices, data, barcodes
    if not path.endswith(".mtx.gz"):
        raise ClusterError("%s: expected a .cellcounts.npz or a .cellcounts.mtx.gz" % path)
    side = path[:-len(".mtx.gz")] + ".barcodes.tsv"
    if not os.path.exists(side):
        raise ClusterError("%s: no such file" % side)
    with open(side, "rb") as f:
        barcodes = [b for b in f.read().split(b"\n") if b]
    with gzip.open(path, "rb") as f:
        text = f.read()
    head, _, rest = text.partition(b"\n")
    if not head.startswith(b"%%MatrixMarket matrix coordinate"):
        raise ClusterError("%s: not a MatrixMarket coordinate file" % path)
    while rest[:1] == b"%":
        rest = rest.partition(b"\n")[2]
    dims, _, body = rest.partition(b"\n")
    try:
        n_rows, n_cols, nnz = (int(v) for v in dims.split())
        trip = np.array(body.split(), dtype=np.int64).reshape(-1, 3)
    except ValueError:
        raise ClusterError("%s: malformed MatrixMarket text" % path)
    if len(trip) != nnz or n_cols != len(barcodes):
        raise ClusterError("%s: %d entries and %d columns stated, %d entries and %d barcodes found" % (path, nnz, n_cols, len(trip), len(barcodes)))
    if nnz and (trip[:, 0].min() < 1 or trip[:, 0].max() > n_rows or trip[:, 1].min() < 1 or trip[:, 1].max() > n_cols):
        raise ClusterError("%s: an entry lies outside the %d x %d matrix" % (path, n_rows, n_cols))
    order = np.lexsort((trip[:, 1], trip[:, 0]))
    trip = trip[order]
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(trip[:, 0] - 1, minlength=n_rows), out=indptr[1:])
    return indptr, (trip[:, 1] - 1).astype(np.int32), trip[:, 2].astype(np.int32), barcodes


def tfidf_weights(indptr, indices, data, n_cells, binarize=False, min_cells=1):
    """(total int64[n_cells], row_weight float64[n_windows], col_scale float64[n_cells]) by the rule of the module docstring; a dropped
    cell or window has scale or weight 0"""
    a = np.ones(len(indices), np.int64) if binarize else np.asarray(data, np.int64)
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    total = np.zeros(n_cells, np.int64)
    np.add.at(total, np.asarray(indices, np.int64), a)
    t_w = np.zeros(len(indptr) - 1, np.int64)
    np.add.at(t_w, rows, a)
    cell_keep = total > 0
    win_keep = (np.diff(indptr) >= max(int(min_cells), 1)) & (t_w > 0)
    n_kept = int(cell_keep.sum())
    col_scale = np.zeros(n_cells, np.float64)
    col_scale[cell_keep] = 1.0 / total[cell_keep]
    row_weight = np.zeros(len(t_w), np.float64)
    row_weight[win_keep] = float(n_kept) / t_w[win_keep]
    return total, row_weight, col_scale


def depth_correlation(E, total):
    """pearson(E[:, j], log10(total)) for every column; 0 where either side is constant"""
    d = np.log10(np.asarray(total, np.float64))
    d = d - d.mean()
    Ec = E - E.mean(axis=0)
    den = np.sqrt((Ec * Ec).sum(axis=0) * (d * d).sum())
    num = Ec.T.dot(d)
    out = np.zeros(E.shape[1], np.float64)
    ok = den > 0
    out[ok] = num[ok] / den[ok]
    return out


def unit_rows(E):
    norm = np.sqrt((E * E).sum(axis=1))
    out = np.zeros_like(E)
    ok = norm > 0
    out[ok] = E[ok] / norm[ok, None]
    return out


def _sq_dist(X, C):
    """squared distances rows of X to rows of C, through one matrix product"""
    d = (X * X).sum(axis=1)[:, None] - 2.0 * X.dot(C.T) + (C * C).sum(axis=1)[None, :]
    return np.maximum(d, 0.0)


def kmeans(X, k, max_iter=100):
    """(labels int64[n] in [0, k), iterations) by the fixed rules of the module docstring; the labels are the raw centre indices"""
    centres = np.empty((k, X.shape[1]), np.float64)
    centres[0] = X[int(np.argmax(_sq_dist(X, X.mean(axis=0)[None, :])[:, 0]))]
    near = _sq_dist(X, centres[:1])[:, 0]
    for j in range(1, k):
        centres[j] = X[int(np.argmax(near))]
        near = np.minimum(near, _sq_dist(X, centres[j:j + 1])[:, 0])
    labels, it = None, 0
    while it < max_iter:
        new = np.argmin(_sq_dist(X, centres), axis=1)
        it += 1
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        for j in range(k):
            mine = labels == j
            if mine.any():                  # an emptied cluster keeps its centre
                centres[j] = X[mine].mean(axis=0)
    return labels.astype(np.int64), it


def name_clusters(labels, k):
    """rank[j] = the 0-based place of raw cluster j in the naming order: by size descending, then by lowest cell index"""
    size = np.bincount(labels, minlength=k)
    first = np.full(k, len(labels), np.int64)
    np.minimum.at(first, labels, np.arange(len(labels), dtype=np.int64))
    order = sorted(range(k), key=lambda j: (-int(size[j]), int(first[j]), j))
    rank = np.empty(k, np.int64)
    rank[order] = np.arange(k)
    return rank, size[order]


def _savez_fixed(path, **arrays):
    """numpy's .npz with the members' timestamps fixed: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def _device_svd(*args, **kw):
    from .. import get_context
    return get_context().sparse_lsi(*args, **kw)


def cluster_cells(indptr, indices, data, n_cells, clusters, components=30, oversample=10, iterations=4, method="log", binarize=False,
                  min_cells=1, max_depth_cor=0.75, max_iter=100, seed=1, svd=None):
    """the computation of `pyatac cluster` on CSR arrays -> dict(total, cell_keep, win_keep, sigma, depth_cor, components_kept, embedding,
    labels, sizes, kmeans_iterations, r).  svd(indptr, indices, data, n_cells, row_weight, col_scale, r, n_iter, q0, scale=, transform=,
    binarize=) -> (sigma, U, V) defaults to Context.sparse_lsi; it raises ValueError("rank") when the matrix has fewer than r directions."""
    if clusters < 1:
        raise ClusterError("--clusters must be at least 1 (got %d)" % clusters)
    if components < 1 or oversample < 0 or components + oversample > 64:
        raise ClusterError("--components must be at least 1, --oversample at least 0 and their sum at most 64 (got %d + %d)" % (components, oversample))
    if iterations < 1 or max_iter < 1 or min_cells < 1:
        raise ClusterError("--iterations, --max_iter and --min_cells must be at least 1")
    if method not in ("log", "linear"):
        raise ClusterError("--method must be log or linear (got %s)" % method)
    if not 0.0 <= max_depth_cor <= 1.0:
        raise ClusterError("--max_depth_cor must be in [0, 1] (got %g)" % max_depth_cor)
    r = components + oversample
    total, row_weight, col_scale = tfidf_weights(indptr, indices, data, n_cells, binarize, min_cells)
    cell_keep, win_keep = col_scale > 0, row_weight > 0
    n_kept = int(cell_keep.sum())
    if n_kept < clusters:
        raise ClusterError("%d cells kept, fewer than the %d clusters asked for" % (n_kept, clusters))
    if r > n_kept or r > int(win_keep.sum()):
        raise ClusterError("%d cells and %d windows kept, fewer than --components + --oversample = %d: lower --components"
                           % (n_kept, int(win_keep.sum()), r))
    q0 = np.random.default_rng(seed).standard_normal((len(indptr) - 1, r))
    try:
        sigma, U, V = (svd or _device_svd)(indptr, indices, data, n_cells, row_weight, col_scale, r, iterations, q0, scale=SCALE,
                                           transform=method, binarize=binarize)
    except ValueError as e:
        if str(e) != "rank":
            raise
        raise ClusterError("the weighted matrix has fewer than %d independent directions: lower --components" % r)
    E = (U[:, :components] * sigma[:components])[cell_keep]
    depth_cor = depth_correlation(E, total[cell_keep])
    comp_keep = np.flatnonzero(~(np.abs(depth_cor) > max_depth_cor))
    if len(comp_keep) < 1:
        raise ClusterError("every component tracks sequencing depth (|correlation| > %g): none is left" % max_depth_cor)
    emb = unit_rows(E[:, comp_keep])
    raw, km_it = kmeans(emb, clusters, max_iter)
    rank, sizes = name_clusters(raw, clusters)
    return dict(total=total, cell_keep=cell_keep, win_keep=win_keep, sigma=sigma, depth_cor=depth_cor, components_kept=comp_keep,
                embedding=emb, labels=rank[raw], sizes=sizes, kmeans_iterations=km_it, r=r)


def default_base(counts):
    base = os.path.basename(str(counts))
    for suf in (".cellcounts.npz", ".cellcounts.mtx.gz", ".npz", ".mtx.gz"):
        if base.endswith(suf):
            return base[:-len(suf)]
    return base


def get_cluster(args, svd=None):
    """`pyatac cluster`: writes BASE.clusters.tsv, BASE.lsi.npz and BASE.cluster.txt and returns their paths.  Everything is computed
    before the first file is written, so an error leaves nothing behind.  svd: see cluster_cells."""
    indptr, indices, data, barcodes = read_counts(args.counts)
    res = cluster_cells(indptr, indices, data, len(barcodes), args.clusters, args.components, args.oversample, args.iterations, args.method,
                        args.binarize, args.min_cells, args.max_depth_cor, args.max_iter, args.seed, svd=svd)
    base = args.out if args.out else default_base(args.counts)
    kept = np.flatnonzero(res["cell_keep"])
    labels = res["labels"]
    table = b"".join([barcodes[c] + b"\tc%d\n" % (labels[i] + 1) for i, c in enumerate(kept.tolist())])
    removed = [j + 1 for j in range(args.components) if j not in set(res["components_kept"].tolist())]
    summary = ("cells_listed\t%d\ncells_kept\t%d\ncells_dropped\t%d\nwindows_kept\t%d\nwindows_dropped\t%d\nnnz\t%d\nr\t%d\niterations\t%d\n"
               "components_removed\t%s\nkmeans_iterations\t%d\n"
               % (len(barcodes), len(kept), len(barcodes) - len(kept), int(res["win_keep"].sum()), int((~res["win_keep"]).sum()),
                  len(indices), res["r"], args.iterations, ",".join("%d" % j for j in removed) if removed else "none",
                  res["kmeans_iterations"]))
    summary += "".join("c%d\t%d\n" % (j + 1, s) for j, s in enumerate(res["sizes"].tolist()))
    paths = [base + ".clusters.tsv", base + ".lsi.npz", base + ".cluster.txt"]
    with open(paths[0], "wb") as f:
        f.write(table)
    _savez_fixed(paths[1], barcodes=np.array(barcodes, dtype="S"), embedding=res["embedding"], sigma=res["sigma"], depth_cor=res["depth_cor"],
                 kept=res["cell_keep"], components=res["components_kept"].astype(np.int64), labels=labels)
    with open(paths[2], "w") as f:
        f.write(summary)
    return paths
