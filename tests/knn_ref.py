"""natac_knn and the host rule of `pyatac doublets` restated in NumPy from the rules of include/natac.h, not from their code: the squared
distance as a column loop acc = acc + t * t (every operation an IEEE fp64 operation of NumPy, rounded once), the order by
numpy.lexsort((j, acc)), the case builders of the GPU tests and the planted-doublet recipe."""
import numpy as np

import lsi_ref


def knn(points, k, queries=None, self_offset=None):
    """(idx int32[nq, k], dist2 float64[nq, k]) by the rule; queries=None: all points, self excluded"""
    x = np.ascontiguousarray(points, np.float64)
    if queries is None:
        q, so = x, 0
    else:
        q, so = np.ascontiguousarray(queries, np.float64), -1 if self_offset is None else int(self_offset)
    nq, nr = q.shape[0], x.shape[0]
    idx = np.full((nq, k), -1, np.int32)
    d2 = np.full((nq, k), np.inf, np.float64)
    j = np.arange(nr)
    with np.errstate(under="ignore"):
        for lo in range(0, nq, 256):
            qb = q[lo:lo + 256]
            acc = np.zeros((qb.shape[0], nr), np.float64)
            for c in range(x.shape[1]):
                t = qb[:, c][:, None] - x[:, c][None, :]
                acc = acc + t * t
            for i in range(qb.shape[0]):
                order = np.lexsort((j, acc[i]))
                if so >= 0:
                    order = order[order != lo + i + so]
                order = order[:k]
                idx[lo + i, :len(order)] = order
                d2[lo + i, :len(order)] = acc[i, order]
    return idx, d2


def knn_loops(points, k):
    """the same for all points against all points, self excluded, with Python floats and sorted tuples: slow, for a handful of points"""
    x = [[float(v) for v in row] for row in points]
    idx, d2 = [], []
    for i, qi in enumerate(x):
        pairs = []
        for j, xj in enumerate(x):
            if j == i:
                continue
            acc = 0.0
            for c in range(len(qi)):
                t = qi[c] - xj[c]
                acc = acc + t * t
            pairs.append((acc, j))
        pairs.sort()
        pairs = pairs[:k] + [(float("inf"), -1)] * (k - len(pairs[:k]))
        idx.append([p[1] for p in pairs])
        d2.append([p[0] for p in pairs])
    return np.array(idx, np.int32), np.array(d2, np.float64)


def same(a, b):
    """idx equal and dist2 equal bit for bit"""
    return np.array_equal(a[0], b[0]) and a[1].shape == b[1].shape and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


# ---- case builders ----
def gauss(nr, dim, seed=0, scale=1.0):
    return np.random.default_rng(seed).standard_normal((nr, dim)) * scale


def lattice(n=16):
    """the n x n integer lattice in 2 dimensions: large groups of equal distances"""
    g = np.arange(n, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)


def ordered_from(points, query, farthest_first):
    """the points sorted by distance to `query`: farthest first makes every reference a candidate, nearest first none after the first k"""
    d = ((points - query) ** 2).sum(axis=1)
    order = np.argsort(d, kind="stable")
    return points[order[::-1] if farthest_first else order]


# ---- the planted-doublet case of `pyatac doublets` ----
def planted_doublets(seed=1):
    """(indptr, indices, data, n_cells, group int[400], pa, pb): lsi_ref.planted(seed) with 40 planted doublets appended, columns
    A[:, pa] + A[:, pb]"""
    A, group = lsi_ref.planted(seed=seed)
    rng = np.random.default_rng(101)
    pa = rng.integers(0, 400, 40)
    pb = rng.integers(0, 400, 40)
    A = A.tocsc()
    import scipy.sparse as sp
    full = sp.hstack([A, A[:, pa] + A[:, pb]]).tocsr()
    ip, ix, da = lsi_ref.csr_of(full)
    return ip, ix, da, 440, group, pa, pb


def recovered(score, group, pa, pb, top=40):
    """(heterotypic planted doublets among the `top` highest scores by (score descending, index ascending), heterotypic planted doublets)"""
    het = np.flatnonzero(group[pa] != group[pb]) + 400
    order = np.lexsort((np.arange(len(score)), -np.asarray(score)))[:top]
    return int(np.isin(het, order).sum()), len(het)


def likelihood(n_syn, k_adj, rr, rho):
    """Scrublet's likelihood in the operation order of the rule, Python floats"""
    q = (n_syn + 1) / (k_adj + 2)
    return q * rho / rr / (1 - rho - q * (1 - rho - rho / rr))
