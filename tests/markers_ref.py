"""The restatement of `pyatac markers` the tests compare with (NumPy / scipy / exact rationals on the CPU; of the package only the
MatrixMarket writer of `cellcounts` is used, for the command's input files):
the four integer arrays of natac_group_rank_sums by exact midranks (rank_sums), the host statistics one window and group at a time
(statistics), Benjamini-Hochberg (bh), the cases of the device tests (make_case; short_stride_case, block_stride_case, border_case and big_case for
the launch edges) and the command's inputs (write_counts, planted_case).
include/natac.h states the rule."""
import math
from fractions import Fraction

import numpy as np

BIG = (1 << 31) - 1


def rank_sums(indptr, indices, data, n_cells, depth, group, n_groups):
    """(detected int32[m, G], total int64[m, G], rank2 int64[m, G], ties int64[m]) in Python integers and exact rationals: an entry's
    value is Fraction(a, d[c]); less / eq are counted among the row's entries; 2 rank = 2 z0 + 2 less + eq + 1, a zero cell's z0 + 1"""
    m, N, G = len(indptr) - 1, int(n_cells), int(n_groups)
    n_g = [0] * G
    for g in group:
        n_g[int(g)] += 1
    detected = np.zeros((m, G), np.int32)
    total = np.zeros((m, G), np.int64)
    rank2 = np.zeros((m, G), np.int64)
    ties = np.zeros(m, np.int64)
    for p in range(m):
        cells = [int(c) for c in indices[indptr[p]:indptr[p + 1]]]
        counts = [int(a) for a in data[indptr[p]:indptr[p + 1]]]
        vals = [Fraction(a, int(depth[c])) for a, c in zip(counts, cells)]
        z0 = N - len(cells)
        # every distinct value: how many entries lie below it, how many are equal
        size = {}
        for v in vals:
            size[v] = size.get(v, 0) + 1
        below, seen = {}, 0
        for v in sorted(size):
            below[v] = seen
            seen += size[v]
        det, tot, rk = [0] * G, [0] * G, [0] * G
        t = z0 ** 3 - z0
        for v, a, c in zip(vals, counts, cells):
            g = int(group[c])
            det[g] += 1
            tot[g] += a
            rk[g] += 2 * z0 + 2 * below[v] + size[v] + 1
            t += size[v] ** 2 - 1
        for g in range(G):
            detected[p, g], total[p, g], rank2[p, g] = det[g], tot[g], (n_g[g] - det[g]) * (z0 + 1) + rk[g]
        ties[p] = t
    return detected, total, rank2, ties


def device_stand_in(indptr, indices, data, n_cells, depth, group, n_groups):
    """rank_sums with the signature of Context.group_rank_sums: what get_markers(args, rank=...) takes"""
    return rank_sums(np.asarray(indptr), np.asarray(indices), np.asarray(data), n_cells, np.asarray(depth), np.asarray(group), n_groups)


def statistics(detected, total, rank2, ties, depth, group, n_groups, min_cells):
    """the host part, one window and group at a time in Python floats: dict of tested bool[m] and float64[m, G] z, p, auc, pct_in, pct_rest,
    log2fc (NaN where the window is untested or the group has no cell or every cell)"""
    from scipy.stats import norm
    m, G, N = detected.shape[0], int(n_groups), len(depth)
    n_g = [int(np.sum(np.asarray(group) == g)) for g in range(G)]
    D = [sum(int(d) for d, gg in zip(depth, group) if int(gg) == g) for g in range(G)]
    D_all = sum(int(d) for d in depth)
    out = {k: np.full((m, G), np.nan) for k in ("z", "p", "auc", "pct_in", "pct_rest", "log2fc")}
    tested = np.zeros(m, bool)
    for w in range(m):
        row_det, row_tot = int(detected[w].sum()), int(total[w].sum())
        tested[w] = row_det >= min_cells
        if not tested[w]:
            continue
        for g in range(G):
            ng, nr = n_g[g], N - n_g[g]
            if ng == 0 or nr == 0:
                continue
            U = int(rank2[w, g]) / 2.0 - ng * (ng + 1) / 2.0
            mu = ng * nr / 2.0
            var = ng * nr / 12.0 * ((N + 1) - int(ties[w]) / (N * (N - 1.0)))
            if var == 0:
                z = float("nan")
            else:
                sign = (U > mu) - (U < mu)
                z = (U - mu - 0.5 * sign) / math.sqrt(var)
            out["z"][w, g] = z
            out["p"][w, g] = min(1.0, 2.0 * float(norm.sf(abs(z)))) if z == z else float("nan")
            out["auc"][w, g] = U / (float(ng) * nr)
            out["pct_in"][w, g] = int(detected[w, g]) / float(ng)
            out["pct_rest"][w, g] = (row_det - int(detected[w, g])) / float(nr)
            out["log2fc"][w, g] = math.log2(((int(total[w, g]) + 1) / float(D[g])) / ((row_tot - int(total[w, g]) + 1) / float(D_all - D[g])))
    out["tested"] = tested
    return out


def bh(p):
    """Benjamini-Hochberg over the finite values of p (the others stay NaN): rank by (p, index), q = p n / rank, then a running minimum
    from the largest rank down"""
    p = np.asarray(p, np.float64)
    q = np.full(p.shape, np.nan)
    idx = [i for i in range(len(p)) if math.isfinite(p[i])]
    idx.sort(key=lambda i: (p[i], i))
    n, low = len(idx), float("inf")
    for rank in range(n, 0, -1):
        i = idx[rank - 1]
        low = min(low, p[i] * n / rank)
        q[i] = low
    return q




COLLIDING = ((BIG, BIG - 1), (BIG - 1, BIG - 2))        # (a, d) twice: equal as fp64 quotients, different as rationals


def make_case(seed, N, G, m=300, all_in_one=False):
    """a CSR matrix of m windows x N cells with depths and groups, for the device tests.  The first rows are: 0 empty; 1 one entry;
    2 dense (L = N); 3 every value 1 through different (a, d) = (d, d); 4 every value 1/2 through (d / 2, d) over the cells of even
    depth (1/2, 2/4, 3/6 ...); 5 the pair COLLIDING in cells 0 and 1; 6 counts next to 2^31 - 1 over cells some of which are as deep.
    The other rows have between 0 and N entries, short ones most often, with counts 1 .. 5 over depths 1 .. 39: many tied values.
    Groups: with all_in_one every cell is in group G // 2; else with G > 2 group G - 1 has no cell and the others are drawn evenly.
    Returns dict(indptr, indices, data, depth, group, N, G)."""
    rng = np.random.default_rng(seed)
    if all_in_one:
        group = np.full(N, G // 2, np.int32)
    else:
        group = rng.integers(0, G - 1 if G > 2 else G, N).astype(np.int32)
    depth = rng.integers(1, 40, N).astype(np.int64)
    depth[0], depth[1] = COLLIDING[0][1], COLLIDING[1][1]
    deep = rng.choice(np.arange(2, N), min(N - 2, 3), replace=False) if N > 2 else np.zeros(0, np.int64)
    depth[deep] = [BIG, BIG - 1, 1 << 30][:len(deep)]
    some = lambda k: np.sort(rng.choice(N, k, replace=False))       # noqa: E731
    rows = [(np.zeros(0, np.int64), [])]
    rows.append((some(1), [3]))
    rows.append((np.arange(N), rng.integers(1, 5, N).tolist()))
    cells = some(max(2, (2 * N) // 3))
    rows.append((cells, [int(depth[c]) for c in cells]))
    even = np.flatnonzero(depth % 2 == 0)
    rows.append((even, [int(depth[c]) // 2 for c in even]))
    rows.append((np.array([0, 1]), [COLLIDING[0][0], COLLIDING[1][0]]))
    cells = np.union1d(some(min(N, 7)), deep).astype(np.int64)
    rows.append((cells, [int(v) for v in rng.choice([BIG, BIG - 1, BIG - 2, 1, 2], len(cells))]))
    while len(rows) < m:
        u = rng.random()
        top = min(N, 12) if u < 0.6 else min(N, 80) if u < 0.85 else N
        cells = some(int(rng.integers(0, top + 1)))
        rows.append((cells, rng.integers(1, 6, len(cells)).tolist()))
    indptr = np.zeros(m + 1, np.int64)
    indptr[1:] = np.cumsum([len(r[0]) for r in rows])
    indices = np.array([c for r in rows for c in r[0]], np.int32)
    data = np.array([a for r in rows for a in r[1]], np.int32)
    return dict(indptr=indptr, indices=indices, data=data, depth=depth, group=group, N=N, G=G)


# ---- the cases of tests/test_gpu_markers_launch_edges.py (sized on the CPU by tests/test_markers_host.py) -----------------------------------
def case_of_rows(rows, depth, group, G):
    """make_case's dict from rows of (cells ascending, counts)"""
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r[0]) for r in rows])
    indices = np.concatenate([np.asarray(r[0], np.int64) for r in rows]).astype(np.int32)
    data = np.concatenate([np.asarray(r[1], np.int64) for r in rows]).astype(np.int32)
    return dict(indptr=indptr, indices=indices, data=data, depth=np.asarray(depth, np.int64), group=np.asarray(group, np.int32), N=len(depth), G=G)


def _case_of_lengths(rng, L, N, G):
    """a case whose row p has L[p] cells drawn without replacement, counts 1 .. 5 over depths 1 .. 39 (many tied values), every group drawn
    evenly"""
    L = np.asarray(L, np.int64)
    first = np.argsort(rng.random((len(L), N)), axis=1)                 # a permutation of the cells per row: its first L[p] are the row's
    member = np.zeros((len(L), N), bool)
    np.put_along_axis(member, first, np.arange(N)[None, :] < L[:, None], axis=1)
    indptr = np.zeros(len(L) + 1, np.int64)
    np.cumsum(L, out=indptr[1:])
    indices = np.nonzero(member)[1].astype(np.int32)                    # row-major: ascending within a row
    return dict(indptr=indptr, indices=indices, data=rng.integers(1, 6, len(indices)).astype(np.int32),
                depth=rng.integers(1, 40, N).astype(np.int64), group=rng.integers(0, G, N).astype(np.int32), N=N, G=G)


def short_stride_case(seed, n_rows, per_trip, N=48, G=5, top=8, lead=None):
    """n_rows rows of 0 .. top entries for the short arm, whose workgroups take per_trip rows a trip (rows a workgroup x grid): row
    per_trip + j follows row j in one lane group.  Two of three such pairs are a full row (top entries) followed by an empty row and by
    a row of one entry, so that what the first leaves in the counters would be counted.  lead: the entries of row 0 (it sets the lanes)."""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, top + 1, n_rows)
    j = np.arange(max(0, n_rows - per_trip))
    L[j[j % 3 != 2]] = top
    L[per_trip + j[j % 3 == 0]] = 0
    L[per_trip + j[j % 3 == 1]] = 1
    if lead is not None:
        L[0] = lead
    return _case_of_lengths(rng, L, N, G)


def block_stride_case(seed, n_block, grid, short_max=4, N=48, G=5):
    """n_block rows of short_max + 1 .. 40 entries for the block arm under NATAC_MARKERS_SHORT_MAX = short_max, launched with `grid`
    workgroups: block row grid + j follows block row j in one workgroup.  Two of three such pairs are a row of 40 entries followed by one
    of short_max + 1 and of short_max + 2.  After every fourth block row stands a row of 0 .. short_max entries (the short arm's).
    Returns (case, the index of every block row)."""
    rng = np.random.default_rng(seed)
    Lb = rng.integers(short_max + 1, 41, n_block)
    j = np.arange(max(0, n_block - grid))
    Lb[j[j % 3 != 2]] = 40
    Lb[grid + j[j % 3 == 0]] = short_max + 1
    Lb[grid + j[j % 3 == 1]] = short_max + 2
    L, where = [], []
    for b in range(n_block):
        where.append(len(L))
        L.append(int(Lb[b]))
        if b % 4 == 3:
            L.append((b // 4) % (short_max + 1))
    return _case_of_lengths(rng, L, N, G), np.array(where)


BORDER_ROWS = (0, 1, 64, 65, 4096, 4097, 8192, 8193, 9000)             # entries of the first rows of border_case: every arm's borders


def border_case(seed, G, N=9000):
    """rows of BORDER_ROWS entries with counts 1 .. 5 over depths 1 .. 39; row 9: 8500 entries whose values are all 1 through (d, d);
    row 10: 8700 entries that hold the pair COLLIDING in cells 0 and 1.  Groups as make_case draws them."""
    rng = np.random.default_rng(seed)
    group = np.zeros(N, np.int32) if G == 1 else rng.integers(0, G - 1 if G > 2 else G, N).astype(np.int32)
    depth = rng.integers(1, 40, N).astype(np.int64)
    depth[0], depth[1] = COLLIDING[0][1], COLLIDING[1][1]
    some = lambda k: np.sort(rng.choice(N, k, replace=False))       # noqa: E731
    rows = []
    for k in BORDER_ROWS:
        rows.append((some(k), rng.integers(1, 6, k)))
    cells = some(8500)
    rows.append((cells, depth[cells]))
    cells = np.union1d([0, 1], 2 + np.sort(rng.choice(N - 2, 8698, replace=False)))
    counts = rng.integers(1, 6, len(cells))
    counts[0], counts[1] = COLLIDING[0][0], COLLIDING[1][0]
    rows.append((cells, counts))
    return case_of_rows(rows, depth, group, G)


def big_case(seed, N=1 << 20, G=3):
    """N cells: row 0 empty; 1 the last cell only; 2 the first cell only; 3 10,000 entries (the long arm); 4 5,000 entries (the block
    arm); 5 40 entries"""
    rng = np.random.default_rng(seed)
    group = rng.integers(0, G, N).astype(np.int32)
    depth = rng.integers(1, 40, N).astype(np.int64)
    rows = [(np.zeros(0, np.int64), np.zeros(0, np.int64)), (np.array([N - 1]), np.array([3])), (np.array([0]), np.array([2]))]
    for k in (10000, 5000, 40):
        cells = np.sort(rng.choice(N, k, replace=False))
        if k == 10000:
            cells[-1] = N - 1                                           # the long row reaches the last cell
        rows.append((cells, rng.integers(1, 6, k)))
    return case_of_rows(rows, depth, group, G)


# ---- the command's inputs ----------------------------------------------------------------------------------------------------------------
def csr_of(A):
    """(indptr int64, indices int32, data int32) of the positive entries of a dense matrix"""
    A = np.asarray(A, np.int64)
    r, c = np.nonzero(A)
    indptr = np.zeros(A.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=A.shape[0]), out=indptr[1:])
    return indptr, c.astype(np.int32), A[r, c].astype(np.int32)


def regions(n, width=40):
    chrom = ["chrA" if i % 3 else "chrB" for i in range(n)]
    start = np.array([i * 50 for i in range(n)], np.int64)
    return chrom, start, start + width


def write_counts(base, X, barcodes, fmt, with_regions=True):
    """what `cellcounts --format fmt` writes, as far as `markers` reads it (the MatrixMarket text is get_cellcounts.mtx_text's) -> path"""
    import gzip
    from nucleoatac_amd.pyatac.get_cellcounts import mtx_text
    ip, ix, da = csr_of(X)
    c, s, e = regions(len(X))
    if fmt == "npz":
        reg = dict(region_chrom=np.array(c, dtype="U"), region_start=s, region_end=e) if with_regions else {}
        np.savez_compressed(base + ".cellcounts.npz", indptr=ip, indices=ix, data=da, shape=np.array(np.shape(X), np.int64),
                            barcodes=np.array(barcodes, dtype="S"), **reg)
        return base + ".cellcounts.npz"
    with gzip.open(base + ".cellcounts.mtx.gz", "wb") as f:
        f.write(mtx_text(ip, ix, da, np.shape(X)[1]))
    with open(base + ".cellcounts.barcodes.tsv", "wb") as f:
        f.write(b"".join(b + b"\n" for b in barcodes))
    if with_regions:
        with open(base + ".cellcounts.regions.bed", "w") as f:
            f.write("".join("%s\t%d\t%d\n" % r for r in zip(c, s.tolist(), e.tolist())))
    return base + ".cellcounts.mtx.gz"


def planted_case(seed=3, n_groups=3, per_group=60, n_windows=400, planted=40, fold=8.0):
    """a dense count matrix of n_windows x (n_groups * per_group) cells in which windows [g * planted, (g + 1) * planted) are `fold` times
    more open in group g than elsewhere -> (X int64, barcodes, group index of every cell)"""
    rng = np.random.default_rng(seed)
    n = n_groups * per_group
    grp = np.arange(n) % n_groups
    depth = rng.uniform(0.5, 2.0, n)
    rate = np.full((n_windows, n), 0.06) * depth[None, :]
    for g in range(n_groups):
        rate[g * planted:(g + 1) * planted, grp == g] *= fold
    X = rng.poisson(rate).astype(np.int64)
    return X, [b"CELL%04d" % i for i in range(n)], grp
