"""The restatement of `pyatac coaccess` the tests compare with (NumPy / scipy / Python integers / decimal on the CPU; of the package only
the MatrixMarket writer of `cellcounts` is used, for the command's input files): the pair lists by a plain double loop (pair_lists), the
two integer arrays of natac_window_pair_sums in Python integers (pair_sums) and from scipy.sparse int64 products restricted to the pairs
(pair_sums_sparse), r by the stated operation order one pair at a time (r_of) and in 50-digit decimal from the exact integers
(r_decimal), the cases of the device tests (make_case; stride_case for a second trip of the grid) and the command's inputs (write_counts, command_case).  include/natac.h states the
rule."""
import math
from decimal import Decimal, getcontext

import numpy as np


def pair_lists(chrom, start, end, tested, max_distance):
    """(order, hi): per chromosome in order of first appearance, the tested windows by (centre, index); hi[i] = one past the last later
    window of the chromosome whose centre is at most max_distance past that of order[i] -- by a double loop"""
    seen = []
    for c in chrom:
        if c not in seen:
            seen.append(c)
    order, hi = [], []
    for c in seen:
        mine = sorted(((int(start[w]) + int(end[w])) // 2, w) for w in range(len(chrom)) if chrom[w] == c and tested[w])
        base = len(order)
        for i, (ci, _) in enumerate(mine):
            last = i
            for j in range(i + 1, len(mine)):
                if mine[j][0] - ci <= max_distance:
                    last = j
            hi.append(base + last + 1)
        order += [w for _, w in mine]
    return np.array(order, np.int32), np.array(hi, np.int64)


def pairs_of(order, hi):
    """(pair_a, pair_b): the owner and the partner of every pair, in the order of the outputs"""
    a, b = [], []
    for i in range(len(order)):
        for j in range(i + 1, int(hi[i])):
            a.append(int(order[i]))
            b.append(int(order[j]))
    return np.array(a, np.int64), np.array(b, np.int64)


def pair_sums(indptr, indices, data, n_cells, order, hi):
    """(sxy int64, both int32) per pair, in Python integers; the signature of Context.window_pair_sums, so that it is what
    get_coaccess(args, pairs=...) takes"""
    rows = [dict(zip(indices[indptr[p]:indptr[p + 1]].tolist(), (int(v) for v in data[indptr[p]:indptr[p + 1]]))) for p in range(len(indptr) - 1)]
    sxy, both = [], []
    for p, q in zip(*pairs_of(order, hi)):
        common = [c for c in rows[q] if c in rows[p]]
        s = sum(rows[p][c] * rows[q][c] for c in common)
        assert s < 1 << 63
        sxy.append(s)
        both.append(len(common))
    return np.array(sxy, np.int64), np.array(both, np.int32)


def pair_sums_sparse(indptr, indices, data, n_cells, order, hi):
    """the same from scipy.sparse: the int64 elementwise product of the owners' and the partners' rows, summed per pair"""
    import scipy.sparse as sp
    m = len(indptr) - 1
    X = sp.csr_matrix((np.asarray(data, np.int64), np.asarray(indices, np.int64), np.asarray(indptr, np.int64)), shape=(m, int(n_cells)))
    a, b = pairs_of(order, hi)
    if not len(a):
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    P = X[a].multiply(X[b]).tocsr()
    return np.asarray(P.sum(axis=1)).ravel().astype(np.int64), np.diff(P.indptr).astype(np.int32)


def row_sums(indptr, data):
    """(det, S1, S2) per row in Python integers"""
    det, s1, s2 = [], [], []
    for p in range(len(indptr) - 1):
        a = [int(v) for v in data[indptr[p]:indptr[p + 1]]]
        det.append(len(a))
        s1.append(sum(a))
        s2.append(sum(v * v for v in a))
    return det, s1, s2


def r_of(N, sxy, s1p, s1q, s2p, s2q):
    """r of one pair in Python floats by the stated order; NaN where a D is 0"""
    num = N * sxy - s1p * s1q
    Dp, Dq = N * s2p - s1p * s1p, N * s2q - s1q * s1q
    if Dp == 0 or Dq == 0:
        return float("nan")
    return max(-1.0, min(1.0, float(num) / math.sqrt(float(Dp) * float(Dq))))


def r_decimal(N, sxy, s1p, s1q, s2p, s2q):
    """r of one pair to 50 digits from the exact integers (None where a D is 0)"""
    getcontext().prec = 50
    num = N * sxy - s1p * s1q
    Dp, Dq = N * s2p - s1p * s1p, N * s2q - s1q * s1q
    if Dp == 0 or Dq == 0:
        return None
    return Decimal(num) / (Decimal(Dp) * Decimal(Dq)).sqrt()


def p_of(r, N):
    from scipy.stats import t as student
    if r != r:
        return float("nan")
    if abs(r) == 1.0:
        return 0.0
    t = r * math.sqrt((N - 2) / ((1.0 - r) * (1.0 + r)))
    return 2.0 * float(student.sf(abs(t), N - 2))


def make_case(seed, m, N, mean_len, partners=10, max_count=5, long_rows=(), alone_every=0):
    """a CSR matrix of m windows x N cells with its `order` and `hi`, for the device tests.  Planted rows: 0 empty; 1 one entry; 2 every
    cell; 3 and 4 identical (r == 1); 5 and 6 with disjoint columns; long_rows[j] entries in row 7 + j.  The other rows have about
    mean_len entries (between 0 and min(N, 2 mean_len)) with counts 1 .. max_count.  order: two "chromosomes", so no pair crosses -- rows
    0, 2, 5, 6 and then the other even rows shuffled; rows 3, 4, 3 (one window listed twice), 1, the long rows and then the other odd
    rows shuffled.  Every owner reaches partners // 2 to 2 x partners windows ahead (fewer at its chromosome's end: the last owner has
    none), and one owner in the middle of each chromosome has none (hi[i] == i + 1); the planted rows open their chromosomes, so each is
    an owner with partners.  alone_every = e > 0: every e-th owner of a chromosome (i % e == e - 1) has none either.  Returns
    dict(indptr, indices, data, N, order, hi)."""
    rng = np.random.default_rng(seed)
    some = lambda k: np.sort(rng.choice(N, k, replace=False))       # noqa: E731
    rows = [(np.zeros(0, np.int64), [])]
    rows.append((some(1), [3]))
    rows.append((np.arange(N), rng.integers(1, max_count + 1, N).tolist()))
    cells = some(max(2, N // 3))
    vals = rng.integers(1, max_count + 1, len(cells)).tolist()
    vals[0] = vals[1] + 1 if len(vals) > 1 else vals[0]                # not constant: D > 0
    rows.append((cells, vals))
    rows.append((cells, list(vals)))
    half = rng.permutation(N)
    rows.append((np.sort(half[:N // 2]), rng.integers(1, max_count + 1, N // 2).tolist()))
    rows.append((np.sort(half[N // 2:]), rng.integers(1, max_count + 1, N - N // 2).tolist()))
    for L in long_rows:
        rows.append((some(L), rng.integers(1, max_count + 1, L).tolist()))
    while len(rows) < m:
        cells = some(int(rng.integers(0, min(N, 2 * mean_len) + 1)))
        rows.append((cells, rng.integers(1, max_count + 1, len(cells)).tolist()))
    indptr = np.zeros(m + 1, np.int64)
    indptr[1:] = np.cumsum([len(r[0]) for r in rows])
    indices = np.array([c for r in rows for c in r[0]], np.int32)
    data = np.array([a for r in rows for a in r[1]], np.int32)
    n_planted = 7 + len(long_rows)
    order, hi = [], []
    for parity, planted in ((0, [0, 2, 5, 6]), (1, [3, 4, 3, 1] + list(range(7, n_planted)))):
        rest = [w for w in range(n_planted, m) if w % 2 == parity]
        mine = planted + rng.permutation(rest).tolist()
        base, n = len(order), len(mine)
        alone = n // 2
        for i in range(n):
            reach = 0 if i == alone or (alone_every and i % alone_every == alone_every - 1) else int(rng.integers(max(1, partners // 2), 2 * partners + 1))
            hi.append(base + min(n, i + 1 + reach))
        order += mine
    return dict(indptr=indptr, indices=indices, data=data, N=N, order=np.array(order, np.int32), hi=np.array(hi, np.int64))


STRIDE_PLANTS = ((2, 0), (2, 1), (1, 2), (5, 3), (3, 5), (2, 6))        # (row of owner i, row of owner i + grid): see stride_case


def stride_case(seed, grid):
    """make_case(seed, m, 64, 8, partners=3, alone_every=7) with m = max(3000, 7 / 6 (grid + 600)) windows, so that six owners of seven
    have partners and those exceed the grid by 500, for a launch of `grid` workgroups, where owner i + grid follows owner i in one
    workgroup: at six places with partners on both sides, i and i + grid are given the rows of STRIDE_PLANTS -- every cell (row 2, 64
    entries) followed by the empty row, by the row of one entry and by a row of 32; one entry followed by every cell; 32 entries
    followed by about 21 and the reverse.  Returns (case, [(i, row of i, row of i + grid)])."""
    case = make_case(seed, max(3000, (grid + 600) * 7 // 6), 64, 8, partners=3, alone_every=7)
    order, hi = case["order"].copy(), case["hi"]
    k = len(order)
    has = hi - np.arange(k) > 1
    free = [i for i in range(16, k - grid) if has[i] and has[i + grid]]
    planted = []
    for (first, second), i in zip(STRIDE_PLANTS, free[::len(free) // len(STRIDE_PLANTS)]):
        order[i], order[i + grid] = first, second
        planted.append((i, first, second))
    return dict(case, order=order), planted


# ---- the command's inputs ----------------------------------------------------------------------------------------------------------------
def csr_of(A):
    """(indptr int64, indices int32, data int32) of the positive entries of a dense matrix"""
    A = np.asarray(A, np.int64)
    r, c = np.nonzero(A)
    indptr = np.zeros(A.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=A.shape[0]), out=indptr[1:])
    return indptr, c.astype(np.int32), A[r, c].astype(np.int32)


def regions(n, spacing=2000, width=500):
    """two chromosomes, interleaved in the file as chrA chrA chrB ...; within a chromosome the windows are `spacing` apart, two of them
    (3 and 6) share a centre, and every seventh from 4 on is wider, so that its centre lies past that of the chromosome's next window: file
    order and centre order differ"""
    chrom = ["chrB" if i % 3 == 2 else "chrA" for i in range(n)]
    start = np.array([(i // 3) * spacing * 2 + (i % 3 == 1) * spacing for i in range(n)], np.int64)
    end = start + width
    if n > 7:
        start[6], end[6] = start[3], end[3]                            # a tie in centre: the index decides
        end[4::7] += 5 * spacing
    return chrom, start, end


def write_counts(base, X, barcodes, fmt, with_regions=True):
    """what `cellcounts --format fmt` writes, as far as `coaccess` reads it (the MatrixMarket text is get_cellcounts.mtx_text's) -> path"""
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


def command_case(seed=2, n_windows=40, n_cells=30, n_groups=6):
    """a dense count matrix in which windows 3 k, 3 k + 1 (neighbours on chrA) follow one of four hidden programmes per cell group, so that
    there are links; one cell has no count; -> (X int64, barcodes, group index of every cell)"""
    rng = np.random.default_rng(seed)
    grp = np.arange(n_cells) % n_groups
    programme = rng.integers(0, 4, n_windows // 3 + 1)
    level = rng.uniform(0.1, 3.0, (4, n_groups))
    rate = np.empty((n_windows, n_cells))
    for w in range(n_windows):
        rate[w] = level[programme[w // 3]][grp] if w % 3 != 2 else 0.7
    X = rng.poisson(rate).astype(np.int64)
    X[:, 5] = 0
    return X, [b"CELL%04d" % i for i in range(n_cells)], grp
