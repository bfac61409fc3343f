"""NumPy restatement of `pyatac genescores` (include/natac.h states the rule), written from the header and shared by the host and the
GPU tests: both insertion arrays with their cells, per gene two boolean masks and numpy.bincount(cell, weights), the window rule and the
weight table, make_case, the crafted chromosome the GPU tests run on, and what the stride tests ask of a case (window_hits, tile_pairs)."""
import numpy as np

SHORT_MAX = 64          # NATAC_GENESCORES_SHORT_CAP
MAX_WEIGHT = 1 << 20    # NATAC_GENESCORES_MAX_WEIGHT


def insertions(pos, tlen, cell, lower, upper):
    """(x, c): the insertions of the records that pass the size filter, left ends first, and their cells"""
    pos, tlen, cell = np.asarray(pos, np.int64), np.asarray(tlen, np.int64), np.asarray(cell, np.int64)
    l, ilen = pos + 4, tlen - 8
    r = l + ilen - 1
    ok = (ilen >= lower) & (ilen < upper)
    return np.concatenate([l[ok], r[ok]]), np.concatenate([cell[ok], cell[ok]])


def gene_row(x, c, n_cells, wl, wh, bs, be, weight):
    """(sum int64[n_cells], hits) of one gene"""
    in_win = (x >= wl) & (x < wh)
    in_body = (x >= bs) & (x < be)
    d = np.where(in_body, 0, np.where(x < bs, bs - x, x - be + 1))
    w = np.asarray(weight, np.int64)[d[in_win]]
    return np.bincount(c[in_win], weights=w, minlength=n_cells).astype(np.int64), int(in_win.sum())


def gene_cell_scores(pos, tlen, cell, n_cells, win_lo, win_hi, body_lo, body_hi, weight, lower, upper, with_hits=False, with_arm_rows=False,
                     with_kernel_ms=False, short_max=SHORT_MAX):
    """Context.gene_cell_scores restated: (indptr int64, indices int32, data int32[, hits int64][, arm_rows int64[2]][, 0.0]).  The
    entry's one device bound, hits * max(weight) < 2^31, raises NatacError as the library does."""
    from nucleoatac_amd._lib import NatacError
    x, c = insertions(pos, tlen, cell, lower, upper)
    n = len(win_lo)
    indptr, cols, vals, hits = np.zeros(n + 1, np.int64), [], [], np.zeros(n, np.int64)
    for g in range(n):
        s, hits[g] = gene_row(x, c, n_cells, win_lo[g], win_hi[g], body_lo[g], body_hi[g], weight)
        if hits[g] * int(np.max(weight)) >= 1 << 31:
            raise NatacError(-1, "gene %d: %d insertions count and the largest weight is %d: an entry could reach 2^31" % (g, hits[g], np.max(weight)))
        nz = np.flatnonzero(s)
        cols.append(nz)
        vals.append(s[nz])
        indptr[g + 1] = indptr[g] + len(nz)
    res = (indptr, np.concatenate(cols).astype(np.int32) if n else np.zeros(0, np.int32),
           np.concatenate(vals).astype(np.int32) if n else np.zeros(0, np.int32))
    if with_hits:
        res += (hits,)
    if with_arm_rows:
        res += (np.array([np.count_nonzero((hits > 0) & (hits <= short_max)), np.count_nonzero(hits > short_max)], np.int64),)
    return res + (0.0,) if with_kernel_ms else res


def gene_windows(chrom, start, end, minus, upstream, e_min, e_max, boundaries=True):
    """the window rule, gene by gene: (bs, be, wl, wh) as lists of int"""
    n = len(start)
    bs = [int(start[g]) if minus[g] else max(0, int(start[g]) - upstream) for g in range(n)]
    be = [int(end[g]) + upstream if minus[g] else int(end[g]) for g in range(n)]
    wl, wh = [], []
    for g in range(n):
        others = [h for h in range(n) if h != g and chrom[h] == chrom[g]] if boundaries else []
        before = [be[h] for h in others if be[h] <= bs[g]]
        after = [bs[h] for h in others if bs[h] >= be[g]]
        lo = max(bs[g] - e_max, min(bs[g] - e_min, max(before))) if before else bs[g] - e_max
        hi = min(be[g] + e_max, max(be[g] + e_min, min(after))) if after else be[g] + e_max
        wl.append(max(0, lo))
        wh.append(hi)
    return bs, be, wl, wh


def weight_table(e_max, decay, unit):
    return np.array([int(np.rint(unit * (np.exp(-d / decay) + np.exp(-1.0)))) for d in range(e_max + 1)], np.int32)


CHROM_LEN = 200_000
REACH = 3000            # a window reaches at most this far beyond its body: n_w = REACH + 1
_DESERTS = ((148_500, 153_500), (159_000, 165_000), (169_000, 177_000))     # no random record has an insertion in these


def make_case(seed, n_frags=6000, n_cells=100, n_genes=120, lower=0, upper=1000):
    """one chromosome of 200,000 bases as the GPU tests take it: dict of pos (sorted), tlen, cell, n_cells, win_lo, win_hi, body_lo,
    body_hi, weight, lower, upper and `special`, the row index of every crafted gene (found again after the genes are shuffled):
    none (no insertion reaches it), one (exactly one hit), h64 and h65 (exactly 64 and 65 hits; h65's cells lie in the upper 15 % of the
    cell range), all (its window covers every record), twin_a / twin_b (identical), lap_a / lap_b (overlapping), empty_body
    (body_lo == body_hi), flush (win_lo == body_lo), both (a record with both insertions inside).  The records hold ilen 0 and 1,
    negative ilen (filtered by lower = 0) and ilen >= upper; the last cell has no record."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, CHROM_LEN - 1000, n_frags)
    tlen = rng.choice([40, 90, 150, 210, 400, 700], n_frags) + rng.integers(0, 40, n_frags) + 8
    tlen[:40] = rng.integers(0, 8, 40)                      # ilen < 0: filtered by lower
    tlen[40:80] = 8 + upper + rng.integers(0, 300, 40)      # filtered by upper
    tlen[80:100] = 8                                        # ilen 0: r == l - 1
    tlen[100:120] = 9                                       # ilen 1: r == l
    l, r = pos + 4, pos + 4 + tlen - 8 - 1
    keep = np.ones(n_frags, bool)
    for a, b in _DESERTS:                                   # 2000 bases more than the longest record on either side
        keep &= (np.maximum(l, r) < a - 2000) | (np.minimum(l, r) >= b + 2000)
    pos, tlen = pos[keep], tlen[keep]
    cell = rng.integers(0, n_cells - 1, len(pos))
    top = (max(0, int(n_cells * 0.85)), n_cells - 1)        # the upper cells (never the last)
    plant_pos, plant_tlen, plant_cell = [162_000 - 4], [300 + 8], [n_cells - 2]             # `one`: l = 162000 in, r = 162299 out
    for k, (n, a) in enumerate(((64, 171_000), (65, 173_000))):                              # l in [a, a + 200), r beyond a + 500
        plant_pos += (a + rng.integers(0, 200, n) - 4).tolist()
        plant_tlen += (600 + rng.integers(0, 100, n) + 8).tolist()
        plant_cell += (rng.integers(0, max(1, (n_cells - 1) // 3), n) if k == 0 else rng.integers(top[0], top[1], n)).tolist()
    plant_pos.append(100_000 - 4)                           # `both`: l = 100000, r = 100049
    plant_tlen.append(50 + 8)
    plant_cell.append(0)
    pos = np.concatenate([pos, plant_pos]).astype(np.int64)
    tlen = np.concatenate([tlen, plant_tlen]).astype(np.int64)
    cell = np.concatenate([cell, plant_cell]).astype(np.int32)
    order = np.argsort(pos, kind="stable")
    pos, tlen, cell = pos[order], tlen[order], cell[order]
    # genes as (wl, bs, be, wh)
    genes = dict(none=(150_000, 150_500, 151_500, 152_000), one=(161_990, 162_000, 162_005, 162_010), h64=(171_000, 171_100, 171_300, 171_500),
                 h65=(173_000, 173_100, 173_300, 173_500), all=(0, 2_500, CHROM_LEN - 2_000, CHROM_LEN + 500), twin_a=(60_000, 61_000, 62_000, 64_500),
                 twin_b=(60_000, 61_000, 62_000, 64_500), lap_a=(80_000, 81_000, 83_000, 84_000), lap_b=(81_500, 82_000, 85_000, 86_000),
                 empty_body=(90_000, 91_000, 91_000, 92_500), flush=(95_000, 95_000, 96_000, 96_700), both=(99_990, 99_995, 100_060, 100_100))
    rows = list(genes.values())
    while len(rows) < n_genes:
        bs = int(rng.integers(3_000, 140_000))
        be = bs + int(rng.choice([0, 1, 300, 2_000]))
        reach = int(rng.choice([100, 600, REACH]))           # narrow windows too: rows of a few hits
        rows.append((max(0, bs - int(rng.integers(0, reach + 1))), bs, be, be + int(rng.integers(0, reach + 1))))
    perm = rng.permutation(len(rows))                       # unsorted
    g = np.array(rows, np.int64)[perm]
    special = {name: int(np.flatnonzero(perm == k)[0]) for k, name in enumerate(genes)}
    weight = weight_table(REACH, 1500, 64)
    return dict(pos=pos, tlen=tlen, cell=cell, n_cells=n_cells, win_lo=g[:, 0].copy(), body_lo=g[:, 1].copy(), body_hi=g[:, 2].copy(),
                win_hi=g[:, 3].copy(), weight=weight, lower=lower, upper=upper, special=special)


def window_hits(case):
    """hits per gene of a make_case by two binary searches in the sorted insertions: gene_cell_scores' hits without its rows"""
    x, _ = insertions(case["pos"], case["tlen"], case["cell"], case["lower"], case["upper"])
    x = np.sort(x)
    return (np.searchsorted(x, case["win_hi"], "left") - np.searchsorted(x, case["win_lo"], "left")).astype(np.int64)


def tile_pairs(indptr, indices, rows, tile, n_tiles):
    """int64[len(rows) * n_tiles]: the entries of row rows[r] whose cell lies in tile t, at r * n_tiles + t -- the table arm's items in
    the order its workgroups take them"""
    out = np.zeros(len(rows) * n_tiles, np.int64)
    for r, g in enumerate(rows):
        out[r * n_tiles:(r + 1) * n_tiles] = np.bincount(indices[indptr[g]:indptr[g + 1]] // tile, minlength=n_tiles)
    return out


def planted_world(seed=7, n_groups=3, per_group=30, n_genes=30, background=300, extra=15):
    """a fragment file of n_groups planted cell groups on one chromosome: gene i is [5000 + 10000 i, 7000 + 10000 i), named GENE<i>, in
    set i % n_groups; every cell has `background` fragments anywhere and a cell of group k `extra` more with their left end within 2 kb of
    every gene of set k -> dict of text (the fragment lines, bytes), barcodes, group (index per cell), genes (the BED text), table (the
    barcode / group table text), records {chrom: (pos, tlen, cell)} sorted by pos, and sets (list of gene index lists).  With the
    command's defaults the markers of group k are the genes of set k and only those, for the restatement and so for the device."""
    rng = np.random.default_rng(seed)
    n, length = n_groups * per_group, 10000 * n_genes + 5000
    barcodes = [b"PLANT%03d" % i for i in range(n)]
    group = np.arange(n) % n_groups
    starts, cells = [], []
    for c in range(n):
        s = [rng.integers(0, length - 700, background)]
        for i in range(group[c], n_genes, n_groups):
            s.append(rng.integers(5000 + 10000 * i - 2000, 7000 + 10000 * i + 2000, extra))
        s = np.concatenate(s)
        starts.append(s)
        cells.append(np.full(len(s), c))
    start, cell = np.concatenate(starts).astype(np.int64), np.concatenate(cells).astype(np.int32)
    ilen = rng.integers(30, 600, len(start))
    order = np.lexsort((cell, start))
    start, cell, ilen = start[order], cell[order], ilen[order]
    text = "".join("chrP\t%d\t%d\t%s\t1\n" % (s, s + n_, barcodes[c].decode()) for s, n_, c in zip(start.tolist(), ilen.tolist(), cell.tolist()))
    genes = "".join("chrP\t%d\t%d\tGENE%d\t0\t%s\n" % (5000 + 10000 * i, 7000 + 10000 * i, i, "+-"[i % 2]) for i in range(n_genes))
    table = "".join("%s\tg%d\n" % (b.decode(), g) for b, g in zip(barcodes, group))
    return dict(text=text.encode(), barcodes=barcodes, group=group, genes=genes, table=table, records={"chrP": (start - 4, ilen + 8, cell)},
                sets=[list(range(k, n_genes, n_groups)) for k in range(n_groups)])


def planted_chain(tmp_path, score, rank):
    """writes planted_world, runs `genescores` and then `markers` on its matrix -> (world, the matrix as (indptr, indices, data),
    {group: set of marker names}).  score / rank: the device calls of the two commands, None for the device itself."""
    from helpers import bgzf_bytes
    from nucleoatac_amd.pyatac.cli import pyatac_parser
    from nucleoatac_amd.pyatac.get_genescores import get_genescores
    from nucleoatac_amd.pyatac.get_markers import get_markers
    w = planted_world()
    frag, genes, table = str(tmp_path / "planted.tsv.gz"), str(tmp_path / "planted.genes.bed"), str(tmp_path / "planted.groups.tsv")
    open(frag, "wb").write(bgzf_bytes(w["text"], blk=60000))
    open(genes, "w").write(w["genes"])
    open(table, "w").write(w["table"])
    base = str(tmp_path / "planted")
    # --upstream 2000: the extended bodies of neighbouring genes of opposite strands stay apart, so every window stops at its neighbours
    mat = get_genescores(pyatac_parser().parse_args(["genescores", "--fragments", frag, "--cells", table, "--genes", genes, "--upstream", "2000",
                                                     "--out", base]), score=score)
    paths = get_markers(pyatac_parser().parse_args(["markers", "--counts", base + ".genescores.npz", "--groups", table, "--out", base]), rank=rank)
    return w, mat, markers_by_group(open(paths[1]).read())


def markers_by_group(tsv_text):
    """{group: set of names} from a BASE.markers.tsv that carries the `name` column"""
    rows = [ln.split("\t") for ln in tsv_text.split("\n")[1:] if ln]
    out = {}
    for r in rows:
        out.setdefault(r[0], set()).add(r[-1])
    return out


def case_args(case):
    """the positional arguments of gene_cell_scores"""
    return tuple(case[k] for k in ("pos", "tlen", "cell", "n_cells", "win_lo", "win_hi", "body_lo", "body_hi", "weight", "lower", "upper"))
