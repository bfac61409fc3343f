"""`pyatac deviations`: per-cell motif accessibility deviations and z-scores from the cell-by-window count matrix of `pyatac cellcounts` and
the window-by-motif hit matrix of `pyatac motifs`.  This command is this package's own, like `cluster` and `motifs`: the reference has no
such tool.  It answers, after clustering, which factors' sites are more or less accessible in which cells and clusters (the analysis
chromVAR made usual), with fixed rules so that the result is a function of the inputs and the seed.

Inputs.  X is the windows x cells count matrix (get_cluster.read_counts), H the windows x motifs hit matrix; both files carry their
regions, and the two lists must be equal row for row in chrom, start and end.  Window p is annotated with motif m when H[p, m] > 0.
Windows with row sum 0 and cells with column sum 0 are dropped, then motifs left with no annotated live window (`NA` in the outputs).
P windows and N cells stay; rs[p] is a row sum, d[c] a column sum, T the total, and T < 2^31 is required.

GC content.  gc[p] = (C + G) / (A + C + G + T) of the window's bases in the FASTA, case ignored (Context.base_counts(per_range=True)), 0.5
for a window with no such base.

Background table (host, NumPy, integers out).  From n_g = --gc_bins and n_a = --acc_bins: while P // (n_g * n_a) < --min_bin and
n_g * n_a > 1 the larger of the two is lowered by 1, n_a on a tie.  The windows ranked by (gc, index) are cut into GC bins, bin k the ranks
[floor(k P / n_g), floor((k + 1) P / n_g)); inside each GC bin the windows ranked by (rs, index) are cut into n_a parts in the same way.  A
window's candidates are the windows of its cell of that grid, itself included, in ascending index order.  With
r = numpy.random.default_rng(seed).random((B, P)), B = --iterations in [2, 1024]: bg[b][p] = candidates(p)[int(r[b - 1, p] *
len(candidates(p)))] for b = 1 .. B; bg[0] is the identity.

Device (Context.motif_deviations, csrc/natac_deviations.hpp; include/natac.h states it).  For b = 0 .. B, motif m and cell c the exact
integers O_b[m, c] = sum over the annotated p of X[bg[b][p], c] and E_b[m] = sum over the annotated p of rs[bg[b][p]]; then in fp64, one
rounded operation at a time, x = E_b[m] * d[c] / T, Y_b = (O_b[m, c] - x) / x, raw = Y_0, and Welford's recurrence over Y_1 .. Y_B in
order, which gives bg_mean and bg_m2.  That is the hot path: (B + 1) gathers of every motif's rows of X.

Host.  sd = sqrt(bg_m2 / (B - 1)), deviation = raw - bg_mean, z = deviation / sd or NaN where sd == 0.  A motif's variability is the
standard deviation (n - 1) of z over the cells whose z is finite (NA with fewer than two).  With --groups (the table `cluster` writes): the
mean z per group and motif over that group's cells that are in the matrix and whose z is finite.

Not done here: bootstrap intervals, k-mer or peak-set annotations other than the motif matrix, the density-weighted background sampling of
chromVAR, a differential test.

Measured on the MI355X box (tools/bench_deviations.py, one box, one process, three runs after a warm-up: 10,000 cells x 100,000 windows,
3.19 M entries, 500 motifs with 4.57 M hits, B = 50; 7.44e9 gathered entries): the device call 0.28 s (the sort of the hits by motif, the host's checks
and row split, uploads and 120 MB of results included; 36.2 ms in the kernel); the same result through scipy.sparse products and NumPy on
that box 32.9 s, the fp64 outputs the same bytes.
"""
import gzip
import os
import zipfile

import numpy as np

from .get_cluster import ClusterError, _savez_fixed, read_counts

MAX_B = 1024            # NATAC_DEVIATIONS_MAX_B


class DeviationsError(ValueError):
    """an input or a parameter `pyatac deviations` cannot use; one line"""


def _regions_npz(z, path):
    for k in ("region_chrom", "region_start", "region_end"):
        if k not in z.files:
            raise DeviationsError("%s: no array %r: the file carries no regions" % (path, k))
    return [str(c) for c in z["region_chrom"].tolist()], z["region_start"].astype(np.int64), z["region_end"].astype(np.int64)


def _regions_bed(path):
    if not os.path.exists(path):
        raise DeviationsError("%s: no such file" % path)
    chrom, start, end = [], [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            p = line.rstrip("\n").split("\t")
            try:
                chrom.append(p[0])
                start.append(int(p[1]))
                end.append(int(p[2]))
            except (IndexError, ValueError):
                raise DeviationsError("%s: line %d: expected chrom, start and end" % (path, no))
    return chrom, np.array(start, np.int64), np.array(end, np.int64)


def read_regions(path):
    """the regions either output of `cellcounts` or `motifs` carries -> (chrom list of str, start int64, end int64)"""
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return _regions_npz(z, path)
    return _regions_bed(path[:-len(".mtx.gz")] + ".regions.bed")


def read_hits(path):
    """either output of `pyatac motifs` -> (indptr int64, indices int32, data int32, ids, alts): CSR with one row per window, the motifs
    ascending within a row.  BASE.motifs.mtx.gz comes with BASE.motifs.names.tsv beside it."""
    if not os.path.exists(path):
        raise DeviationsError("%s: no such file" % path)
    if path.endswith(".npz"):
        try:
            z = np.load(path, allow_pickle=False)
        except (ValueError, OSError, EOFError, zipfile.BadZipFile):
            raise DeviationsError("%s: not a motifs .npz" % path)
        with z:
            for k in ("indptr", "indices", "data", "shape", "motifs"):
                if k not in z.files:
                    raise DeviationsError("%s: no array %r: not a motifs .npz" % (path, k))
            indptr, indices, data = z["indptr"].astype(np.int64), z["indices"].astype(np.int32), z["data"].astype(np.int32)
            ids = [b.decode("latin-1") for b in z["motifs"].tolist()]
            alts = [str(a) for a in z["alts"].tolist()] if "alts" in z.files else [""] * len(ids)
            n_rows, n_cols = (int(v) for v in z["shape"])
        if len(indptr) != n_rows + 1 or len(ids) != n_cols or len(alts) != n_cols:
            raise DeviationsError("%s: the arrays do not have the shape the file states" % path)
        return indptr, indices, data, ids, alts
    if not path.endswith(".mtx.gz"):
        raise DeviationsError("%s: expected a .motifs.npz or a .motifs.mtx.gz" % path)
    side = path[:-len(".mtx.gz")] + ".names.tsv"
    if not os.path.exists(side):
        raise DeviationsError("%s: no such file" % side)
    with open(side) as f:
        names = [line.rstrip("\n").split("\t") for line in f if line.rstrip("\n")]
    ids, alts = [n[0] for n in names], [n[1] if len(n) > 1 else "" for n in names]
    with gzip.open(path, "rb") as f:
        text = f.read()
    head, _, rest = text.partition(b"\n")
    if not head.startswith(b"%%MatrixMarket matrix coordinate"):
        raise DeviationsError("%s: not a MatrixMarket coordinate file" % path)
    while rest[:1] == b"%":
        rest = rest.partition(b"\n")[2]
    dims, _, body = rest.partition(b"\n")
    try:
        n_rows, n_cols, nnz = (int(v) for v in dims.split())
        trip = np.array(body.split(), dtype=np.int64).reshape(-1, 3)
    except ValueError:
        raise DeviationsError("%s: malformed MatrixMarket text" % path)
    if len(trip) != nnz or n_cols != len(ids):
        raise DeviationsError("%s: %d entries and %d columns stated, %d entries and %d names found" % (path, nnz, n_cols, len(trip), len(ids)))
    if nnz and (trip[:, 0].min() < 1 or trip[:, 0].max() > n_rows or trip[:, 1].min() < 1 or trip[:, 1].max() > n_cols):
        raise DeviationsError("%s: an entry lies outside the %d x %d matrix" % (path, n_rows, n_cols))
    trip = trip[np.lexsort((trip[:, 1], trip[:, 0]))]
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(trip[:, 0] - 1, minlength=n_rows), out=indptr[1:])
    return indptr, (trip[:, 1] - 1).astype(np.int32), trip[:, 2].astype(np.int32), ids, alts


def check_regions(a, b, path_a, path_b):
    """DeviationsError naming the first row at which the two region lists differ"""
    (ca, sa, ea), (cb, sb, eb) = a, b
    n = min(len(ca), len(cb))
    diff = np.flatnonzero((np.array(ca[:n], dtype=object) != np.array(cb[:n], dtype=object)) | (sa[:n] != sb[:n]) | (ea[:n] != eb[:n]))
    if len(diff) or len(ca) != len(cb):
        i = int(diff[0]) if len(diff) else n
        show = lambda c, s, e: "%s:%d-%d" % (c[i], s[i], e[i]) if i < len(c) else "no such row"      # noqa: E731
        raise DeviationsError("the regions of %s and %s differ at row %d (%s against %s): give `cellcounts` and `motifs` the same BED"
                              % (path_a, path_b, i + 1, show(ca, sa, ea), show(cb, sb, eb)))


def check_params(iterations, gc_bins, acc_bins, min_bin):
    if not 2 <= iterations <= MAX_B:
        raise DeviationsError("--iterations must be in [2, %d] (got %d)" % (MAX_B, iterations))
    if gc_bins < 1 or acc_bins < 1 or min_bin < 1:
        raise DeviationsError("--gc_bins, --acc_bins and --min_bin must be at least 1 (got %d, %d, %d)" % (gc_bins, acc_bins, min_bin))


def grid_shape(P, gc_bins, acc_bins, min_bin):
    """(n_g, n_a) after the reduction of the module docstring"""
    n_g, n_a = int(gc_bins), int(acc_bins)
    while P // (n_g * n_a) < min_bin and n_g * n_a > 1:
        if n_g > n_a:
            n_g -= 1
        else:
            n_a -= 1
    return n_g, n_a


def grid_cells(gc, rs, n_g, n_a):
    """int64[P]: the cell k * n_a + j of the GC x accessibility grid every window lies in"""
    P = len(gc)
    idx = np.arange(P, dtype=np.int64)
    by_gc = np.lexsort((idx, gc))
    g_edge = (np.arange(n_g + 1, dtype=np.int64) * P) // n_g
    cell = np.empty(P, np.int64)
    for k in range(n_g):
        members = by_gc[g_edge[k]:g_edge[k + 1]]
        by_rs = members[np.lexsort((members, rs[members]))]
        a_edge = (np.arange(n_a + 1, dtype=np.int64) * len(members)) // n_a
        for j in range(n_a):
            cell[by_rs[a_edge[j]:a_edge[j + 1]]] = k * n_a + j
    return cell


def background_table(gc, rs, iterations, gc_bins=25, acc_bins=25, min_bin=10, seed=1):
    """(bg int32[B, P], (n_g, n_a), (smallest, largest cell of the grid)) by the rule of the module docstring"""
    P = len(gc)
    n_g, n_a = grid_shape(P, gc_bins, acc_bins, min_bin)
    cell = grid_cells(np.asarray(gc, np.float64), np.asarray(rs, np.int64), n_g, n_a)
    order = np.argsort(cell, kind="stable")                 # by (cell, index): every cell's windows in ascending index order
    size = np.bincount(cell, minlength=n_g * n_a)
    first = np.zeros(n_g * n_a + 1, np.int64)
    np.cumsum(size, out=first[1:])
    r = np.random.default_rng(seed).random((iterations, P))
    pick = (r * size[cell][None, :].astype(np.float64)).astype(np.int64)
    bg = order[first[cell][None, :] + pick].astype(np.int32)
    return bg, (n_g, n_a), (int(size.min()), int(size.max()))


def _device_deviations(*args, **kw):
    from .. import get_context
    return get_context().motif_deviations(*args, **kw)


def _device_base_counts(seq, starts, ends):
    from .. import get_context
    return get_context().base_counts(seq, starts, ends, per_range=True)


def gc_from_counts(acgt):
    """gc = (C + G) / (A + C + G + T) per row of int64[n, 4]; 0.5 where the row is empty"""
    acgt = np.asarray(acgt, np.int64)
    tot = acgt.sum(axis=1)
    gc = np.full(len(acgt), 0.5, np.float64)
    ok = tot > 0
    gc[ok] = (acgt[ok, 1] + acgt[ok, 2]).astype(np.float64) / tot[ok].astype(np.float64)
    return gc


def window_gc(fasta_path, chrom, start, end, base_counts=None):
    """gc of every window from the FASTA, one per-range base count per chromosome"""
    from .seq import FastaStore
    if not os.path.exists(fasta_path):
        raise DeviationsError("%s: no such file" % fasta_path)
    fasta = FastaStore.open(fasta_path)
    chrom = np.array(chrom, dtype=object)
    acgt = np.zeros((len(start), 4), np.int64)
    for c in sorted(set(chrom.tolist())):
        idx = np.flatnonzero(chrom == c)
        if c not in fasta.seqs:
            raise DeviationsError("%s: no chromosome %s (window %s:%d-%d)" % (fasta_path, c, c, start[idx[0]], end[idx[0]]))
        seq = fasta.seqs[c]
        bad = np.flatnonzero((start[idx] < 0) | (end[idx] > len(seq)) | (end[idx] < start[idx]))
        if len(bad):
            i = idx[bad[0]]
            raise DeviationsError("%s: the window %s:%d-%d reaches past the chromosome (%d bases)" % (fasta_path, c, start[i], end[i], len(seq)))
        acgt[idx] = (base_counts or _device_base_counts)(seq, start[idx], end[idx])
    return gc_from_counts(acgt)


def _take_rows(indptr, indices, data, rows):
    """the CSR rows `rows` (ascending) of a CSR matrix"""
    n = np.diff(indptr)[rows]
    ptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(n, out=ptr[1:])
    src = np.repeat(indptr[:-1][rows] - ptr[:-1], n) + np.arange(int(ptr[-1]), dtype=np.int64)
    return ptr, indices[src], data[src]


def motif_deviations(indptr, indices, data, n_cells, h_indptr, h_indices, h_data, n_motifs, gc_of, iterations=50, gc_bins=25, acc_bins=25,
                     min_bin=10, seed=1, device=None):
    """the computation of `pyatac deviations` on CSR arrays -> dict.  gc_of(kept window indices) -> gc float64 of those windows.
    device(indptr, indices, data, n_cells, hit_indptr, hit_indices, n_motifs, bg) -> (raw, bg_mean, bg_m2) defaults to
    Context.motif_deviations."""
    check_params(iterations, gc_bins, acc_bins, min_bin)
    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(data, np.int64)
    n_win = len(indptr) - 1
    if len(h_indptr) - 1 != n_win:
        raise DeviationsError("the count matrix has %d windows, the motif matrix %d" % (n_win, len(h_indptr) - 1))
    row_of = np.repeat(np.arange(n_win, dtype=np.int64), np.diff(indptr))
    rs_all = np.zeros(n_win, np.int64)
    np.add.at(rs_all, row_of, data)
    d_all = np.zeros(n_cells, np.int64)
    np.add.at(d_all, indices, data)
    win_keep, cell_keep = rs_all > 0, d_all > 0
    wins, cells = np.flatnonzero(win_keep), np.flatnonzero(cell_keep)
    P, N = len(wins), len(cells)
    if P == 0 or N == 0:
        raise DeviationsError("no window or no cell with a count is left")
    T = int(rs_all.sum())
    if T >= 1 << 31:
        raise DeviationsError("the counts add up to %d, 2^31 or more" % T)
    # the live matrix: zero entries go, windows and cells are renumbered
    pos = data > 0
    ptr_pos = np.zeros(n_win + 1, np.int64)
    np.cumsum(np.bincount(row_of[pos], minlength=n_win), out=ptr_pos[1:])
    new_cell = np.cumsum(cell_keep) - 1
    x_ptr, x_idx, x_val = _take_rows(ptr_pos, new_cell[indices[pos]], data[pos], wins)
    # the live annotation
    h_indptr, h_indices, h_data = np.asarray(h_indptr, np.int64), np.asarray(h_indices, np.int64), np.asarray(h_data, np.int64)
    h_row = np.repeat(np.arange(n_win, dtype=np.int64), np.diff(h_indptr))
    live = (h_data > 0) & win_keep[h_row]
    annotated = np.bincount(h_indices[live], minlength=n_motifs)
    motif_keep = annotated > 0
    motifs = np.flatnonzero(motif_keep)
    M = len(motifs)
    if M == 0:
        raise DeviationsError("no motif with an annotated window is left")
    new_motif = np.cumsum(motif_keep) - 1
    new_win = np.cumsum(win_keep) - 1
    hp = np.zeros(P + 1, np.int64)
    np.cumsum(np.bincount(new_win[h_row[live]], minlength=P), out=hp[1:])
    hx = new_motif[h_indices[live]]
    rs, d = rs_all[wins], d_all[cells]
    gc = np.asarray(gc_of(wins), np.float64)
    bg, grid, extremes = background_table(gc, rs, iterations, gc_bins, acc_bins, min_bin, seed)
    raw, bg_mean, bg_m2 = (device or _device_deviations)(x_ptr, x_idx.astype(np.int32), x_val.astype(np.int32), N, hp, hx, M, bg)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(bg_m2 / float(iterations - 1))
        dev = raw - bg_mean
        z = np.where(sd == 0, np.nan, dev / sd)
    variability = np.full(M, np.nan)
    for k in range(M):
        zk = z[k][np.isfinite(z[k])]
        if len(zk) >= 2:
            variability[k] = np.std(zk, ddof=1)
    return dict(win_keep=win_keep, cell_keep=cell_keep, motif_keep=motif_keep, annotated=annotated[motifs], gc=gc, rs=rs, d=d, T=T, bg=bg,
                grid=grid, grid_extremes=extremes, raw=raw, bg_mean=bg_mean, bg_m2=bg_m2, deviations=dev, z=z, variability=variability)


def group_means(z, kept_barcodes, groups):
    """(names, float64[M, n_groups]): the mean z per group and motif over the group's cells in the matrix whose z is finite; NaN without one"""
    where = {bc: k for k, bc in enumerate(kept_barcodes)}
    out = np.full((z.shape[0], len(groups.names)), np.nan)
    for g in range(len(groups.names)):
        cols = [where[bc] for bc, gg in zip(groups.barcodes, groups.group_of) if gg == g and bc in where]
        if not cols:
            continue
        zg = z[:, sorted(cols)]
        for k in range(z.shape[0]):
            zk = zg[k][np.isfinite(zg[k])]
            if len(zk):
                out[k, g] = zk.sum() / len(zk)
    return groups.names, out


def default_base(counts):
    base = os.path.basename(str(counts))
    for suf in (".cellcounts.npz", ".cellcounts.mtx.gz", ".npz", ".mtx.gz"):
        if base.endswith(suf):
            return base[:-len(suf)]
    return base


def output_texts(res, ids, alts, iterations, seed, n_windows, n_cells, groups_table=None):
    """(variability.tsv, groups.tsv or None, summary) as text, and the full-size arrays of the .npz"""
    M_all = len(ids)
    kept = np.flatnonzero(res["motif_keep"])
    N = res["z"].shape[1]
    full = lambda a: _spread(a, kept, M_all)                 # noqa: E731
    var_all, win_all = full(res["variability"]), np.zeros(M_all, np.int64)
    win_all[kept] = res["annotated"]
    ranked = sorted((k for k in range(M_all) if np.isfinite(var_all[k])), key=lambda k: (-var_all[k], k))
    unranked = [k for k in range(M_all) if not np.isfinite(var_all[k])]
    lines = ["id\talt\twindows\tvariability\trank\n"]
    for rank, k in enumerate(ranked, 1):
        lines.append("%s\t%s\t%d\t%.6f\t%d\n" % (ids[k], alts[k], win_all[k], var_all[k], rank))
    for k in unranked:
        lines.append("%s\t%s\t%d\tNA\tNA\n" % (ids[k], alts[k], win_all[k]))
    groups_text = None
    if groups_table is not None:
        names, means = groups_table
        means = full(means)
        rows = ["id\t%s\n" % "\t".join(names)]
        for k in range(M_all):
            rows.append("%s\t%s\n" % (ids[k], "\t".join("NA" if not np.isfinite(v) else "%.4f" % v for v in means[k])))
        groups_text = "".join(rows)
    summary = ("windows_listed\t%d\nwindows_kept\t%d\nwindows_dropped\t%d\ncells_listed\t%d\ncells_kept\t%d\ncells_dropped\t%d\n"
               "motifs_kept\t%d\nmotifs_dropped\t%d\niterations\t%d\ngc_bins\t%d\nacc_bins\t%d\nsmallest_bin\t%d\nlargest_bin\t%d\nseed\t%d\n"
               % (n_windows, int(res["win_keep"].sum()), n_windows - int(res["win_keep"].sum()), n_cells, N, n_cells - N, len(kept),
                  M_all - len(kept), iterations, res["grid"][0], res["grid"][1], res["grid_extremes"][0], res["grid_extremes"][1], seed))
    arrays = dict(deviations=full(res["deviations"]), z=full(res["z"]), variability=var_all, windows_annotated=win_all)
    return "".join(lines), groups_text, summary, arrays


def _spread(a, kept, M_all):
    out = np.full((M_all,) + a.shape[1:], np.nan)
    out[kept] = a
    return out


def get_deviations(args, device=None, base_counts=None):
    """`pyatac deviations`: writes BASE.deviations.npz, .variability.tsv, .txt and, with --groups, .groups.tsv; returns their paths.
    Everything is computed before the first file is written, so an error leaves nothing behind.  device / base_counts: the two device
    calls (motif_deviations, window_gc), for the tests."""
    from .cellgroups import read_groups
    check_params(args.iterations, args.gc_bins, args.acc_bins, args.min_bin)
    for path in (args.counts, args.motifs, args.fasta, args.groups):
        if path is not None and not os.path.exists(path):
            raise DeviationsError("%s: no such file" % path)
    try:
        indptr, indices, data, barcodes = read_counts(args.counts)
    except ClusterError as e:
        raise DeviationsError(str(e))
    h_indptr, h_indices, h_data, ids, alts = read_hits(args.motifs)
    reg_x, reg_h = read_regions(args.counts), read_regions(args.motifs)
    check_regions(reg_x, reg_h, args.counts, args.motifs)
    chrom, start, end = reg_x
    if len(start) != len(indptr) - 1:
        raise DeviationsError("%s: %d regions for %d rows" % (args.counts, len(start), len(indptr) - 1))
    groups = read_groups(args.groups, header=args.header) if args.groups else None
    chrom_arr = np.array(chrom, dtype=object)
    gc_of = lambda wins: window_gc(args.fasta, chrom_arr[wins], start[wins], end[wins], base_counts=base_counts)     # noqa: E731
    res = motif_deviations(indptr, indices, data, len(barcodes), h_indptr, h_indices, h_data, len(ids), gc_of, args.iterations, args.gc_bins,
                           args.acc_bins, args.min_bin, args.seed, device=device)
    kept_barcodes = [barcodes[c] for c in np.flatnonzero(res["cell_keep"]).tolist()]
    table = group_means(res["z"], kept_barcodes, groups) if groups is not None else None
    var_text, groups_text, summary, arrays = output_texts(res, ids, alts, args.iterations, args.seed, len(indptr) - 1, len(barcodes), table)
    base = (args.out if args.out else default_base(args.counts)) + ".deviations"
    paths = [base + ".npz", base + ".variability.tsv", base + ".txt"]
    _savez_fixed(paths[0], motifs=np.array([i.encode("latin-1") for i in ids], dtype="S"), barcodes=np.array(kept_barcodes, dtype="S"), **arrays)
    with open(paths[1], "w") as f:
        f.write(var_text)
    with open(paths[2], "w") as f:
        f.write(summary)
    if groups_text is not None:
        paths.append(base + ".groups.tsv")
        with open(paths[-1], "w") as f:
            f.write(groups_text)
    return paths
