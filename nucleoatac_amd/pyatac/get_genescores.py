"""`pyatac genescores`: a gene activity score per cell from a single-cell fragment file and a BED file of genes -- per gene and cell the
sum over the cell's Tn5 insertions around the gene of an integer weight that falls with the distance to the gene body, as a sparse matrix
in the layout of `pyatac cellcounts`.  This command is this package's own, like `cellcounts` and `markers`: the reference has no such tool.
It is the bridge from windows to genes: after `cluster`, `markers --counts BASE.genescores.npz --groups BASE.clusters.tsv` lists the genes
that are more accessible in cluster c3 than elsewhere, by name.  The model is ArchR's gene score (accessibility around a gene weighted by
distance to the gene body and capped at the neighbouring genes); the flat form, fragments in a gene body, is `cellcounts --bed genes.bed`.

Genes.  --genes is a TAB-separated BED: chrom, start, end, a name in column --name and a strand in column --strand (`-` is minus,
anything else plus).  `#` lines and empty lines are skipped; a line with too few fields, end - start < 1 or a name that is empty or longer
than 255 bytes stops the command with `<path>: line <N>: <reason>`.  Names need not be unique; rows stay in file order.  A gene on a
chromosome the fragment file never mentions is an empty row, as in `cellcounts`.

Extended body, with u = --upstream in [0, 2^20]: [bs, be) = [max(0, start - u), end) for a plus gene, [start, end + u) for a minus gene.

Window, with e_min = --min_extend and e_max = --max_extend, 0 <= e_min <= e_max <= 2^20, per chromosome: prev(g) is the largest be_h over
the other genes h with be_h <= bs_g (-infinity if there is none), next(g) the smallest bs_h over the other genes with bs_h >= be_g
(+infinity if none); wl = max(0, max(bs - e_max, min(bs - e_min, prev))) and wh = min(be + e_max, max(be + e_min, next)).  The window
reaches up to e_max on either side, stops at the nearest gene that lies wholly beyond and always reaches at least e_min; genes that
overlap g do not limit it.  --no_boundaries takes prev = -infinity and next = +infinity.  Integer work on the host (gene_windows).

Weights, with D = --decay in [1, 10^7] and U = --unit in [4, 65536]: w[d] = int(numpy.rint(U * (numpy.exp(-d / D) + numpy.exp(-1.0))))
for d = 0 .. e_max, int32, formed once on the host in fp64 (weight_table); every w[d] is at least 1.

Records are read as `cellcounts` reads them (FragmentStore.from_fragments_cells, the --cells table, --header).  A record has l = pos + 4,
ilen = tlen - 8 and r = l + ilen - 1 and counts when lower <= ilen < upper, 0 <= lower < upper <= 50000.  Its two insertions are l and r;
each counts on its own, also when r == l or r == l - 1.

Score.  An insertion x with wl <= x < wh has the distance d = 0 when bs <= x < be, d = bs - x to the left of the body and d = x - be + 1
to the right.  It adds w[d] to entry (gene, cell).  An entry exists where at least one insertion hit; its value is the exact integer sum.
That sum is the device's part (Context.gene_cell_scores, csrc/natac_genescores.hpp; include/natac.h states it): one call per chromosome,
rows of at most 64 hits sorted in the lanes of one wave, every other row summed in a table of per-cell LDS counters.

Not done: gene-length scale factors (a constant per gene, without effect on a per-gene rank test), the 500-base tiles ArchR sums over, a
ceiling per tile, depth normalisation of the written values (`markers` divides by the column sum itself), an expression input,
peak-to-gene links, GTF or GFF parsing.

Files.  BASE.genescores.npz (--format npz; fixed timestamps) has the `cellcounts` layout, so `cluster`, `markers` and `coaccess` take it:
indptr, indices, data int32, shape, barcodes, region_chrom / region_start / region_end (the gene's own BED row), and region_name,
region_minus, window_start, window_end, body_start, body_end and params (upstream, min_extend, max_extend, decay, unit, lower, upper,
boundaries).  --format mtx: BASE.genescores.mtx.gz, .barcodes.tsv and .regions.bed as `cellcounts` writes them.  BASE.genescores.genes.tsv,
always: `name chrom start end strand body_start body_end window_start window_end hits cells total` behind a `#` header, in row order.
BASE.genescores.txt: barcodes listed and seen, data and unassigned lines, records counted and filtered by size, genes, genes with a hit,
hits, entries, the largest entry, the largest column sum and the rows per arm.  Everything is computed before the first file is written.

Measured on the MI355X box (tools/bench_genescores.py, one box, one process, three runs after a warm-up: 10 M fragments in 10,000 cells,
99 MB BGZF, 20,000 genes on 4 chromosomes of 50 Mbp with the default geometry, 90.0 M hits at 4,500 a row, 40.0 M entries): the tagged
read 0.35 s, the eight device calls 0.044 to 0.061 s (uploads, the host's checks, round trips and 320 MB of results included; 6.9 ms
between their first and last kernel), the rows put into BED order 0.18 s more; the restatement of tests/genescores_ref.py on 200 of those
genes 5.04 s on that box, and equal.
"""
import gzip
import os
import time

import numpy as np

MAX_EXTEND = 1 << 20
PARAM_NAMES = ("upstream", "min_extend", "max_extend", "decay", "unit", "lower", "upper", "boundaries")
_FAR = np.int64(1) << 62       # stands for infinity in the window rule: every coordinate is far below it


class GenescoresError(ValueError):
    """an input or a parameter `pyatac genescores` cannot use; one line"""


def check_params(upstream, min_extend, max_extend, decay, unit, lower, upper, name_col=4, strand_col=6):
    if not 0 <= upstream <= MAX_EXTEND:
        raise GenescoresError("--upstream must be in [0, %d] (got %d)" % (MAX_EXTEND, upstream))
    if not 0 <= min_extend <= max_extend <= MAX_EXTEND:
        raise GenescoresError("0 <= --min_extend <= --max_extend <= %d must hold (got %d and %d)" % (MAX_EXTEND, min_extend, max_extend))
    if not 1 <= decay <= 10 ** 7:
        raise GenescoresError("--decay must be in [1, 10000000] (got %d)" % decay)
    if not 4 <= unit <= 65536:
        raise GenescoresError("--unit must be in [4, 65536] (got %d)" % unit)
    if not 0 <= lower < upper <= 50000:
        raise GenescoresError("0 <= --lower < --upper <= 50000 must hold (got %d and %d)" % (lower, upper))
    if name_col < 4 or strand_col < 4 or name_col == strand_col:
        raise GenescoresError("--name and --strand must be two different columns from the 4th on (got %d and %d)" % (name_col, strand_col))


def read_genes(path, name_col=4, strand_col=6):
    """the gene BED -> (chrom_names list of str in order of first appearance, chrom int64 index into it, start int64, end int64,
    names list of str, minus bool), rows in file order; GenescoresError `<path>: line <N>: <reason>` for a line it cannot take"""
    need = max(3, name_col, strand_col)
    chrom_names, where = [], {}
    chrom, start, end, names, minus = [], [], [], [], []
    with open(path, "rb") as f:
        for no, raw in enumerate(f, 1):
            line = raw.rstrip(b"\r\n")
            if not line or line.startswith(b"#"):
                continue
            p = line.split(b"\t")
            if len(p) < need:
                raise GenescoresError("%s: line %d: %d fields, at least %d are needed" % (path, no, len(p), need))
            try:
                s, e = int(p[1]), int(p[2])
            except ValueError:
                raise GenescoresError("%s: line %d: start and end must be integers" % (path, no))
            if s < 0:
                raise GenescoresError("%s: line %d: start %d is negative" % (path, no, s))
            if e - s < 1:
                raise GenescoresError("%s: line %d: end - start is %d, less than 1" % (path, no, e - s))
            if e >= 1 << 40:
                raise GenescoresError("%s: line %d: end %d is 2^40 or more" % (path, no, e))
            name = p[name_col - 1]
            if not name:
                raise GenescoresError("%s: line %d: the name in column %d is empty" % (path, no, name_col))
            if len(name) > 255:
                raise GenescoresError("%s: line %d: the name in column %d has %d bytes, more than 255" % (path, no, name_col, len(name)))
            c = p[0].decode("latin-1")
            if c not in where:
                where[c] = len(chrom_names)
                chrom_names.append(c)
            chrom.append(where[c])
            start.append(s)
            end.append(e)
            names.append(name.decode("latin-1"))
            minus.append(p[strand_col - 1] == b"-")
    return (chrom_names, np.array(chrom, np.int64), np.array(start, np.int64), np.array(end, np.int64), names, np.array(minus, bool))


def gene_windows(chrom, start, end, minus, upstream=5000, min_extend=1000, max_extend=100000, boundaries=True):
    """(body_start, body_end, window_start, window_end), int64 each, by the rule of the module docstring; chrom is any integer label"""
    chrom, start, end = np.asarray(chrom, np.int64), np.asarray(start, np.int64), np.asarray(end, np.int64)
    minus = np.asarray(minus, bool)
    bs = np.where(minus, start, np.maximum(0, start - upstream))
    be = np.where(minus, end + upstream, end)
    prev, nxt = np.full(len(bs), -_FAR), np.full(len(bs), _FAR)
    if boundaries:
        for c in np.unique(chrom):
            idx = np.flatnonzero(chrom == c)
            ends, starts = np.sort(be[idx]), np.sort(bs[idx])
            # be_g > bs_g: a gene never bounds itself, nor does one that overlaps it
            k = np.searchsorted(ends, bs[idx], "right")             # ends[:k] <= bs_g
            prev[idx] = np.where(k > 0, ends[np.maximum(k - 1, 0)], -_FAR)
            k = np.searchsorted(starts, be[idx], "left")            # starts[k:] >= be_g
            nxt[idx] = np.where(k < len(idx), starts[np.minimum(k, len(idx) - 1)], _FAR)
    wl = np.maximum(0, np.maximum(bs - max_extend, np.minimum(bs - min_extend, prev)))
    wh = np.minimum(be + max_extend, np.maximum(be + min_extend, nxt))
    return bs, be, wl, wh


def weight_table(max_extend, decay, unit):
    """w[d] for d = 0 .. max_extend, int32"""
    d = np.arange(int(max_extend) + 1, dtype=np.float64)
    return np.rint(unit * (np.exp(-d / decay) + np.exp(-1.0))).astype(np.int64).astype(np.int32)


def _device_scores(*args, **kw):
    from .. import get_context
    return get_context().gene_cell_scores(*args, **kw)


def gene_scores(store, n_cells, chrom_names, chrom, wl, wh, bs, be, weight, lower, upper, score=None, timing=None):
    """(indptr int64, indices int32, data int32, hits int64[n_genes], arm_rows int64[2]) of the genes, rows in their order, columns the
    cells of the tagged `store`: one call per chromosome that has genes and is in the store.  score(pos, tlen, cell, n_cells, win_lo,
    win_hi, body_lo, body_hi, weight, lower, upper, with_hits=True, with_arm_rows=True, with_kernel_ms=True) -> (indptr, indices, data,
    hits, arm_rows, ms) defaults to Context.gene_cell_scores."""
    t = timing if timing is not None else {}
    t.setdefault("device_s", 0.0)
    t.setdefault("kernel_ms", 0.0)
    n_rows = len(wl)
    row_nnz, hits, arms = np.zeros(n_rows, np.int64), np.zeros(n_rows, np.int64), np.zeros(2, np.int64)
    parts = []
    for k, c in enumerate(chrom_names):
        if c not in store.pos:
            continue                         # the file never mentions it: empty rows
        idx = np.flatnonzero(chrom == k)
        t0 = time.perf_counter()
        ptr, col, val, h, a, ms = (score or _device_scores)(store.pos[c], store.tlen[c], store.cell[c], n_cells, wl[idx], wh[idx], bs[idx],
                                                          be[idx], weight, lower, upper, with_hits=True, with_arm_rows=True,
                                                          with_kernel_ms=True)
        t["device_s"] += time.perf_counter() - t0
        t["kernel_ms"] += ms
        row_nnz[idx] = np.diff(ptr)
        hits[idx] = h
        arms += a
        parts.append((idx, ptr, col, val))
    indptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(row_nnz, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), np.int32)
    data = np.empty(int(indptr[-1]), np.int32)
    for idx, ptr, col, val in parts:         # entry q of the chromosome's row j goes to indptr[idx[j]] + (q - ptr[j])
        dest = np.repeat(indptr[idx] - ptr[:-1], np.diff(ptr)) + np.arange(len(col), dtype=np.int64)
        indices[dest] = col
        data[dest] = val
    return indptr, indices, data, hits, arms


def get_genescores(args, score=None, timing=None):
    """`pyatac genescores`: writes BASE.genescores.npz or .mtx.gz + .barcodes.tsv + .regions.bed, BASE.genescores.genes.tsv and
    BASE.genescores.txt; returns (indptr, indices, data).  Everything is computed before the first file is written, so an error leaves
    nothing behind.  score: the device call (gene_scores), for the tests."""
    from .._lib import NatacError
    from .cellgroups import CellGroupError, read_groups
    from .fragments import FragmentStore
    from .get_cellcounts import mtx_text
    from .get_cluster import _savez_fixed
    name_col, strand_col = getattr(args, "name", 4), getattr(args, "strand", 6)
    boundaries = not getattr(args, "no_boundaries", False)
    check_params(args.upstream, args.min_extend, args.max_extend, args.decay, args.unit, args.lower, args.upper, name_col, strand_col)
    t = timing if timing is not None else {}
    for path in (args.cells, args.genes, args.fragments):
        if not os.path.exists(path):
            raise CellGroupError("%s: no such file" % path)
    if args.out is None:
        args.out = ".".join(os.path.basename(args.genes).split(".")[0:-1])
    barcodes = read_groups(args.cells, header=args.header).barcodes
    chrom_names, chrom, start, end, names, minus = read_genes(args.genes, name_col, strand_col)
    bs, be, wl, wh = gene_windows(chrom, start, end, minus, args.upstream, args.min_extend, args.max_extend, boundaries)
    weight = weight_table(args.max_extend, args.decay, args.unit)
    t0 = time.perf_counter()
    store, bc_count, n_unassigned = FragmentStore.from_fragments_cells(args.fragments, barcodes)
    t["read_s"] = time.perf_counter() - t0
    n_counted = n_sized_out = 0
    for c in store.pos:
        ilen = np.asarray(store.tlen[c], np.int64) - 8
        ok = int(np.count_nonzero((ilen >= args.lower) & (ilen < args.upper)))
        n_counted += ok
        n_sized_out += len(ilen) - ok
    try:
        indptr, indices, data, hits, arms = gene_scores(store, len(barcodes), chrom_names, chrom, wl, wh, bs, be, weight, args.lower, args.upper,
                                                        score=score, timing=t)
    except NatacError as e:
        if "2^31" in str(e):
            raise GenescoresError("%s: lower --unit (now %d)" % (e, args.unit))
        raise
    col_sum = np.bincount(indices, weights=data, minlength=len(barcodes)).astype(np.int64) if len(indices) else np.zeros(len(barcodes), np.int64)
    if len(col_sum) and col_sum.max() >= 1 << 31:
        w = int(np.argmax(col_sum))
        raise GenescoresError("cell %s has a column sum of %d, 2^31 or more, and `markers` needs less: lower --unit (now %d)"
                              % (barcodes[w].decode("latin-1"), col_sum[w], args.unit))
    base = args.out + ".genescores"
    n_genes = len(start)
    region_chrom = np.array(chrom_names, dtype=object)[chrom] if n_genes else np.zeros(0, dtype=object)
    row_cells = np.diff(indptr)
    row_total = np.zeros(n_genes, np.int64)
    if len(data):
        row_total = np.bincount(np.repeat(np.arange(n_genes), row_cells), weights=data, minlength=n_genes).astype(np.int64)
    genes_tsv = ["#name\tchrom\tstart\tend\tstrand\tbody_start\tbody_end\twindow_start\twindow_end\thits\tcells\ttotal\n"]
    for i in range(n_genes):
        genes_tsv.append("%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (names[i], region_chrom[i], start[i], end[i], "-" if minus[i] else "+",
                                                                             bs[i], be[i], wl[i], wh[i], hits[i], row_cells[i], row_total[i]))
    summary = ("barcodes_listed\t%d\nbarcodes_seen\t%d\ndata_lines\t%d\nunassigned_lines\t%d\nrecords_counted\t%d\nrecords_filtered_by_size\t%d\n"
               "genes\t%d\ngenes_with_hit\t%d\nhits\t%d\nentries\t%d\nlargest_entry\t%d\nlargest_column_sum\t%d\nrows_short\t%d\nrows_table\t%d\n"
               % (len(barcodes), int(np.count_nonzero(bc_count)), int(bc_count.sum()) + n_unassigned, n_unassigned, n_counted, n_sized_out,
                  n_genes, int(np.count_nonzero(hits)), int(hits.sum()), len(indices), int(data.max()) if len(data) else 0,
                  int(col_sum.max()) if len(col_sum) else 0, arms[0], arms[1]))
    t0 = time.perf_counter()
    if args.format == "npz":
        _savez_fixed(base + ".npz", indptr=indptr, indices=indices, data=data, shape=np.array([n_genes, len(barcodes)], np.int64),
                     barcodes=np.array(barcodes, dtype="S"), region_chrom=region_chrom.astype("U"), region_start=start, region_end=end,
                     region_name=np.array(names, dtype="U"), region_minus=minus, window_start=wl, window_end=wh, body_start=bs, body_end=be,
                     params=np.array([args.upstream, args.min_extend, args.max_extend, args.decay, args.unit, args.lower, args.upper,
                                      int(boundaries)], np.int64), param_names=np.array(PARAM_NAMES, dtype="U"))
    else:
        text = mtx_text(indptr, indices, data, len(barcodes))
        bed = "".join(["%s\t%d\t%d\n" % r for r in zip(region_chrom.tolist(), start.tolist(), end.tolist())])
        with open(base + ".mtx.gz", "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:      # no name, no time
            f.write(text)
        with open(base + ".barcodes.tsv", "wb") as f:
            f.write(b"".join([b + b"\n" for b in barcodes]))
        with open(base + ".regions.bed", "w") as f:
            f.write(bed)
    with open(base + ".genes.tsv", "w") as f:
        f.write("".join(genes_tsv))
    with open(base + ".txt", "w") as f:
        f.write(summary)
    t["write_s"] = time.perf_counter() - t0
    return indptr, indices, data
