"""The cell-by-region count matrix (natac_region_cell_counts, `pyatac cellcounts`) restated in NumPy from the rule of include/natac.h, not
from the kernels: brute force, every record against every region, then np.unique per row.  And the crafted single-cell fragment file the
CPU and GPU tests of the command share."""
import numpy as np

from cellgroups_ref import crafted
from sites_ref import fragment_ends


def cell_counts_brute(pos, tlen, cell, starts, ends, lower, upper, atac):
    """CSR (indptr int64, indices int32, data int32): rows = regions in the given order, columns ascending within a row"""
    l, ilen, r = fragment_ends(pos, tlen, atac)
    cell = np.asarray(cell, np.int64)
    ok = (ilen >= lower) & (ilen < upper)
    indptr, cols, vals = [0], [], []
    for s, e in zip(starts, ends):
        hit = ok & (((l >= s) & (l < e)) | ((r >= s) & (r < e)))
        c, n = np.unique(cell[hit], return_counts=True)
        cols.append(c)
        vals.append(n)
        indptr.append(indptr[-1] + len(c))
    cat = (lambda x: np.concatenate(x) if x else np.zeros(0))
    return np.array(indptr, np.int64), cat(cols).astype(np.int32), cat(vals).astype(np.int32)


def cell_counts_ref(pos, tlen, cell, n_cells, starts, ends, lower, upper, atac):
    """the same matrix for many regions: per region only the records whose left end lies within upper + |lower| + 16 of it (pos is sorted)
    are tested, all (region, record) pairs at once, and one np.unique over region * n_cells + cell gives the entries"""
    l, ilen, r = fragment_ends(pos, tlen, atac)
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    ok = (ilen >= lower) & (ilen < upper)
    margin = abs(int(upper)) + abs(int(lower)) + 16
    a = np.searchsorted(l, starts - margin, "left")
    n = np.maximum(np.searchsorted(l, ends + margin, "right") - a, 0)
    row = np.repeat(np.arange(len(starts), dtype=np.int64), n)
    rec = np.repeat(a - (np.cumsum(n) - n), n) + np.arange(int(n.sum()), dtype=np.int64)
    s, e = starts[row], ends[row]
    hit = ok[rec] & (((l[rec] >= s) & (l[rec] < e)) | ((r[rec] >= s) & (r[rec] < e)))
    key, val = np.unique(row[hit] * int(n_cells) + np.asarray(cell, np.int64)[rec[hit]], return_counts=True)
    indptr = np.zeros(len(starts) + 1, np.int64)
    np.cumsum(np.bincount(key // int(n_cells), minlength=len(starts)), out=indptr[1:])
    return indptr, (key % int(n_cells)).astype(np.int32), val.astype(np.int32)


def row_sums(indptr, data):
    return np.array([int(np.asarray(data[a:b], np.int64).sum()) for a, b in zip(indptr[:-1], indptr[1:])], np.int64)


def assert_same_csr(got, want):
    for g, w, name in zip(got, want, ("indptr", "indices", "data")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def crafted_cells(seed=11):
    """-> (text, barcodes): ~3,000 lines on three chromosomes of which chr1 comes back (plus one on which nothing is listed), a 10x '#'
    header, 40 cell barcodes of which the 30 in `barcodes` are listed, CRLF lines, duplicate lines, and -- put in by hand right behind the
    header -- a line with an empty barcode, one with a 256-byte barcode, one with end == start and a CRLF line, all on chr1"""
    text, listed = crafted(seed=seed)
    barcodes = listed[:30]
    head, nl, rest = text.partition(b"\n")
    extra = [b"chr1\t1000\t1200\t\n", b"chr1\t1000\t1200\t" + b"Q" * 256 + b"\n", b"chr1\t5000\t5000\t" + barcodes[3] + b"\n",
             b"chr1\t5001\t5100\t" + barcodes[4] + b"\r\n", b"chr1\t5001\t5100\t" + barcodes[4] + b"\r\n"]
    return head + nl + b"".join(extra) + rest, barcodes


def crafted_windows(with_missing=True):
    """BED text over the crafted file's chromosomes: tiles of chr1, overlapping and repeated windows on chr2 and chr3_random in mixed order,
    a zero-length row (dropped), one window over all of chr1, and (with_missing) one on a chromosome the file never mentions"""
    rows = [("chr2", 0, 2_000_000), ("chr1", 4990, 5010)]
    rows += [("chr1", s, s + 40_000) for s in range(0, 2_000_000, 40_000)]
    rows += [("chr3_random", s, s + 150_000) for s in range(1_900_000, -1, -100_000)]
    rows += [("chr2", 300, 301), ("chr2", 100, 100), ("chr2", 290, 1000), ("chr2", 290, 1000), ("chr1", 0, 2_100_000)]
    if with_missing:
        rows.insert(7, ("chrNowhere", 10, 500))
    rows += [("chrOnlyUnassigned", 0, 2_000_000)]
    return "".join("%s\t%d\t%d\n" % r for r in rows).encode()
