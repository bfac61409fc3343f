"""The cells rule of include/natac.h (natac_frag_cells) written out a second time, from the rule's text alone, for VALID files: a dict in
line order over the text.  Nothing here imports the package; the crafted single-cell text is the split's (tests/cellgroups_ref.py)."""
import re

import numpy as np

from cellgroups_ref import crafted, every_barcode      # noqa: F401 -- the tests of the cells rule take them from here

_DATA = re.compile(rb"([^\t]+)\t([0-9]+)\t([0-9]+)\t([^\t]*)(?:\t.*)?\Z", re.S)      # chrom, start, end, barcode, anything


def cells_ref(text, nfr_upper=147, mono_upper=294):
    """-> dict(barcodes (order of first appearance), n_frag, n_nfr, n_mono (int64), n_data, n_unassigned)"""
    assert 0 < nfr_upper < mono_upper
    body, nl, tail = text.rpartition(b"\n")
    lines = [x[:-1] if x.endswith(b"\r") else x for x in body.split(b"\n")] if nl else []      # (only a line that HAD its '\n' loses a '\r')
    if tail:
        lines.append(tail)
    cells = {}                                         # barcode -> [n_frag, n_nfr, n_mono]; a dict keeps the order of first insertion
    n_data = n_unassigned = 0
    for line in lines:
        if line == b"" or line.startswith(b"#"):
            continue
        m = _DATA.match(line)
        assert m, line
        start, end, bc = int(m.group(2)), int(m.group(3)), m.group(4)
        assert start <= end <= 2 ** 31 - 1
        n_data += 1
        if not 1 <= len(bc) <= 255:
            n_unassigned += 1
            continue
        c = cells.setdefault(bc, [0, 0, 0])
        c[0] += 1
        if end - start < nfr_upper:
            c[1] += 1
        elif end - start < mono_upper:
            c[2] += 1
    counts = np.array(list(cells.values()), dtype=np.int64).reshape(-1, 3)
    return dict(barcodes=list(cells), n_frag=counts[:, 0], n_nfr=counts[:, 1], n_mono=counts[:, 2], n_data=n_data, n_unassigned=n_unassigned)


def assert_table_equals_ref(table, ref):
    """table: a CellTable of FragmentStore.discover_cells*"""
    assert table.barcodes == ref["barcodes"]
    for name in ("n_frag", "n_nfr", "n_mono"):
        got = getattr(table, name)
        assert got.dtype == np.int64 and np.array_equal(got, ref[name]), name
    assert (table.n_data, table.n_unassigned) == (ref["n_data"], ref["n_unassigned"])
    assert int(table.n_frag.sum()) + table.n_unassigned == table.n_data


def assert_same_table(a, b):
    assert a.barcodes == b.barcodes and (a.n_data, a.n_unassigned) == (b.n_data, b.n_unassigned)
    for name in ("n_frag", "n_nfr", "n_mono"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
