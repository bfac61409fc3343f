"""The split rule of include/natac.h (natac_frag_split) written out a second time, from the rule's text alone, for VALID files; and the crafted
single-cell fragment text the CPU and GPU tests of the split share.  Nothing here imports the package."""
import re

import numpy as np

_DATA = re.compile(rb"([^\t]+)\t([0-9]+)\t([0-9]+)\t([^\t]*)(?:\t.*)?\Z", re.S)      # chrom, start, end, barcode, anything


def split_ref(text, barcodes, group_of, n_groups):
    """-> dict(names, lengths, pos[g][chrom], tlen[g][chrom] (sorted by pos, ties in file order), bc_count, n_unassigned, n_data)"""
    body, nl, tail = text.rpartition(b"\n")
    lines = [x[:-1] if x.endswith(b"\r") else x for x in body.split(b"\n")] if nl else []      # (only a line that HAD its '\n' loses a '\r')
    if tail:
        lines.append(tail)
    listed = {}
    for k, b in enumerate(barcodes):
        assert 1 <= len(b) <= 255 and b not in listed
        listed[b] = k
    names, length = [], {}
    recs = [dict() for _ in range(n_groups)]
    bc_count = np.zeros(len(barcodes), dtype=np.int64)
    n_unassigned = n_data = 0
    for line in lines:
        if line == b"" or line.startswith(b"#"):
            continue
        m = _DATA.match(line)
        assert m, line
        chrom, start, end, bc = m.group(1).decode(), int(m.group(2)), int(m.group(3)), m.group(4)
        assert start <= end <= 2 ** 31 - 1
        n_data += 1
        if chrom not in length:
            names.append(chrom)
            length[chrom] = 0
        length[chrom] = max(length[chrom], end)
        k = listed.get(bc) if 1 <= len(bc) <= 255 else None
        if k is None:
            n_unassigned += 1
            continue
        bc_count[k] += 1
        recs[group_of[k]].setdefault(chrom, []).append((start - 4, end - start + 8))
    pos, tlen = [], []
    for g in range(n_groups):
        by = {c: sorted(recs[g].get(c, []), key=lambda r: r[0]) for c in names}        # sorted() is stable
        pos.append({c: np.array([r[0] for r in by[c]], dtype=np.int64) for c in names})
        tlen.append({c: np.array([r[1] for r in by[c]], dtype=np.int64) for c in names})
    return dict(names=names, lengths=[length[c] for c in names], pos=pos, tlen=tlen, bc_count=bc_count, n_unassigned=n_unassigned, n_data=n_data)


def assert_split_equals_ref(got, ref):
    """got = (stores, bc_count, n_unassigned) of FragmentStore.split_fragments*"""
    stores, bc_count, n_unassigned = got
    assert len(stores) == len(ref["pos"])
    for g, st in enumerate(stores):
        assert st.references == ref["names"] and list(st.lengths) == ref["lengths"], g
        for c in ref["names"]:
            assert st.pos[c].dtype == np.int64 and np.array_equal(st.pos[c], ref["pos"][g][c]), (g, c)
            assert np.array_equal(st.tlen[c], ref["tlen"][g][c]), (g, c)
    assert np.asarray(bc_count).dtype == np.int64 and np.array_equal(bc_count, ref["bc_count"])
    assert n_unassigned == ref["n_unassigned"]
    assert sum(len(st.pos[c]) for st in stores for c in st.references) + n_unassigned == ref["n_data"]


def assert_same_split(a, b):
    for x, y in zip(a[0], b[0]):
        assert x.references == y.references and list(x.lengths) == list(y.lengths)
        for c in x.references:
            assert np.array_equal(x.pos[c], y.pos[c]) and np.array_equal(x.tlen[c], y.tlen[c]), c
    assert len(a[0]) == len(b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _bc(rng):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 16)) + b"-1"


NEVER = b"GGGGGGGGGGGGGGGG-1"          # listed, on no line of the crafted file
TWIN_A, TWIN_B = b"TTTTGGGGCCCCAAAA-1", b"TTTTGGGGCCCCAAAA-2"      # differ in the last byte only
HASHED = b"ACGTAC#TACGTAC-1"           # a '#' inside a barcode is a byte like any other
LONGEST = b"Q" * 255                   # the longest barcode a table can hold; the file also has b"Q" * 256


def crafted(seed=0, n=3000, n_cells=40):
    """-> (text, listed): ~n lines of every clause of the split rule (tests/test_cellgroups_host.py lists them)"""
    rng = np.random.default_rng(seed)
    cells = [_bc(rng) for _ in range(n_cells)]
    listed = cells[:n_cells * 3 // 4] + [NEVER, TWIN_A, TWIN_B, HASHED, LONGEST]
    unlisted = cells[n_cells * 3 // 4:]                               # the same length as the listed ones
    odd = [b"", b"Q" * 256, listed[0][:-1], listed[0] + b"X", listed[1][1:], b" " + listed[2], listed[3].lower()]
    pool = listed[:n_cells * 3 // 4] + [TWIN_A, TWIN_B, HASHED, LONGEST] + unlisted + odd
    weight = np.array([4.0] * (len(pool) - len(odd) - len(unlisted)) + [2.0] * len(unlisted) + [1.0] * len(odd))
    out = [b"# id=crafted\n", b"#\tprimary_contig=chr1\n", b"\n"]

    def stretch(chrom, count, sort=True, only=None):
        start = rng.integers(0, 2_000_000, count)
        if sort:
            start = np.sort(start)
        end = start + rng.integers(0, 900, count)
        for i in range(count):
            bc = (only or pool)[int(rng.choice(len(only or pool), p=None if only else weight / weight.sum()))]
            kind = int(rng.integers(0, 16))
            line = b"%s\t%d\t%d\t%s" % (chrom, start[i], end[i], bc)
            if kind % 2:
                line += b"\t%d" % int(rng.integers(1, 9))            # the fifth column
            out.append(line + (b"\r\n" if kind in (4, 5) else b"\n"))     # CRLF: kind 4 directly behind a 4-field barcode
            if kind == 6:
                out.append(out[-1])                                   # a duplicate line
            if kind == 7:
                out.append((b"\n", b"# note %d\n" % i, b"\r\n")[i % 3])
    stretch(b"chr1", n // 3)
    stretch(b"chr2", n // 6, sort=False)
    # equal starts, different ends, one cell (so one group whatever the table): the order of the ends shows a stable partition
    for s, e in ((500, 900), (500, 700), (300, 310), (500, 800), (300, 305), (500, 600), (500, 650)):
        out.append(b"chr2\t%d\t%d\t%s\n" % (s, e, listed[0]))
    stretch(b"chr2", n // 6)
    stretch(b"chrOnlyUnassigned", 50, only=unlisted + odd)            # a chromosome on which no group has anything
    stretch(b"chr3_random", n // 6)
    stretch(b"chr1", n // 6)                                          # chr1 comes back
    out.append(b"chr3_random\t10\t20\t" + listed[1] + b"\r")          # an open last line keeps its '\r': listed plus one byte, unassigned
    return b"".join(out), listed


def every_barcode(text):
    """the distinct fourth fields of a text whose data lines all have one of 1-255 bytes"""
    seen = {}
    for line in text.split(b"\n"):
        line = line[:-1] if line.endswith(b"\r") else line
        if line and not line.startswith(b"#"):
            seen.setdefault(line.split(b"\t")[3], None)
    return list(seen)
