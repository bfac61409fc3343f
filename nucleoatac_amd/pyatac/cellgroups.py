"""Cell groups of a single-cell fragment file: the barcode table `pyatac split` reads (read_groups) and the command itself (split_cells),
which turns one fragment file into one FragmentStore per group in a single pass (FragmentStore.split_fragments) and writes every group
where the other commands take it through --bam: BASE.<group>.npz, or BASE.<group>.tsv.gz with its .tbi."""
import gzip
import os
import re

MAX_GROUPS = 255            # NATAC_SPLIT_MAX_GROUPS of include/natac.h
DEFAULT_GROUP = "selected"  # the group of a table without a second column: a whitelist
_GROUP_NAME = re.compile(r"[A-Za-z0-9._-]{1,64}\Z")


class CellGroupError(ValueError):
    """a barcode table `pyatac split` cannot use; the message names the file and the line"""


class CellGroups(object):
    """names[g] = the name of group g (order of first appearance); barcodes[k] (bytes, distinct) belongs to group group_of[k]"""

    def __init__(self, names, barcodes, group_of):
        self.names, self.barcodes, self.group_of = list(names), list(barcodes), list(group_of)

    def listed(self):
        """barcodes listed per group"""
        n = [0] * len(self.names)
        for g in self.group_of:
            n[g] += 1
        return n


def read_groups(path, header=False):
    """TAB-separated: column 1 the barcode (taken byte for byte), column 2 the group (absent: every barcode is in `selected`); further columns
    are ignored.  Lines that are empty or start with '#' are skipped; header=True drops the first remaining line.  Group names match
    [A-Za-z0-9._-]{1,64} (they become parts of file names) and are numbered in order of first appearance; a barcode listed twice in one group
    counts once.  CellGroupError("<path>: line N: ...") for a barcode in two groups, an empty barcode or one longer than 255 bytes, a bad
    group name, more than 255 groups, and for a table without any barcode."""
    with open(path, "rb") as fh:
        zipped = fh.read(2) == b"\x1f\x8b"
    with (gzip.open if zipped else open)(path, "rb") as fh:
        lines = fh.read().split(b"\n")
    names, ids, barcodes, group_of, where = [], {}, [], [], {}
    for no, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line or line[:1] == b"#":
            continue
        if header:
            header = False
            continue
        f = line.split(b"\t")
        bc = f[0]
        if not bc:
            raise CellGroupError("%s: line %d: empty barcode" % (path, no))
        if len(bc) > 255:
            raise CellGroupError("%s: line %d: barcode longer than 255 bytes" % (path, no))
        name = f[1].decode("latin-1") if len(f) > 1 else DEFAULT_GROUP
        if not _GROUP_NAME.match(name):
            raise CellGroupError("%s: line %d: group name %r does not match [A-Za-z0-9._-]{1,64}" % (path, no, name))
        if name not in ids:
            if len(names) == MAX_GROUPS:
                raise CellGroupError("%s: line %d: more than %d groups" % (path, no, MAX_GROUPS))
            ids[name] = len(names)
            names.append(name)
        g = ids[name]
        if bc in where:
            k, first = where[bc]
            if group_of[k] != g:
                raise CellGroupError("%s: line %d: barcode %s is in group %s here and in group %s on line %d"
                                     % (path, no, bc.decode("latin-1"), name, names[group_of[k]], first))
            continue
        where[bc] = (len(barcodes), no)
        barcodes.append(bc)
        group_of.append(g)
    if not barcodes:
        raise CellGroupError("%s: line %d: no barcode in the table" % (path, len(lines)))
    return CellGroups(names, barcodes, group_of)


def default_base(fragments):
    """the fragment file's basename without its suffixes"""
    from .fragments import FRAGMENT_SUFFIXES
    base = os.path.basename(str(fragments))
    for suf in sorted(FRAGMENT_SUFFIXES, key=len, reverse=True):
        if base.endswith(suf):
            return base[:-len(suf)]
    return base


def split_cells(args):
    """`pyatac split`: everything is computed before the first file is written, so an error leaves nothing behind"""
    from .fragments import FragmentStore
    groups = read_groups(args.groups, header=args.header)
    if not os.path.exists(args.fragments):
        raise CellGroupError("%s: no such file" % args.fragments)
    stores, bc_count, n_unassigned = FragmentStore.split_fragments(args.fragments, groups.barcodes, groups.group_of, len(groups.names))
    base = args.out if args.out else default_base(args.fragments)
    seen = [0] * len(groups.names)
    for k, g in enumerate(groups.group_of):
        seen[g] += 1 if bc_count[k] > 0 else 0
    written = []
    for name, st in zip(groups.names, stores):
        if args.format == "npz":
            st.save_npz("%s.%s.npz" % (base, name))
            written.append("%s.%s.npz" % (base, name))
        else:
            written.append(st.save_fragments("%s.%s.tsv.gz" % (base, name)))
    with open(base + ".split.txt", "w") as fh:
        fh.write("group\tbarcodes_listed\tbarcodes_seen\tfragments\n")
        for name, st, n_listed, n_seen in zip(groups.names, stores, groups.listed(), seen):
            fh.write("%s\t%d\t%d\t%d\n" % (name, n_listed, n_seen, sum(len(st.pos[c]) for c in st.references)))
        fh.write("unassigned\t%d\n" % n_unassigned)
    return written + [base + ".split.txt"]
