"""`pyatac cells`: which barcodes of a single-cell fragment file are cells.  This command is this package's own, like `split` and
`cellcounts`, and it comes before both: it builds the barcode table they take from the fragment file itself.

The file is read ONCE (FragmentStore.discover_cells): every barcode in order of first appearance with three exact counters -- its
fragments, those shorter than --nfr_upper (nucleosome-free) and those from --nfr_upper up to --mono_upper (mono-nucleosomal).  A cell
passes when fragments >= --min_fragments and, if --max_nucleosome_signal X is given, mono / nfr <= X (a cell without a nucleosome-free
fragment fails that test).  The thresholds are the user's: no knee is searched for.

BASE.cells.tsv      the passing barcodes, one per line, in order of first appearance: `split --groups` and `cellcounts --cells` take it
                    unchanged;
BASE.cells.qc.tsv   every discovered cell: barcode, fragments, nfr, mono, nucleosome_signal (%.4f, NA when nfr is 0), pass (1 / 0),
                    behind a header line that begins with '#';
BASE.cells.txt      data_lines, unassigned_lines, barcodes, passing, fragments_in_passing.
Everything is computed before the first file is written, so an error leaves nothing behind.  (The table reader of `split` and `cellcounts`
skips lines that begin with '#' and drops a '\r' at a line's end: a barcode of that shape is in the files here and is not read back.)"""
import os

import numpy as np


class CellsError(ValueError):
    """`pyatac cells` cannot answer: a missing file, or thresholds no cell passes"""


def passing_cells(table, min_fragments=1000, max_nucleosome_signal=None):
    """bool per cell of a CellTable: n_frag >= min_fragments and, with a bound, n_nfr > 0 and n_mono / n_nfr <= bound"""
    ok = table.n_frag >= min_fragments
    if max_nucleosome_signal is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            signal = table.n_mono / table.n_nfr.astype(np.float64)
        ok &= (table.n_nfr > 0) & (signal <= max_nucleosome_signal)
    return ok


def get_cells(args):
    """`pyatac cells`: writes BASE.cells.tsv, BASE.cells.qc.tsv and BASE.cells.txt; returns (table, pass per cell)"""
    from .cellgroups import default_base
    from .fragments import FragmentStore
    if not os.path.exists(args.fragments):
        raise CellsError("%s: no such file" % args.fragments)
    base = args.out if args.out else default_base(args.fragments)
    table = FragmentStore.discover_cells(args.fragments, nfr_upper=args.nfr_upper, mono_upper=args.mono_upper)
    ok = passing_cells(table, args.min_fragments, args.max_nucleosome_signal)
    if not ok.any():
        raise CellsError("%s: no cell passes (%d barcodes, the largest has %d fragments; --min_fragments is %d)"
                         % (args.fragments, len(table), int(table.n_frag.max()) if len(table) else 0, args.min_fragments))
    keep = [b for b, o in zip(table.barcodes, ok.tolist()) if o]
    qc = [b"#barcode\tfragments\tnfr\tmono\tnucleosome_signal\tpass\n"]
    for b, f, n, m, o in zip(table.barcodes, table.n_frag.tolist(), table.n_nfr.tolist(), table.n_mono.tolist(), ok.tolist()):
        signal = b"%.4f" % (m / n) if n else b"NA"
        qc.append(b"%s\t%d\t%d\t%d\t%s\t%d\n" % (b, f, n, m, signal, o))
    summary = ("data_lines\t%d\nunassigned_lines\t%d\nbarcodes\t%d\npassing\t%d\nfragments_in_passing\t%d\n"
               % (table.n_data, table.n_unassigned, len(table), len(keep), int(table.n_frag[ok].sum())))
    with open(base + ".cells.tsv", "wb") as fh:
        fh.write(b"".join([b + b"\n" for b in keep]))
    with open(base + ".cells.qc.tsv", "wb") as fh:
        fh.write(b"".join(qc))
    with open(base + ".cells.txt", "w") as fh:
        fh.write(summary)
    return table, ok
