"""`pyatac nucleotide`: mono- or dinucleotide frequency around a set of sites (the reference's pyatac/get_nucleotide.py).

The reference fetches the window of every site and builds a Python list per word, per column, per site.  Here the sites are read
as columns, centred on the host, grouped by chromosome, and one natac_site_seq_counts call per chromosome adds every window into
an exact int64 [words x (up + down + 1)] matrix.  The finish -- M / n, the background division of --norm -- is float64 on the host
in the reference's order, so the returned matrix is bit-identical to the reference's.

The site rule (Python-2 integer division): centre = start + len // 2 on plus, end - len // 2 - 1 on minus ("-" is minus, every other
strand value and no --strand is plus); the window is the centre extended by `up` upstream and `down` (+ 1 with --dinucleotide)
downstream, clipped to the chromosome; a site whose clipped window is shorter than up + down + 1 (+ 1) is skipped and not counted
in n (so is a site whose clipped window is empty, on which the reference's seq_to_mat raises with --dinucleotide).  On the minus strand the window is reversed and complemented by translate('ACGT' -> 'TGCA') BEFORE it is upper-cased, so a
soft-masked (lower-case) base of a minus-strand site is reversed but not complemented; the sequence is therefore loaded with its case
(FastaStore.open_cased).  Letters other than A C G T after upper-casing match no row.

Backgrounds of --norm: mononucleotide frequencies are seq.getNucFreqs (device).  Dinucleotide frequencies are the reference's
line.count(word) per FASTA line -- non-overlapping, blind to words across a line break, divided by the base count -- which depends
on the file's line layout; they are counted on the host over the text file that way, and a FastaStore .npz, which has no lines, is
refused.

Value text: the reference writes result.astype('|S8'), the first 8 bytes of Python 2's float text: _py2_float_str(v)[:8].
ONE DELIBERATE DEVIATION: when that text carries an exponent (values below 1e-4, common with --dinucleotide over many sites) the
8-byte cut drops the exponent and the file would say 8.333333 for 8.33e-05; exactly those values are written as '%.2e' % v, which
is 8 bytes and correct.  Where the reference writes NaN because no site was used, NucleotideError is raised and nothing is written.
"""
import gzip
import itertools
import os
import time

import numpy as np

from .chunk import read_bed_columns
from .seq import ACGT, FastaStore, getNucFreqs
from .tracks import _py2_float_str

DINUCLEOTIDES = ["".join(p) for p in itertools.product("CGAT", repeat=2)]      # the reference's row order, get_nucleotide.py:48-53


class NucleotideError(Exception):
    """`pyatac nucleotide` cannot run on these arguments, or no site was used (nothing is written)"""


def site_centers(start, end, minus):
    """Chunk.center per site (pyatac/chunk.py:41-54): the base the window is built around"""
    half = (end - start) // 2
    return np.where(minus, end - half - 1, start + half)


def count_sites(names, chrom, start, end, minus, fasta, up, down, dinucleotide=False, timing=None):
    """(M int64[words, up + down + 1], n sites used, sites skipped) over the sites (columns of read_bed_columns): one
    natac_site_seq_counts call per chromosome that has sites.  A centre outside its chromosome has a clipped window (skipped)."""
    from .. import get_context
    fs = FastaStore.open_cased(fasta)
    missing = [c for c in names if c not in fs.seqs]
    if missing:
        raise NucleotideError("chromosome %s of the bed file is not in %s" % (", ".join(missing),
                                                                               fasta if isinstance(fasta, str) else "the FASTA"))
    t = timing if timing is not None else {}
    t.setdefault("device_s", 0.0)
    t.setdefault("kernel_ms", 0.0)
    word = 2 if dinucleotide else 1
    M = np.zeros((16 if dinucleotide else 4, up + down + 1), np.int64)
    n = 0
    center = site_centers(start, end, minus)
    for k, c in enumerate(names):
        s = fs.seqs[c]
        idx = np.flatnonzero((chrom == k) & (center >= 0) & (center < len(s)))
        if not len(idx):
            continue
        t0 = time.perf_counter()
        m, used, ms = get_context().site_seq_counts(s, center[idx], minus[idx], up, down, word, with_kernel_ms=True)
        t["device_s"] += time.perf_counter() - t0
        t["kernel_ms"] += ms
        M += m
        n += used
    return M, n, len(start) - n


def dinucleotide_line_freqs(fasta, words=DINUCLEOTIDES):
    """seq.getNucFreqs of the reference (pyatac/seq.py:47-58) for words of two letters, line by line over the text file"""
    out = np.zeros(len(words))
    n = 0.0
    bw = [w.encode("ascii") for w in words]
    with (gzip.open if fasta.endswith(".gz") else open)(fasta, "rb") as f:
        for line in f:
            if line[:1] != b">":
                sequence = line.rstrip(b"\n").upper()
                out += [sequence.count(w) for w in bw]
                n += len(sequence)
    return out / n


def value_text(v):
    """a value as the .nucfreq.txt file holds it: the first 8 bytes of Python 2's str(float); with an exponent, '%.2e'"""
    s = _py2_float_str(float(v))
    return "%.2e" % v if "e" in s else s[:8]


def nucfreq_text(words, result):
    return "".join(w + "\t" + "\t".join(value_text(v) for v in row) + "\n" for w, row in zip(words, result))


def get_nucleotide(args, timing=None):
    """`pyatac nucleotide` (get_nucleotide.py:61-83): writes <out>.nucfreq.txt and returns the full-precision matrix"""
    if not args.out:
        args.out = ".".join(os.path.basename(args.bed).split(".")[0:-1])
    if args.up < 0 or args.down < 0:
        raise NucleotideError("--up (%d) and --down (%d) must not be negative" % (args.up, args.down))
    if args.dinucleotide and args.norm and args.fasta.endswith(".npz"):
        raise NucleotideError("--dinucleotide --norm counts the background per line of the FASTA text, as the reference does; "
                              "the FastaStore %s has no lines: give the text FASTA" % args.fasta)
    t = timing if timing is not None else {}
    t0 = time.perf_counter()
    names, chrom, start, end, minus = read_bed_columns(args.bed, strand_col=args.strand)
    t["bed_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    fs = FastaStore.open_cased(args.fasta)
    t["fasta_s"] = time.perf_counter() - t0
    M, n, skipped = count_sites(names, chrom, start, end, minus, args.fasta, args.up, args.down, args.dinucleotide, timing=t)
    print("%d sites used, %d skipped (window clipped by a chromosome end)" % (n, skipped))
    if n == 0:
        raise NucleotideError("no site of %s has its whole window of %d bases inside a chromosome: nothing to average (no file written)" % (
            args.bed, args.up + args.down + 1 + int(args.dinucleotide)))
    words = DINUCLEOTIDES if args.dinucleotide else ACGT
    result = np.asarray(M, dtype=np.float64) / float(n)
    if args.norm:
        t0 = time.perf_counter()
        normfreqs = dinucleotide_line_freqs(args.fasta) if args.dinucleotide else getNucFreqs(fs, ACGT)
        t["background_s"] = time.perf_counter() - t0
        result = result / np.reshape(np.repeat(normfreqs, result.shape[1]), result.shape)
    t0 = time.perf_counter()
    with open(args.out + ".nucfreq.txt", "w") as f:
        f.write(nucfreq_text(words, result))
    t["text_s"] = time.perf_counter() - t0
    return result
