#!/usr/bin/env python3
"""Generate tests/golden/pyatac_sites.npz by RUNNING THE REFERENCE'S `pyatac counts` (pyatac/get_counts.py) and `pyatac nucleotide`
(pyatac/get_nucleotide.py) on a seeded synthetic genome and fragment store.

Runs only in the build container (needs the reference and the Python-3 scratch copy made by oracle/make_scratch_ref.py), like
make_golden_bias.py.  Everything stored is data: the genome, the fragment records, the BED text and, per case, the arguments, the
text of the file the reference wrote (gzip-compressed) and, for `nucleotide`, the full-precision matrix, the sites the reference
used and its background frequencies.

The genome: chrA (4000 bases) with a stretch of N, isolated Ns, IUPAC letters and two soft-masked (lower-case) stretches; chrB
(1500) starting with lower-case n; chrC (60), shorter than any window of the cases.  The fragment store has records on chrA and chrB
with |tlen| from 0 to 700: tlen == 8 is an insert of 0 under the ATAC offsets (r = l - 1), tlen < 8 a negative one.  The BED has six
columns with the strand in column 6 ("+", "-", "." and "*"); regions of even and odd length, so centre differs by strand; sites
whose window is clipped at the start and at the end of a chromosome, one whose centre lies past a chromosome's end and one on chrC
(none whose clipped window is empty: with --dinucleotide the reference's seq_to_mat raises on an empty sequence);
overlapping, repeated and unsorted regions; two of length zero (dropped by ChunkList.read); a minus-strand site in the middle of the
soft-masked stretch, whose bases the reference reverses but does not complement; and a window that ends exactly at the left end of
an insert-0 fragment, which counts through r = l - 1 alone.

Cases: counts with and without --not_atac for (lower, upper) = (0, 500) and (100, 300); nucleotide mono / --dinucleotide, with /
without --strand 6, with / without --norm at up = down = 40, and mono --strand 6 with up = 25, down = 60.  --norm reads the text
FASTA (lines of LINE_WIDTH bases, case kept) the way the reference does; the tests write the same file.

Traps stepped around here, not in the reference:
  * np.int (gone from NumPy) in get_counts: the module sees a numpy whose `int` is the builtin;
  * the process pool of get_nucleotide runs in this process;
  * result.astype('|S8') under Python 3 cuts repr(float) to 8 bytes, not Python 2's str(float): the matrices of get_nucleotide are
    made an ndarray subclass whose astype('|S8') records the full-precision matrix and returns Python 2's float text ('%.12g', with
    '.0' for integers) cut to 8 characters -- a reading of what the reference's NumPy did under Python 2, which is not on this machine.
    This generator asserts that no value's Python-2 text carries an exponent, so the package's one deliberate deviation from that
    rule (nucleoatac_amd/pyatac/get_nucleotide.py) never touches a golden;
  * the pysam stand-in reads .npz stores while seq.getNucFreqs opens its argument as text: it is handed the text FASTA.

usage:  python oracle/make_scratch_ref.py /tmp/natac_scratch_ref
        python tests/golden/make_golden_sites.py [/tmp/natac_scratch_ref]
"""
import argparse
import gzip
import os
import sys

import numpy as np

SCRATCH = sys.argv[1] if len(sys.argv) > 1 else "/tmp/natac_scratch_ref"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(SCRATCH, "stubs"), os.path.join(SCRATCH, "src")]
os.environ.setdefault("MPLBACKEND", "agg")
os.chdir(os.path.join(SCRATCH, "src"))

import pyatac.get_counts as GC  # noqa: E402
import pyatac.get_nucleotide as GN  # noqa: E402

TMP = os.path.join(SCRATCH, "work_sites")
os.makedirs(TMP, exist_ok=True)

CHROMS = {"chrA": 4000, "chrB": 1500, "chrC": 60}
LINE_WIDTH = 60
ZERO_INSERT_POS = 2500          # a tlen == 8 record here: l = 2504, r = 2503
BED = [  # chrom, start, end, name, score, strand
    ("chrA", 1000, 1500, "a", 0, "+"), ("chrA", 1000, 1500, "a_minus", 0, "-"),          # even length: centre 1250 / 1249
    ("chrA", 1000, 1501, "odd", 0, "+"), ("chrA", 1000, 1501, "odd_minus", 0, "-"),      # odd length: centre 1250 either way
    ("chrA", 1290, 1311, "masked_minus", 0, "-"), ("chrA", 1290, 1311, "masked_plus", 0, "+"),
    ("chrA", 3000, 3400, "late", 0, "."), ("chrA", 200, 900, "early_unsorted", 0, "*"),
    ("chrA", 600, 1100, "overlap", 0, "-"), ("chrA", 600, 1100, "overlap", 0, "-"),
    ("chrA", 0, 30, "clip_start", 0, "+"), ("chrA", 0, 30, "clip_start_minus", 0, "-"),
    ("chrA", 3950, 4000, "clip_end", 0, "+"), ("chrA", 3930, 3990, "clip_end_minus", 0, "-"),
    ("chrA", 500, 500, "zero", 0, "+"), ("chrA", 100, 140, "nstretch", 0, "-"),
    ("chrA", 2494, 2504, "zero_insert_right_end", 0, "+"), ("chrA", 0, 4000, "whole", 0, "+"),
    ("chrB", 700, 701, "one_base", 0, "-"), ("chrB", 1490, 1520, "past_end", 0, "+"),
    ("chrB", 0, 100, "lower_n", 0, "+"), ("chrB", 900, 900, "zero2", 0, "-"), ("chrB", 300, 1200, "big", 0, "-"),
    ("chrC", 10, 50, "short_chrom", 0, "+"), ("chrA", 1995, 2006, "iupac", 0, "+"),
]
COUNT_CASES = [(atac, lo, up) for atac in (1, 0) for lo, up in ((0, 500), (100, 300))]
NUC_CASES = [(di, strand, norm, 40, 40) for di in (0, 1) for strand in (0, 6) for norm in (0, 1)] + [(0, 6, 0, 25, 60)]


def py2_float_str(v):
    s = "%.12g" % v
    if "." not in s and "e" not in s and "n" not in s and "i" not in s:
        s += ".0"
    return s


CAPTURE = {}


class Rec(np.ndarray):
    """the matrices of get_nucleotide: astype('|S8') records the matrix and gives Python 2's text of it"""

    def astype(self, dtype, *a, **k):
        if dtype == "|S8":
            full = np.array(self, dtype=np.float64)
            CAPTURE["result"] = full
            texts = [[py2_float_str(float(v)) for v in row] for row in full]
            assert not any("e" in s for row in texts for s in row), "a golden value's Python-2 text carries an exponent"
            return np.array([[s[:8] for s in row] for row in texts])
        return np.ndarray.astype(self, dtype, *a, **k)


class NumpyWithInt(object):
    int = int

    def __getattr__(self, k):
        return getattr(np, k)


class NumpyRec(NumpyWithInt):
    @staticmethod
    def zeros(shape, *a, **k):
        return np.zeros(shape, *a, **k).view(Rec)


class NoPool(object):
    def __init__(self, processes=None):
        pass

    def map(self, fn, items):
        return [fn(x) for x in items]

    def close(self):
        pass

    def join(self):
        pass


def make_genome(rng):
    seqs = {}
    for c, L in CHROMS.items():
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L, p=[0.3, 0.2, 0.2, 0.3]).astype(np.uint8)
        if c == "chrA":
            s[100:130] = ord("N")
            s[[640, 641, 1233, 3100]] = ord("N")
            s[[1999, 2003, 3200]] = [ord("R"), ord("Y"), ord("k")]     # IUPAC letters, one lower case
            s[1200:1400] = s[1200:1400] + 32                           # soft-masked
            s[1296:1300] = ord("A")                                    # upper-case islands inside it: complemented on minus
            s[3380:3420] = s[3380:3420] + 32
        if c == "chrB":
            s[0:25] = ord("n")
            s[690:712] = s[690:712] + 32
        seqs[c] = s
    return seqs


def make_fragments(rng):
    pos, tlen = {}, {}
    for c, n in (("chrA", 1100), ("chrB", 400)):
        p = np.sort(rng.integers(0, CHROMS[c] - 50, size=n))
        t = np.where(rng.random(n) < 0.7, rng.integers(30, 300, size=n), rng.integers(300, 700, size=n))
        odd = rng.random(n)
        t[odd < 0.03] = 8           # insert 0 with the ATAC offsets
        t[odd < 0.02] = rng.integers(1, 8, size=int((odd < 0.02).sum()))
        t[odd < 0.008] = 0
        if c == "chrA":
            k = int(np.searchsorted(p, ZERO_INSERT_POS))
            p[k], t[k] = ZERO_INSERT_POS, 8
            p = np.sort(p)
            assert p[k] == ZERO_INSERT_POS
            near = np.flatnonzero((p >= ZERO_INSERT_POS - 520) & (p <= ZERO_INSERT_POS + 20))
            t[near[near != k]] = 650        # nothing else can count for the window that ends at this record's left end
        pos[c], tlen[c] = p.astype(np.int32), t.astype(np.int32)
    pos["chrC"], tlen["chrC"] = np.zeros(0, np.int32), np.zeros(0, np.int32)
    return pos, tlen


def main():
    rng = np.random.default_rng(20261017)
    seqs = make_genome(rng)
    pos, tlen = make_fragments(rng)
    names = np.array(list(CHROMS))
    lens = np.array(list(CHROMS.values()))
    out = {"chrom_names": names, "chrom_lengths": lens, "fasta_line_width": np.array(LINE_WIDTH)}
    fasta = os.path.join(TMP, "genome.npz")
    np.savez(fasta, chrom_names=names, chrom_lengths=lens, **{"seq_" + c: seqs[c] for c in CHROMS})
    text_fasta = os.path.join(TMP, "genome.fa")
    with open(text_fasta, "wb") as f:
        for c in CHROMS:
            f.write(b">" + c.encode() + b"\n")
            raw = seqs[c].tobytes()
            for i in range(0, len(raw), LINE_WIDTH):
                f.write(raw[i:i + LINE_WIDTH] + b"\n")
    bam = os.path.join(TMP, "frags.npz")
    np.savez(bam, chrom_names=names, chrom_lengths=lens, **{"pos_" + c: pos[c] for c in CHROMS}, **{"tlen_" + c: tlen[c] for c in CHROMS})
    for c in CHROMS:
        out["seq_" + c], out["pos_" + c], out["tlen_" + c] = seqs[c], pos[c], tlen[c]
    bed = os.path.join(TMP, "sites.bed")
    bed_text = "".join("%s\t%d\t%d\t%s\t%d\t%s\n" % r for r in BED)
    with open(bed, "w") as f:
        f.write(bed_text)
    out["bed_text"] = np.array(bed_text)
    kept = [r for r in BED if r[2] - r[1] >= 1]

    GC.np = NumpyWithInt()
    keys = []
    for atac, lo, up in COUNT_CASES:
        key = "counts_%s_%d_%d" % ("atac" if atac else "notatac", lo, up)
        a = argparse.Namespace(bam=bam, bed=bed, out=os.path.join(TMP, key), atac=bool(atac), lower=lo, upper=up)
        GC.get_counts(a)
        with gzip.open(a.out + ".counts.txt.gz", "rt") as f:
            text = f.read()
        vals = [int(x) for x in text.split()]
        assert len(vals) == len(kept) and text == "".join("%d\n" % v for v in vals), key
        if atac and lo == 0:       # the window that ends at the left end of the insert-0 record holds its right end only
            assert vals[[r[3] for r in kept].index("zero_insert_right_end")] == 1, key
        out["text_" + key] = np.frombuffer(gzip.compress(text.encode("ascii"), 9, mtime=0), np.uint8)
        out["args_" + key] = np.array([atac, lo, up])
        keys.append(key)
    out["count_cases"] = np.array(keys)

    GN.np = NumpyRec()
    GN.Pool = NoPool
    get_sequence, get_freqs = GN.seq.get_sequence, GN.seq.getNucFreqs
    lengths = []
    GN.seq.get_sequence = lambda chunk, fa: (lambda s: (lengths.append(len(s)), s)[1])(get_sequence(chunk, fa))
    freqs = {}
    GN.seq.getNucFreqs = lambda fa, nucs: freqs.setdefault(len(nucs), get_freqs(text_fasta, nucs))
    keys = []
    for di, strand, norm, up, down in NUC_CASES:
        key = "nuc_%s_%s_%s_%d_%d" % ("di" if di else "mono", "strand" if strand else "nostrand", "norm" if norm else "raw", up, down)
        a = argparse.Namespace(fasta=fasta, bed=bed, dinucleotide=bool(di), up=up, down=down, strand=strand or None,
                               out=os.path.join(TMP, key), cores=1, norm=bool(norm))
        del lengths[:]
        CAPTURE.clear()
        GN.get_nucleotide(a)
        used = np.array(lengths) == up + down + 1 + di
        assert len(used) == len(kept) and used.any() and not used.all(), key
        with open(a.out + ".nucfreq.txt") as f:
            text = f.read()
        mat = CAPTURE["result"]
        assert mat.shape == (16 if di else 4, up + down + 1) and np.isfinite(mat).all(), key
        assert len(text.splitlines()) == mat.shape[0] and all(len(x.split("\t")) == mat.shape[1] + 1 for x in text.splitlines()), key
        out["text_" + key] = np.frombuffer(gzip.compress(text.encode("ascii"), 9, mtime=0), np.uint8)
        out["mat_" + key] = mat
        out["used_" + key] = used
        out["args_" + key] = np.array([di, strand, norm, up, down])
        keys.append(key)
    out["nuc_cases"] = np.array(keys)
    out["bg_mono"], out["bg_di"] = freqs[4], freqs[16]
    dst = os.path.join(HERE, "pyatac_sites.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s: %d + %d cases, %d bytes" % (dst, len(COUNT_CASES), len(NUC_CASES), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
