#!/usr/bin/env python3
"""Generate tests/golden/pwm_fit.npz by RUNNING THE REFERENCE'S `pyatac pwm` and `pyatac sizes` on seeded synthetic inputs.

Runs only in the build container (needs the reference and the Python-3 scratch copy made by oracle/make_scratch_ref.py), like
make_golden.py.  For every case of the grid (sym / no_sym, genome-wide / --bed, flank 0 / 10 / 100, two (lower, upper) pairs, atac on /
off) it stores, as data only:
  - the summed window counts M and insertion count n of the reference's _pwmHelper over the reference's own chunk sets,
  - the background frequencies (getNucFreqs / getNucFreqsFromChunkList) and their integer numerators and denominator,
  - the matrix get_pwm wrote and the text of its .PWM.txt;
and the .fragmentsizes.txt texts of `pyatac sizes` with and without --bed.  The inputs (genome, reads, BED texts) are stored too.

Two Python-3 traps of the reference are stepped around here, not in the reference: get_pwm's chunks.split(items=bases/splitsize)
gets the integer Python 2 computed, and seq.getNucFreqs (which opens the FASTA as text) gets a text copy of the genome.

usage:  python oracle/make_scratch_ref.py /tmp/natac_scratch_ref
        python tests/golden/make_golden_pwm.py [/tmp/natac_scratch_ref]
"""
import argparse
import os
import sys

import numpy as np

SCRATCH = sys.argv[1] if len(sys.argv) > 1 else "/tmp/natac_scratch_ref"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(SCRATCH, "stubs"), os.path.join(SCRATCH, "src")]
os.environ.setdefault("MPLBACKEND", "agg")
os.chdir(os.path.join(SCRATCH, "src"))

import pyatac.get_pwm as GP  # noqa: E402
import pyatac.seq as SEQ  # noqa: E402
from pyatac.chunk import ChunkList  # noqa: E402
from pyatac.get_sizes import get_sizes  # noqa: E402
from pyatac.utils import read_chrom_sizes_from_fasta  # noqa: E402

TMP = os.path.join(SCRATCH, "work_pwm")
os.makedirs(TMP, exist_ok=True)

CHROMS = {"chrA": 30000, "chrB": 12000, "chrC": 150}     # chrB and chrC carry no reads; chrC is shorter than 2 * 100
FLANKS = (0, 10, 100)
SIZE_PAIRS = ((0, 2000), (50, 300))


def make_genome(rng):
    seqs = {}
    for c, L in CHROMS.items():
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L, p=[0.3, 0.2, 0.2, 0.3])
        if c == "chrA":
            s[4000:4300] = ord("N")                            # N runs
            s[20000:20050] = ord("N")
            s[rng.choice(L, 40, replace=False)] = ord("N")     # isolated Ns
            s[9000:9400] = s[9000:9400] + 32                   # a soft-masked (lower-case) run
        if c == "chrB":
            s[100:160] = ord("N")
        seqs[c] = s.astype(np.uint8)
    return seqs


def make_reads(rng, n=6000):
    L = CHROMS["chrA"]
    tlen = np.concatenate([rng.integers(20, 120, n // 3), rng.integers(120, 400, n // 3), rng.integers(400, 1300, n - 2 * (n // 3))])
    pos = rng.integers(0, L - 20, n)
    # fragments at both chromosome ends
    pos[:30] = rng.integers(0, 40, 30)
    pos[30:60] = L - tlen[30:60] + rng.integers(-30, 5, 30)
    pos = np.clip(pos, 0, L - 1)
    o = np.argsort(pos, kind="stable")
    sign = np.where(rng.random(n) < 0.5, 1, -1)        # template length sign does not matter (|tlen|)
    return pos[o].astype(np.int64), (tlen[o] * sign[o]).astype(np.int64)


BED = [("chrA", 0, 700), ("chrA", 500, 1500), ("chrA", 1200, 1300), ("chrA", 3900, 4500), ("chrA", 8800, 9600),
       ("chrA", 15000, 17000), ("chrA", 16000, 16500), ("chrA", 29500, 30100), ("chrA", 2, 8), ("chrA", 29995, 30000),
       ("chrB", 50, 2000), ("chrZ", 100, 900), ("chrC", 10, 140)]


def bed_text(rows):
    return "".join("%s\t%d\t%d\n" % r for r in rows)


def clipped_bed(rows):
    """flank 0: the reference does not clip a region to its chromosome and fails on one that reaches past the end; the golden
    flank-0 cases use the BED already clipped to [0, L)"""
    out = []
    for c, s, e in rows:
        if c in CHROMS:
            s, e = max(s, 0), min(e, CHROMS[c])
            if e > s:
                out.append((c, s, e))
        else:
            out.append((c, s, e))
    return out


class _NoPool(object):
    def __init__(self, processes=None):
        pass

    def map(self, fn, items):
        return [fn(x) for x in items]

    def close(self):
        pass

    def join(self):
        pass


def main():
    rng = np.random.default_rng(20261015)
    seqs = make_genome(rng)
    pos, tlen = make_reads(rng)
    fa = os.path.join(TMP, "genome.npz")
    np.savez(fa, chrom_names=np.array(list(CHROMS)), chrom_lengths=np.array(list(CHROMS.values())),
             **{"seq_" + c: s for c, s in seqs.items()})
    fa_txt = os.path.join(TMP, "genome.fa")
    with open(fa_txt, "w") as f:
        for c, s in seqs.items():
            f.write(">%s\n" % c)
            b = s.tobytes().decode("ascii")
            for i in range(0, len(b), 60):
                f.write(b[i:i + 60] + "\n")
    bam = os.path.join(TMP, "reads.npz")
    empty = np.zeros(0, np.int64)
    np.savez(bam, chrom_names=np.array(list(CHROMS)), chrom_lengths=np.array(list(CHROMS.values())), pos_chrA=pos, tlen_chrA=tlen,
             pos_chrB=empty, tlen_chrB=empty, pos_chrC=empty, tlen_chrC=empty)
    beds = {}
    for key, rows in (("bed", BED), ("bed_f0", clipped_bed(BED)), ("bed_sizes", [r for r in BED if r[0] in CHROMS])):
        beds[key] = bed_text(rows)
        with open(os.path.join(TMP, key + ".bed"), "w") as f:
            f.write(beds[key])

    # the two Python-3 traps (see the module docstring)
    orig_split, orig_freqs = ChunkList.split, SEQ.getNucFreqs
    ChunkList.split = lambda self, bases=None, items=None: orig_split(self, bases=bases, items=None if items is None else int(items))
    GP.seq.getNucFreqs = lambda fasta, nucleotides: orig_freqs(fa_txt, nucleotides)
    GP.Pool = _NoPool

    out = dict(chrom_names=np.array(list(CHROMS)), chrom_lengths=np.array(list(CHROMS.values())), pos_chrA=pos, tlen_chrA=tlen,
               flanks=np.array(FLANKS), size_pairs=np.array(SIZE_PAIRS), **{"seq_" + c: s for c, s in seqs.items()},
               **{key + "_text": np.array(t) for key, t in beds.items()})
    chrs = read_chrom_sizes_from_fasta(fa)
    nucs = ["A", "C", "G", "T"]
    cases = []
    for sym in (True, False):
        for use_bed in (False, True):
            for flank in FLANKS:
                for lower, upper in SIZE_PAIRS:
                    for atac in (True, False):
                        key = "s%d_b%d_f%d_l%d_u%d_a%d" % (sym, use_bed, flank, lower, upper, atac)
                        bed = os.path.join(TMP, ("bed_f0" if flank == 0 else "bed") + ".bed") if use_bed else None
                        if bed is None:
                            chunks = ChunkList.convertChromSizes(chrs, splitsize=1000, offset=flank)
                            sets = chunks.split(items=50)
                        else:
                            chunks = ChunkList.read(bed, chromDict=chrs, min_offset=flank)
                            sets = chunks.split(bases=50000)
                        params = GP._PWMParameters(bam=bam, up=flank, down=flank, fasta=fa, lower=lower, upper=upper, atac=atac, sym=sym)
                        parts = [GP._pwmHelper((s, params)) for s in sets]
                        M = np.sum([p[0] for p in parts], axis=0)
                        n = float(np.sum([p[1] for p in parts]))
                        assert np.array_equal(M, np.rint(M)) and n == int(n) and n > 0, key
                        if bed is None:
                            freqs = orig_freqs(fa_txt, nucs)
                            bg_n = sum(CHROMS.values())
                        else:
                            freqs = SEQ.getNucFreqsFromChunkList(chunks, fa, nucs)
                            bg_n = sum(c.end - c.start for c in chunks)
                        bg_counts = np.rint(np.asarray(freqs) * bg_n).astype(np.int64)
                        assert np.array_equal(bg_counts / float(bg_n), freqs), key
                        args = argparse.Namespace(bam=bam, fasta=fa, bed=bed, flank=flank, lower=lower, upper=upper, atac=atac, sym=sym,
                                                  dinucleotide=False, cores=1, out=os.path.join(TMP, key))
                        GP.get_pwm(args)
                        with open(args.out + ".PWM.txt") as f:
                            text = f.read()
                        rows = text.split("#mat\n")[1].strip("\n").split("\n")
                        pwm = np.array([[float(x) for x in r.split("\t")] for r in rows])
                        assert pwm.shape == (4, 2 * flank + 1) and np.all(np.isfinite(pwm)), key
                        out.update({"M_" + key: M.astype(np.int64), "n_" + key: np.int64(n), "freqs_" + key: np.asarray(freqs),
                                    "bg_counts_" + key: bg_counts, "bg_n_" + key: np.int64(bg_n), "pwm_" + key: pwm,
                                    "pwm_text_" + key: np.array(text)})
                        cases.append(key)
    out["cases"] = np.array(cases)
    for key, bed in (("sizes_all", None), ("sizes_bed", os.path.join(TMP, "bed_sizes.bed"))):
        for lower, upper, atac in ((0, 500, True), (30, 250, False)):
            k = "%s_l%d_u%d_a%d" % (key, lower, upper, atac)
            args = argparse.Namespace(bam=bam, bed=bed, lower=lower, upper=upper, atac=atac, out=os.path.join(TMP, k), no_plot=True)
            get_sizes(args)
            with open(args.out + ".fragmentsizes.txt") as f:
                out["text_" + k] = np.array(f.read())
    np.savez_compressed(os.path.join(HERE, "pwm_fit.npz"), **out)
    print("wrote %s: %d pwm cases, 4 sizes cases" % (os.path.join(HERE, "pwm_fit.npz"), len(cases)))


if __name__ == "__main__":
    main()
