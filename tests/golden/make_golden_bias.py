#!/usr/bin/env python3
"""Generate tests/golden/pyatac_bias.npz by RUNNING THE REFERENCE'S `pyatac bias` (pyatac/make_bias_track.py) on a seeded synthetic genome.

Runs only in the build container (needs the reference and the Python-3 scratch copy made by oracle/make_scratch_ref.py), like
make_golden_tracks.py.  For every case of the grid (genome-wide / --bed; the built-in Human and Yeast PWMs and an asymmetric
descriptor file with up = 7, down = 12, the kind `pyatac pwm --no_sym` writes) it stores, as data only, the decompressed text of the
.Scores.bedgraph.gz the reference wrote, gzip-compressed, with the case's arguments.  The genome, the BED text and the descriptor
text are stored too.

The genome: chrA (3015 bases: a last 1-kb chunk of 15 bases, longer than either `down`) with a stretch of N, isolated Ns and IUPAC
codes, a 60-base poly-A stretch and a soft-masked (lower-case) stretch, which the reference upper-cases when it fetches
(pyatac/seq.py:22); chrB (1200); chrC (40, longer than the 21- and 20-base PWMs).  The BED regions overlap, touch, run past a
chromosome end, sit at base 0, hold a single base, and one lies on a chromosome the FASTA lacks (dropped with a warning).  No region
has an empty trimmed interval: the reference raises there (see nucleoatac_amd/pyatac/make_bias_track.py), so it cannot make a golden.

The text is the reference's under Python 2: the scratch copy runs on Python 3, whose str(float) is repr, so every value field is
rewritten with Python 2's str(float) (12 significant digits); the line structure, which the reference decides by float equality, is
kept as it is.

Traps stepped around here, not in the reference: make_bias_track's `bases/splitsize` gets the integer Python 2 computed, the process
pool and writer process run in this process, and signal.correlate is called with method="direct".  The reference's scipy (>= 0.16,
before `method=` existed) summed directly; scipy 1.15 resolves mode='valid' for these shapes to the FFT method, under which equal
windows differ in their last bits (a poly-A stretch breaks into a dozen lines, an all-N window gives -2.6e-16 instead of 0).

usage:  python oracle/make_scratch_ref.py /tmp/natac_scratch_ref
        python tests/golden/make_golden_bias.py [/tmp/natac_scratch_ref]
"""
import argparse
import gzip
import os
import queue
import sys
import types
import warnings

import numpy as np

SCRATCH = sys.argv[1] if len(sys.argv) > 1 else "/tmp/natac_scratch_ref"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(SCRATCH, "stubs"), os.path.join(SCRATCH, "src")]
os.environ.setdefault("MPLBACKEND", "agg")
os.chdir(os.path.join(SCRATCH, "src"))

import pyatac.bias as PB  # noqa: E402
import pyatac.make_bias_track as MB  # noqa: E402

TMP = os.path.join(SCRATCH, "work_bias")
os.makedirs(TMP, exist_ok=True)

CHROMS = {"chrA": 3015, "chrB": 1200, "chrC": 40}
BED = [("chrA", 0, 300), ("chrA", 200, 650), ("chrA", 640, 700), ("chrA", 700, 760), ("chrA", 1500, 1501), ("chrA", 2900, 3100),
       ("chrB", 1100, 1300), ("chrB", 5, 60), ("chrC", 0, 40), ("chrZ", 10, 20)]
ASYM_UP, ASYM_DOWN = 7, 12
CORRELATE_METHOD = "direct"


class PyInt(int):
    """an int whose `/` is Python 2's integer division"""

    def __truediv__(self, other):
        return PyInt(int(self) // other)


class _NoPool(object):
    def __init__(self, processes=None):
        pass

    def map(self, fn, items):
        return [fn(x) for x in items]

    def close(self):
        pass

    def join(self):
        pass


class _LateProcess(object):
    """the writer process: runs its loop at join(), after every track and the STOP marker are queued"""

    def __init__(self, target, args):
        self._run = lambda: target(*args)

    def start(self):
        pass

    def join(self):
        self._run()


MP = types.SimpleNamespace(Pool=_NoPool, JoinableQueue=lambda maxsize=0: queue.Queue(), Process=_LateProcess)


def make_genome(rng):
    seqs = {}
    for c, L in CHROMS.items():
        s = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L, p=[0.3, 0.2, 0.2, 0.3]).astype(np.uint8)
        if c == "chrA":
            s[100:130] = ord("N")                              # longer than a PWM: windows of N only score 0
            s[[300, 301, 999, 1000, 2000]] = ord("N")          # isolated Ns, one pair across a chunk boundary
            s[[350, 1777]] = [ord("R"), ord("Y")]              # IUPAC codes add 0 like N
            s[500:560] = ord("A")                              # homopolymer: equal neighbours merge into one line
            s[1200:1420] = s[1200:1420] + 32                   # soft-masked
            s[1300:1340] = ord("c")                            # a soft-masked homopolymer
            s[3005:3015] = s[3005:3015] + 32                   # lower case at the chromosome end
        if c == "chrB":
            s[0:25] = ord("n")
            s[1150:1200] = ord("T")
        seqs[c] = s
    return seqs


def asym_descriptor(rng):
    """the text of a descriptor file in PWM.save's layout (pyatac/bias.py:31-46) with up != down"""
    mat = np.exp(rng.normal(0.0, 0.35, size=(4, ASYM_UP + ASYM_DOWN + 1)))
    out = "#PWM Descriptor File\n#Contains PWM and pertinent information\n#up\n%d\n#down\n%d\n#nucleotides\nA\tC\tG\tT\n#mat\n" % (
        ASYM_UP, ASYM_DOWN)
    for row in mat:
        out += "\t".join("%.12g" % x for x in row) + "\n"
    return out


def py2_float_text(text):
    """rewrite the value column with Python 2's str(float)"""
    out = []
    for line in text.splitlines(True):
        f = line.rstrip("\n").split("\t")
        v = float(f[3])
        s = "%.12g" % v
        if "." not in s and "e" not in s and "n" not in s and "i" not in s:
            s += ".0"
        out.append("\t".join(f[:3] + [s]) + "\n")
    return "".join(out)


def main():
    rng = np.random.default_rng(20261017)
    seqs = make_genome(rng)
    fasta = os.path.join(TMP, "genome.npz")
    arrays = {"chrom_names": np.array(list(CHROMS)), "chrom_lengths": np.array(list(CHROMS.values()))}
    for c in CHROMS:
        arrays["seq_" + c] = seqs[c]
    np.savez(fasta, **arrays)
    bed = os.path.join(TMP, "regions.bed")
    bed_text = "".join("%s\t%d\t%d\n" % r for r in BED)
    with open(bed, "w") as f:
        f.write(bed_text)
    asym = os.path.join(TMP, "asym.PWM.txt")
    asym_text = asym_descriptor(rng)
    with open(asym, "w") as f:
        f.write(asym_text)
    MB.mp = MP
    correlate = PB.signal.correlate
    PB.signal = types.SimpleNamespace(correlate=lambda a, b, mode="full": correlate(a, b, mode=mode, method=CORRELATE_METHOD))
    out = dict(arrays)
    out["bed_text"] = np.array(bed_text)
    out["asym_pwm_text"] = np.array(asym_text)
    out["correlate_method"] = np.array(CORRELATE_METHOD)
    cases = []
    for region in ("genome", "bed"):
        for pwm in ("Human", "Yeast", "asym"):
            key = "%s_%s" % (region, pwm)
            a = argparse.Namespace(fasta=fasta, pwm=asym if pwm == "asym" else pwm, bed=bed if region == "bed" else None,
                                   out=os.path.join(TMP, key), cores=1)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                MB.make_bias_track(a, bases=PyInt(500000))
            dropped = [str(w.message) for w in caught if "not included in" in str(w.message)]
            assert (len(dropped) == 1 and "chrZ" in dropped[0]) if region == "bed" else not dropped, (key, dropped)
            with gzip.open(a.out + ".Scores.bedgraph.gz", "rt") as f:
                text = py2_float_text(f.read())
            assert text, key
            out["text_" + key] = np.frombuffer(gzip.compress(text.encode("ascii"), 9, mtime=0), np.uint8)
            out["args_" + key] = np.array([region, pwm])
            cases.append(key)
    out["cases"] = np.array(cases)
    dst = os.path.join(HERE, "pyatac_bias.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s: %d cases, %d bytes" % (dst, len(cases), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
