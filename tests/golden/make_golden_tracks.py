#!/usr/bin/env python3
"""Generate tests/golden/pyatac_tracks.npz by RUNNING THE REFERENCE'S `pyatac ins` and `pyatac cov` on seeded synthetic reads.

Runs only in the build container (needs the reference and the Python-3 scratch copy made by oracle/make_scratch_ref.py), like
make_golden_pwm.py.  For every case of the grid (genome-wide / --bed; ins with --smooth none / 1 / 10 / 21 / 301; cov with --window
121 / 100 / 1 and --scale 10 / 1; two (lower, upper) pairs; --not_atac) it stores, as data only, the decompressed text of the
.bedgraph.gz the reference wrote, gzip-compressed, with the case's arguments.  The reads and the BED text are stored too.

The text is the reference's under Python 2: the scratch copy runs on Python 3, whose str(float) is repr, so every value field is
rewritten with Python 2's str(float) (12 significant digits) -- the line structure, which the reference decides by float equality,
is kept as it is.

Python-3 traps of the reference's scripts are stepped around here, not in the reference: get_ins / get_cov's `bases/splitsize`,
`args.smooth / 2` and `args.window / 2` get the integers Python 2 computed (the arguments are handed over as an int whose `/` floors),
and the process pool and writer process run in this process.

usage:  python oracle/make_scratch_ref.py /tmp/natac_scratch_ref
        python tests/golden/make_golden_tracks.py [/tmp/natac_scratch_ref]
"""
import argparse
import gzip
import os
import queue
import sys
import types

import numpy as np

SCRATCH = sys.argv[1] if len(sys.argv) > 1 else "/tmp/natac_scratch_ref"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(SCRATCH, "stubs"), os.path.join(SCRATCH, "src")]
os.environ.setdefault("MPLBACKEND", "agg")
os.chdir(os.path.join(SCRATCH, "src"))

import pyatac.get_cov as GC  # noqa: E402
import pyatac.get_ins as GI  # noqa: E402

TMP = os.path.join(SCRATCH, "work_tracks")
os.makedirs(TMP, exist_ok=True)

# chrD carries no reads; chrC (40 bases) is shorter than the default coverage window
CHROMS = {"chrA": 3000, "chrB": 1200, "chrC": 40, "chrD": 800}
BED = [("chrA", 0, 300), ("chrA", 200, 650), ("chrA", 640, 700), ("chrA", 1500, 1501), ("chrA", 2900, 3100), ("chrB", 1100, 1300),
       ("chrB", 5, 60), ("chrC", 0, 40), ("chrD", 100, 200)]


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


def make_reads(rng):
    """forward proper-pair records per chromosome (pos sorted, |tlen|): a size mix, reads at both chromosome ends (some reaching past
    the end), and template lengths that put the insert size exactly at the lower / upper bounds of the grid, atac or not"""
    out = {}
    for c, L, n in (("chrA", 3000, 1500), ("chrB", 1200, 500), ("chrC", 40, 6)):
        if c == "chrC":
            pos = np.array([0, 2, 5, 9, 20, 30])
            tlen = np.array([8, 20, 30, 12, 15, 9])
        else:
            tlen = np.concatenate([rng.integers(1, 120, n // 3), rng.integers(120, 400, n // 3), rng.integers(400, 1100, n - 2 * (n // 3))])
            special = np.array([0, 8, 9, 50, 58, 300, 308, 299, 307, 2000, 2008, 1])
            tlen[:len(special) * 3] = np.tile(special, 3)
            pos = rng.integers(0, L - 10, n)
            pos[:20] = rng.integers(0, 15, 20)
            pos[20:40] = L - np.minimum(tlen[20:40], L - 1) + rng.integers(-20, 8, 20)
            pos = np.clip(pos, 0, L - 1)
        sign = np.where(rng.random(len(pos)) < 0.5, 1, -1)
        o = np.argsort(pos, kind="stable")
        out[c] = (pos[o].astype(np.int64), (tlen[o] * sign[o]).astype(np.int64))
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
    rng = np.random.default_rng(20261016)
    reads = make_reads(rng)
    bam = os.path.join(TMP, "reads.npz")
    arrays = {"chrom_names": np.array(list(CHROMS)), "chrom_lengths": np.array(list(CHROMS.values()))}
    for c in CHROMS:
        p, t = reads.get(c, (np.zeros(0, np.int64), np.zeros(0, np.int64)))
        arrays["pos_" + c], arrays["tlen_" + c] = p, t
    np.savez(bam, **arrays)
    bed = os.path.join(TMP, "regions.bed")
    bed_text = "".join("%s\t%d\t%d\n" % r for r in BED)
    with open(bed, "w") as f:
        f.write(bed_text)
    GI.mp = MP
    GC.mp = MP
    cases = []
    out = dict(arrays)
    out["bed_text"] = np.array(bed_text)
    grid = []
    for region in ("genome", "bed"):
        for lower, upper in ((0, 2000), (50, 300)):
            for atac in (True, False):
                small = (lower, upper) == (0, 2000) and atac       # the full sweep at the defaults; a few cases elsewhere
                for smooth in ((None, 1, 10, 21, 301) if small else (None, 21)):
                    if smooth in (1, 301) and region == "bed":
                        continue
                    grid.append(("ins", region, lower, upper, atac, dict(smooth=smooth)))
                for window, scale in (((121, 10), (100, 10), (1, 1), (121, 1)) if small else ((121, 10), (100, 1))):
                    grid.append(("cov", region, lower, upper, atac, dict(window=window, scale=scale)))
    grid.append(("ins", "genome", 0, 2000, True, dict(smooth=0)))
    for call, region, lower, upper, atac, extra in grid:
        tag = "_".join("%s%s" % (k, v) for k, v in sorted(extra.items()))
        key = "%s_%s_l%d_u%d_a%d_%s" % (call, region, lower, upper, atac, tag)
        a = argparse.Namespace(bam=bam, bed=bed if region == "bed" else None, out=os.path.join(TMP, key), cores=1, lower=lower,
                               upper=upper, atac=atac)
        for k, v in extra.items():
            setattr(a, k, PyInt(v) if isinstance(v, int) and not isinstance(v, bool) else v)
        if call == "ins":
            GI.get_ins(a, bases=PyInt(50000))
        else:
            a.scale = float(a.scale)
            GC.get_cov(a, bases=PyInt(50000))
        with gzip.open(a.out + ".%s.bedgraph.gz" % call, "rt") as f:
            text = py2_float_text(f.read())
        assert text, key
        out["text_" + key] = np.frombuffer(gzip.compress(text.encode("ascii"), 9, mtime=0), np.uint8)
        out["args_" + key] = np.array([call, region, str(lower), str(upper), str(int(atac)), repr(extra)])
        cases.append(key)
    out["cases"] = np.array(cases)
    dst = os.path.join(HERE, "pyatac_tracks.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s: %d cases, %d bytes" % (dst, len(cases), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
