#!/usr/bin/env python3
"""Generate tests/golden/pyatac_signal.npz by RUNNING THE REFERENCE'S `pyatac signal` (pyatac/signal_around_sites.py) on a seeded
synthetic bedGraph track and a hand-made BED.

Runs only in the build container (needs the reference and the Python-3 scratch copy made by oracle/make_scratch_ref.py), like
make_golden_sites.py.  Everything stored is data: the track text, the sizes text, the BED texts and, per case, the arguments, the
text of the files the reference wrote (.tracks.txt.gz decompressed and stored gzip-compressed, .agg.track.txt) and the
full-precision matrix the reference handed to np.savetxt.

The track: chrA (3000 bases) and chrB (40 bases, shorter than the 51 columns of the main cases) have records, chrN (500) is in the
sizes file only.  chrA is run-length records of 1 to 9 bases with values of up to 5 significant digits, negative ones and zeros among
them; no record over [600, 900) (NaN); integer-valued records over [1500, 2100); and two overlapping records, [1200, 1260) = 1.5 then
[1240, 1300) = -0.75, of which the later one wins on [1240, 1260).  The pysam stand-in of the scratch copy scans a gzip text, so the
track is written as plain gzip here; the tests bgzip and index the same text with the package's own writers.

The BED (strand in column 6: "+", "-", "." and "*"): regions of even and odd length on both strands (the centre differs by strand for
an even length); a site clipped at the start of chrA, one whose window starts at 0 exactly (no padding, although it "starts at 0"),
one clipped at the end; one on chrB clipped at both ends, which is padded on the left only; one entirely in the gap (an all-NaN row,
S == 0 under --scale), one half in it; one over the overlapping records; one on chrN; one whose window begins exactly at the end of
chrA (empty read, all padding); two rows of length zero (dropped by ChunkList.read).  A second BED lies wholly in the integer-valued
stretch: its sums are exact in any order.  Two more hold a site whose clipped window has negative length and a site on a chromosome
that is not in the sizes file: the generator asserts that the reference raises on each.

Cases (up = down = 25 unless said): plain, --exp, --positive, --scale and --exp --positive --scale, each with --all, without and with
--strand 6; --norm --scale --strand 6 without --all (the site-by-site aggregate); --no_agg --all; up = down = 0; up = 10, down = 30
with --strand 6; and the integer BED plain and --positive with --strand 6.

Traps stepped around here, not in the reference: the process pool runs in this process; np.savetxt is wrapped to keep a copy of the
matrix before the reference zeroes its NaNs; the .eps the reference plots is written to the scratch directory and dropped.

usage:  python oracle/make_scratch_ref.py /tmp/natac_scratch_ref
        python tests/golden/make_golden_signal.py [/tmp/natac_scratch_ref]
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

import pyatac.signal_around_sites as SA  # noqa: E402

TMP = os.path.join(SCRATCH, "work_signal")
os.makedirs(TMP, exist_ok=True)

SIZES = [("chrA", 3000), ("chrB", 40), ("chrN", 500)]
GAP = (600, 900)
INT_RUN = (1500, 2100)
BED = [  # chrom, start, end, name, score, strand
    ("chrA", 1000, 1100, "even", 0, "+"), ("chrA", 1000, 1100, "even_minus", 0, "-"),        # centre 1050 / 1049
    ("chrA", 1000, 1101, "odd", 0, "+"), ("chrA", 1000, 1101, "odd_minus", 0, "-"),          # centre 1050 either way
    ("chrA", 0, 30, "clip_start", 0, "+"), ("chrA", 0, 30, "clip_start_minus", 0, "-"),
    ("chrA", 15, 36, "starts_at_0_exactly", 0, "+"), ("chrA", 15, 36, "starts_at_0_exactly_minus", 0, "-"),     # centre 25
    ("chrA", 2980, 3000, "clip_end", 0, "+"), ("chrA", 2980, 3000, "clip_end_minus", 0, "-"),
    ("chrA", 500, 500, "zero", 0, "+"),
    ("chrB", 10, 31, "clip_both", 0, "+"), ("chrB", 10, 31, "clip_both_minus", 0, "-"),
    ("chrA", 700, 800, "in_gap", 0, "."), ("chrA", 880, 920, "half_in_gap", 0, "-"),
    ("chrA", 1240, 1262, "overlapping_records", 0, "*"),
    ("chrN", 300, 400, "not_in_track", 0, "+"), ("chrB", 10, 10, "zero2", 0, "-"),
    ("chrA", 1700, 1800, "integers", 0, "-"), ("chrA", 3015, 3036, "all_padding", 0, "-"),   # centre 3025: window starts at 3000
    ("chrA", 2300, 2400, "late", 0, "+"), ("chrA", 1000, 1100, "repeat", 0, "+"),
]
BED_INT = [("chrA", 1600, 1700, "i1", 0, "+"), ("chrA", 1650, 1751, "i2", 0, "-"), ("chrA", 1800, 1900, "i3", 0, "+"),
           ("chrA", 2000, 2040, "i4", 0, "-"), ("chrA", 1530, 1541, "i5", 0, "+"), ("chrA", 2040, 2100, "i6", 0, "-"),
           ("chrA", 1800, 1900, "i3_again", 0, "-")]
BED_NEGATIVE = [("chrA", 3100, 3121, "past_end", 0, "+")]            # centre 3110: the window would start at 3085 > 3000
BED_MISSING = [("chrQ", 10, 20, "no_size", 0, "+")]

FLAGS = [("plain", 0, 0, 0), ("exp", 1, 0, 0), ("positive", 0, 1, 0), ("scale", 0, 0, 1), ("exp_positive_scale", 1, 1, 1)]
# name, up, down, strand, exp, positive, scale, all, no_agg, norm, bed (0 main, 1 integer)
CASES = [("%s_%s" % (n, "strand" if s else "nostrand"), 25, 25, s, e, p, sc, 1, 0, 0, 0) for s in (0, 6) for n, e, p, sc in FLAGS] + [
    ("norm_scale_strand_noall", 25, 25, 6, 0, 0, 1, 0, 0, 1, 0),
    ("noagg_all", 25, 25, 0, 0, 0, 0, 1, 1, 0, 0),
    ("one_column", 0, 0, 6, 0, 0, 0, 1, 0, 0, 0),
    ("up10_down30_strand", 10, 30, 6, 0, 0, 0, 1, 0, 0, 0),
    ("integers_plain_strand", 25, 25, 6, 0, 0, 0, 1, 0, 0, 1),
    ("integers_positive_strand", 25, 25, 6, 0, 1, 0, 1, 0, 0, 1),
]


class NoPool(object):
    def __init__(self, processes=None):
        pass

    def map(self, fn, items):
        return [fn(x) for x in items]

    def close(self):
        pass

    def join(self):
        pass


CAPTURE = {}


class NumpyKeepingMatrix(object):
    @staticmethod
    def savetxt(fname, X, *a, **k):
        if np.ndim(X) == 2:
            CAPTURE["mat"] = np.array(X, dtype=np.float64)
        return np.savetxt(fname, X, *a, **k)

    def __getattr__(self, k):
        return getattr(np, k)


def value_text(rng):
    r = rng.random()
    if r < 0.08:
        return "0"
    if r < 0.12:
        return "0.0"
    v = rng.normal(0.4, 1.2)
    return "%.5g" % v if rng.random() < 0.7 else "%.3f" % v


def make_track(rng):
    lines = []
    pos = 3                                     # the first bases of chrA have no record
    while pos < 3000:
        n = int(rng.integers(1, 10))
        end = min(pos + n, 3000)
        if GAP[0] <= pos < GAP[1]:
            pos = GAP[1]
            continue
        end = min(end, GAP[0]) if pos < GAP[0] else end
        if 1200 <= pos < 1300:
            lines += ["chrA\t1200\t1260\t1.5", "chrA\t1240\t1300\t-0.75"]
            pos = 1300
            continue
        end = min(end, 1200) if pos < 1200 else end
        if INT_RUN[0] <= pos < INT_RUN[1]:
            end = min(end, INT_RUN[1])
            v = int(rng.integers(-4, 9))
            text = ("%d" % v) if rng.random() < 0.6 else ("%d.0" % v)
        else:
            end = min(end, INT_RUN[0]) if pos < INT_RUN[0] else end
            text = value_text(rng)
        if rng.random() < 0.04 and not INT_RUN[0] <= pos < INT_RUN[1]:
            pos = end                           # a short hole: NaN inside otherwise covered windows
            continue
        lines.append("chrA\t%d\t%d\t%s" % (pos, end, text))
        pos = end
    for b, e, v in ((2, 9, "0.25"), (9, 10, "-1.5"), (12, 30, "2"), (30, 40, "-0.125")):
        lines.append("chrB\t%d\t%d\t%s" % (b, e, v))
    return "\n".join(lines) + "\n"


def bed_text(rows):
    return "".join("%s\t%d\t%d\t%s\t%d\t%s\n" % r for r in rows)


def write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return path


def namespace(bed, bg, sizes, out, up, down, strand, e, p, sc, al, no_agg, norm):
    return argparse.Namespace(bed=bed, bg=bg, sizes=sizes, out=out, cores=1, all=bool(al), no_agg=bool(no_agg), up=up, down=down,
                              weight=None, strand=strand or None, exp=bool(e), positive=bool(p), scale=bool(sc), norm=bool(norm))


def main():
    rng = np.random.default_rng(20261017)
    track = make_track(rng)
    bg = os.path.join(TMP, "track.bedgraph.gz")
    with gzip.open(bg, "wt") as f:
        f.write(track)
    sizes_text = "".join("%s\t%d\n" % s for s in SIZES)
    sizes = write(os.path.join(TMP, "genome.sizes"), sizes_text)
    beds = [write(os.path.join(TMP, "sites.bed"), bed_text(BED)), write(os.path.join(TMP, "sites_int.bed"), bed_text(BED_INT))]
    out = {"track_text": np.array(track), "sizes_text": np.array(sizes_text), "bed_text": np.array(bed_text(BED)),
           "bed_int_text": np.array(bed_text(BED_INT)), "bed_negative_text": np.array(bed_text(BED_NEGATIVE)),
           "bed_missing_text": np.array(bed_text(BED_MISSING))}
    SA.Pool = NoPool
    SA.np = NumpyKeepingMatrix()
    stdout = sys.stdout
    names = []
    for name, up, down, strand, e, p, sc, al, no_agg, norm, which in CASES:
        rows = [r for r in (BED_INT if which else BED) if r[2] - r[1] >= 1]
        a = namespace(beds[which], bg, sizes, os.path.join(TMP, name), up, down, strand, e, p, sc, al, no_agg, norm)
        for ext in (".tracks.txt.gz", ".agg.track.txt"):
            if os.path.exists(a.out + ext):
                os.remove(a.out + ext)
        CAPTURE.clear()
        SA.get_signal(a)
        K = up + down + 1
        if al:
            mat = CAPTURE["mat"]
            assert mat.shape == (len(rows), K), name
            with gzip.open(a.out + ".tracks.txt.gz", "rt") as f:
                text = f.read()
            assert len(text.splitlines()) == len(rows), name
            out["mat_" + name] = mat
            out["tracks_" + name] = np.frombuffer(gzip.compress(text.encode("ascii"), 9, mtime=0), np.uint8)
            if not which and not sc:
                assert np.isnan(mat).any() and (np.isnan(mat).all(axis=1)).sum() >= 2, name      # the gap and chrN rows
            if which:
                assert np.isfinite(mat).all() and np.array_equal(mat, np.round(mat)), name
        else:
            assert not os.path.exists(a.out + ".tracks.txt.gz"), name
        if no_agg:
            assert not os.path.exists(a.out + ".agg.track.txt"), name
        else:
            with open(a.out + ".agg.track.txt") as f:
                text = f.read()
            assert len(text.splitlines()) == K, name
            out["agg_" + name] = np.array(text)
        out["args_" + name] = np.array([up, down, strand, e, p, sc, al, no_agg, norm, which])
        names.append(name)
    out["cases"] = np.array(names)
    # the padding rule on the golden itself: clipped at both ends is padded on the left only; a window that starts at 0 unclipped is not
    m = out["mat_plain_nostrand"]
    kept = [r[3] for r in BED if r[2] - r[1] >= 1]
    both = m[kept.index("clip_both")]
    assert np.all(both[:11] == 0) and both[-1] != 0 and not np.isnan(both[-1]), both
    assert np.isnan(m[kept.index("starts_at_0_exactly")][:3]).all()          # bases 0..2 have no record: read, not padded
    assert np.all(m[kept.index("all_padding")] == 0)
    assert np.all(m[kept.index("overlapping_records")][25 - 11:25 + 9] == -0.75)  # centre 1251: columns of [1240, 1260)

    # where the reference raises
    sys.stdout = open(os.devnull, "w")
    try:
        for rows, exc in ((BED_NEGATIVE, ValueError), (BED_MISSING, KeyError)):
            bed = write(os.path.join(TMP, "bad.bed"), bed_text(rows))
            try:
                SA.get_signal(namespace(bed, bg, sizes, os.path.join(TMP, "bad"), 25, 25, 0, 0, 0, 0, 1, 0, 0))
            except exc:
                pass
            else:
                raise AssertionError("the reference did not raise %s on %r" % (exc.__name__, rows))
    finally:
        sys.stdout.close()
        sys.stdout = stdout
    dst = os.path.join(HERE, "pyatac_signal.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s: %d cases, %d bytes" % (dst, len(CASES), os.path.getsize(dst)))


if __name__ == "__main__":
    main()
