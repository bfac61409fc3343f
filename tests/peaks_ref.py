"""The rule of `pyatac peaks` (natac_enriched_regions, include/natac.h) restated in NumPy: bincount, cumsum, clipped differences,
flatnonzero.  Written from the rule's text, not from the kernels; the device must agree with it exactly, in every array."""
import functools
import os
import re

import numpy as np
from scipy.special import gammaincinv

K_TABLE = 65536
_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "natac.h")).read()
SEGMENT, SHORT_MAX, FIRST_CAPACITY, MAX_WINDOW = (int(re.search(r"#define NATAC_PEAKS_%s (\d+)" % k, _HDR).group(1))
                                                  for k in ("SEGMENT_DEFAULT", "SHORT_MAX", "FIRST_CAPACITY", "MAX_WINDOW"))
OPEN = np.full(64, 2 ** 31 - 1, np.int32)    # a table that admits every count
SCAN_TRIP = 1024 * 2048                      # elements a prefix scan covers in one trip of its block sums (natac_textz.hpp)


def critical_rates(mlog10p, n_table=K_TABLE):
    """Lam[k]: the largest rate at which a Poisson count reaches k with probability at most 10^-mlog10p (Lam[0] = 0)"""
    lam = np.zeros(n_table, np.float64)
    lam[1:] = gammaincinv(np.arange(1, n_table, dtype=np.float64), 10.0 ** -float(mlog10p))
    return lam


def tables(h, S, L, mlog10p, n_table=K_TABLE):
    """(Lam, thr_small int32, thr_large int32)"""
    lam = critical_rates(mlog10p, n_table)
    top = 2 ** 31 - 1           # no count reaches it (fewer than 2^30 records a call), so the clip changes no verdict
    return (lam, np.minimum(np.floor(lam * (2 * S + 1) / (2 * h + 1)), top).astype(np.int32),
            np.minimum(np.floor(lam * (2 * L + 1) / (2 * h + 1)), top).astype(np.int32))


def min_pileup(lam, lam_g):
    """max(1, the smallest k with Lam[k] >= lam_g); None when no k of the table has"""
    k = int(np.searchsorted(lam, lam_g, "left"))
    return None if k >= len(lam) else max(1, k)


def insertions(pos, tlen, n):
    """the kept insertions of one chromosome of length n (either end is dropped on its own outside [0, n))"""
    pos, tlen = np.asarray(pos, np.int64), np.asarray(tlen, np.int64)
    x = np.concatenate([pos + 4, pos + tlen - 5])
    return x[(x >= 0) & (x < n)]


def window_counts(cum, n, w):
    """C_w(x) for every base, cum = the insertions in [0, j)"""
    x = np.arange(n, dtype=np.int64)
    return cum[np.minimum(x + w + 1, n)] - cum[np.maximum(x - w, 0)]


def enriched_regions(pos, tlen, n, h, S, L, max_gap, min_length, min_pile, thr_small, thr_large, counts=False):
    """(start, end, summit int64; pileup, n_small, n_large int32) of the kept regions, ascending; counts: also (regions before the
    length rule, significant bases)"""
    cum = np.concatenate([[0], np.cumsum(np.bincount(insertions(pos, tlen, n), minlength=n))]).astype(np.int64)
    p, s, g = (window_counts(cum, n, w) for w in (h, S, L))
    k = np.minimum(p, len(thr_small) - 1)
    sig = np.flatnonzero((p >= min_pile) & (s <= np.asarray(thr_small, np.int64)[k]) & (g <= np.asarray(thr_large, np.int64)[k]))
    out = [[] for _ in range(6)]
    found = 0
    if len(sig):
        cut = np.flatnonzero(np.diff(sig) - 1 > max_gap)          # more than max_gap non-significant bases in between
        first = sig[np.concatenate([[0], cut + 1])]
        last = sig[np.concatenate([cut, [len(sig) - 1]])]
        found = len(first)
        for a, b in zip(first.tolist(), last.tolist()):
            if b + 1 - a < min_length:
                continue
            top = a + np.flatnonzero(p[a:b + 1] == p[a:b + 1].max())
            c = int(top[0] + top[-1]) // 2
            for o, v in zip(out, (a, b + 1, c, p[c], s[c], g[c])):
                o.append(int(v))
    res = tuple(np.asarray(o, t) for o, t in zip(out, (np.int64,) * 3 + (np.int32,) * 3))
    return res + (found, len(sig)) if counts else res


def hotspot_chromosome(seed, n=60000, n_uniform=3000, hotspots=5, per_hotspot=400, spread=60, flush=True):
    """sorted (pos, tlen) of a chromosome with planted hotspots; flush: the first and the last one lie against the chromosome's ends"""
    rng = np.random.RandomState(seed)
    centres = rng.randint(n // 10, n - n // 10, hotspots)
    if flush and hotspots >= 2:
        centres[0], centres[-1] = 40, n - 40
    pos = [rng.randint(-50, n - 20, n_uniform)]
    for c in centres:
        pos.append(c + rng.randint(-spread, spread + 1, per_hotspot) - 60)
    pos = np.sort(np.concatenate(pos)).astype(np.int64)
    tlen = rng.randint(30, 220, len(pos)).astype(np.int64)
    return pos, tlen


def spike_chromosome(seed, n=20000, n_uniform=1000, spikes=6, per_spike=30):
    """sorted (pos, tlen) with point hotspots (every l of a spike at one base, some two and three bases further on): what the small
    geometry (h = 2, S = 5, L = 20) finds improbable"""
    rng = np.random.RandomState(seed)
    pos = [rng.randint(-20, n - 10, n_uniform)]
    for c in rng.randint(100, n - 100, spikes):
        pos.append(np.full(per_spike, c - 4) + rng.choice([0, 0, 0, 0, 2, 3], per_spike))
    pos = np.sort(np.concatenate(pos)).astype(np.int64)
    return pos, rng.randint(30, 220, len(pos)).astype(np.int64)


# ---- constructed cases (tests/test_gpu_enriched_regions*.py run them on the device, tests/test_peaks_host.py checks that each reaches
# the arm it is built for).  A case is (pos, tlen, n, geom, min_pileup, thr_small, thr_large), geom = (h, S, L, max_gap, min_length) ------
def at(xs, n):
    """records whose l are the sorted bases xs and whose r lies past the chromosome's end"""
    xs = np.ascontiguousarray(xs, dtype=np.int64)
    assert np.all(np.diff(xs) >= 0)
    return xs - 4, np.full(len(xs), n + 100, np.int64)


def real_tables(pos, tlen, n, h, S, L, q):
    """(min_pileup, thr_small, thr_large) as `pyatac peaks` derives them for one chromosome"""
    lam, ts, tl = tables(h, S, L, q)
    return min_pileup(lam, (2 * h + 1.0) * len(insertions(pos, tlen, n)) / n), ts, tl


def regions_of(case, counts=True):
    p, t, n, g, mp, ts, tl = case
    return enriched_regions(p, t, n, g[0], g[1], g[2], g[3], g[4], mp, ts, tl, counts=counts)


def run_xs(first, last):
    """insertions at every other base that make, with half_width 1 and min_pileup 1, exactly the bases first..last significant
    (p = 1 on an insertion, 2 between two)"""
    assert last - first >= 2
    xs = list(range(first + 1, last, 2))
    if xs[-1] != last - 1:
        xs.append(last - 1)
    return xs


def pieces(start, end, n, seg):
    """per segment of seg bases: the lengths of the regions' parts inside it, in region order"""
    out = []
    for s0 in range(0, n, seg):
        s1 = min(n, s0 + seg)
        out.append([int(min(e, s1) - max(a, s0)) for a, e in zip(start.tolist(), end.tolist()) if a < s1 and e > s0])
    return out


# -- 1. several default segments, a construction across every border of the scans' trips and of the segments
BORDERS_N = 9_500_000


def scan_borders(n=BORDERS_N, seg=None, large=1):
    """(hist, verdict, segment): the bases at which the insertion histogram's scan starts another trip (dense offset d0 + t * SCAN_TRIP of
    a segment's dense range [d0, d1) = [s0 - large, s1 + large) clipped), those at which the verdicts' scan does (s0 + t * SCAN_TRIP), and
    the first bases of the segments behind the first"""
    seg = seg or SEGMENT
    hist, verdict, segment = [], [], []
    for s0 in range(0, n, seg):
        s1 = min(n, s0 + seg)
        d0, d1 = max(0, s0 - large), min(n, s1 + large)
        hist += list(range(d0 + SCAN_TRIP, d1, SCAN_TRIP))
        verdict += list(range(s0 + SCAN_TRIP, s1, SCAN_TRIP))
        if s0:
            segment.append(s0)
    return hist, verdict, segment


def border_case(max_gap, kind):
    """-> (case, spots).  Geometry (1, 1, 1, max_gap, 1), every table entry open, min_pileup 1: one insertion every 1000 bases (more
    regions than the first capacity), and at every border B of scan_borders (a histogram border is B or B - 1 of a verdict or segment
    border at large = 1) one construction, spots = [(B, what, [(start, end), ...] expected there)]:
      joined  two runs with exactly max_gap other bases between them: one region
      split   the same with max_gap + 1 bases between them: two regions.  In both the later run starts on a base x with
              x - max_gap - 1 < B <= x: the bases before x that decide whether x starts a region lie on both sides of the border
      dense   one run across B, longer behind it than before it (its summit is not at the border)
    dense at the verdict borders comes with a region that ends on the last base before the first segment border and one that starts on
    the first base behind the second."""
    n, g = BORDERS_N, max_gap
    _, verdict, segment = scan_borders(n)
    xs, spots = list(range(900, n, 1000)), []             # (the borders lie at 152, 304, 456 and 608 of their thousands)
    for B in sorted(verdict + segment):
        what = kind
        if kind == "dense" and B in segment:
            what = "ends" if B == segment[0] else "starts"
        g0 = B - (g + (2 if what == "split" else 1)) // 2          # the first base of the gap
        if what == "joined":
            xs += run_xs(g0 - 31, g0 - 1) + run_xs(g0 + g, g0 + g + 40)
            want = [(g0 - 31, g0 + g + 41)]
        elif what == "split":
            xs += run_xs(g0 - 31, g0 - 1) + run_xs(g0 + g + 1, g0 + g + 41)
            want = [(g0 - 31, g0), (g0 + g + 1, g0 + g + 42)]
        elif what == "dense":
            xs += run_xs(B - 11, B + 41)
            want = [(B - 11, B + 42)]
        elif what == "ends":
            xs += run_xs(B - 31, B - 1)
            want = [(B - 31, B)]
        else:
            xs += run_xs(B, B + 40)
            want = [(B, B + 41)]
        spots.append((B, what, want))
    pos, tlen = at(np.sort(np.asarray(xs, np.int64)), n)
    return (pos, tlen, n, (1, 1, 1, g, 1), 1, OPEN, OPEN), spots


BORDER_CASES = [(0, "joined"), (0, "split"), (7, "joined"), (7, "split"), (7, "dense")]       # (at max_gap 0 joined is dense)


@functools.lru_cache(maxsize=None)
def border_case_with_answer(max_gap, kind):
    """(case, spots, the restatement's answer): computed once a process, never changed"""
    case, spots = border_case(max_gap, kind)
    return case, spots, regions_of(case)


# -- 2. long pieces (above SHORT_MAX bases of one region in one segment) in several segments
def long_piece_cases():
    """three chromosomes for a segment of 3000: region A = [2500, 14300) has the pieces 500, 3000, 3000, 3000, 2300, region B =
    [15500, 21500) has 2500, 3000, 500; short regions lie in the segments of A's first and last piece and of B's first and last, and
    nothing else in 3000..12000.  Three extra insertions on a base between two of a run's make p = 5 there and 4 beside it:
      0  A's summit in its short first piece, B's in its long first piece
      1  A's in a long middle piece, B's in its long middle piece
      2  A has two such bases, in its short first piece and in a long later one (the summit 6350 between them has p = 2), B's summit in
         its short last piece"""
    n = 23_500
    base = [1000] + run_xs(2500, 14299) + [14700, 15100] + run_xs(15500, 21499) + [22000]
    tops = [([2700], [16000]), ([7000], [19000]), ([2700, 10000], [21200])]
    cases, summits = [], []
    for ta, tb in tops:
        pos, tlen = at(np.sort(np.asarray(base + (ta + tb) * 3, np.int64)), n)
        cases.append((pos, tlen, n, (1, 1, 1, 0, 1), 1, OPEN, OPEN))
        summits.append((sum(ta) // len(ta), tb[0]))
    return cases, summits


def piece_limit_case():
    """-> (case, [(start, end, summit)]).  Regions of exactly SHORT_MAX - 1, SHORT_MAX and SHORT_MAX + 1 bases, five of each, on one
    chromosome; geometry (1, 1, 1, 0, 1), open tables, min_pileup 3.  One insertion on every base of [a - 1, b + 1] makes p = 3 on a..b
    and 2 on a - 1 and b + 1.  The counts 2, 0, 10, 0, 1, 2 on a - 1 .. a + 4 make p = 12 on a alone (2 on a - 1; 10, 11, 3, 4 behind a),
    mirrored for b; three more insertions on each of a + o - 1 .. a + o + 1 make p = 12 on a + o alone.  The highest pileup lies on the
    first base, the last, base 63, base 64 (either side of the first lane's second turn), and on the first and the last as equals."""
    head = [2, 0, 10, 0, 1, 2]
    lengths, places = (SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1), ("first", "last", 63, 64, "both")
    n = 1000 + 3000 * len(lengths) * len(places)
    c = np.zeros(n, np.int64)
    want = []
    for i, (ln, place) in enumerate((ln, place) for ln in lengths for place in places):
        a = 1000 + 3000 * i
        b = a + ln - 1
        c[a - 1:b + 2] = 1
        if place in ("first", "both"):
            c[a - 1:a + 5] = head
        if place in ("last", "both"):
            c[b - 4:b + 2] = head[::-1]
        if isinstance(place, int):
            c[a + place - 1:a + place + 2] += 3
        want.append((a, b + 1, a + place if isinstance(place, int) else {"first": a, "last": b, "both": (a + b) // 2}[place]))
    pos, tlen = at(np.repeat(np.arange(n, dtype=np.int64), c), n)
    return (pos, tlen, n, (1, 1, 1, 0, 1), 3, OPEN, OPEN), want


# -- 3. the reach: which records the two searches of a dense range (and of a summit's windows) take
REACH_SEGMENT = 1000


def reach_case(drop=()):
    """Geometry (2, 5, 20, 0, 1), 6000 bases, for a segment of 1000; thr_large[k] = k but for thr_large[7] = 8, min_pileup 3.  k records
    with l on one base make p = k on five bases, significant while no other insertion lies within 20 bases (one other at k = 7).  Their
    r and every insertion of the random records (tlen 30..220) stay out of the zones around them.
      "far+"   pos -15, tlen 5000: before every other record; its l is dropped, its r = 4980 is the first base of the dense range of
               segment [5000, 6000): 5 records on 5000 lose 4998..5000 to it, and 7 records on 4960 have it at distance 20 of the summit
      "far-"   pos 6024, tlen -3000: behind every other record; its r = 3019 is the last base of the dense range of [2000, 3000):
               5 records on 2999 lose 2999..3001 to it, and 7 on 3039 have it at distance 20 of the summit
      "zero"   pos 4017, tlen 0 (l = 4021, r = 4012): 5 records on 4000 lose every base
    drop: the names of those to leave out."""
    n = 6000
    rng = np.random.RandomState(11)
    pos, tlen = rng.randint(-10, n, 400).astype(np.int64), rng.randint(30, 221, 400).astype(np.int64)
    keep = np.ones(len(pos), bool)
    for a, b in ((2950, 3090), (3950, 4050), (4910, 5050)):
        for x in (pos + 4, pos + tlen - 5):
            keep &= (x < a) | (x > b)
    pos, tlen = [pos[keep]], [tlen[keep]]
    for x, k in ((2999, 5), (3039, 7), (4000, 5), (4960, 7), (5000, 5)):
        pos.append(np.full(k, x - 4, np.int64))
        tlen.append(150 + 11 * np.arange(k, dtype=np.int64))
    for name, p, t in (("far+", -15, 5000), ("far-", 6024, -3000), ("zero", 4017, 0)):
        if name not in drop:
            pos.append(np.asarray([p], np.int64))
            tlen.append(np.asarray([t], np.int64))
    pos, tlen = np.concatenate(pos), np.concatenate(tlen)
    order = np.argsort(pos, kind="stable")
    tl = np.arange(64, dtype=np.int32)
    tl[7] = 8
    return (pos[order], tlen[order], n, (2, 5, 20, 0, 1), 3, OPEN, tl)


# -- 4. more records in one dense range than one trip of the histogram's grid takes
GRID_RECORDS = 65536 * 256                   # the histogram's grid cap times its workgroup


def grid_stride_case(tail=True):
    """2^24 records with pos evenly over 98,020 bases (171 a base; six times the records of 18 bases moved onto one: spikes) and random
    tlen 30..220, then (tail) 1000 records with l = 99,500 and r within three bases of it, where no other record reaches.  Geometry
    (2, 5, 20, 3, 1), tables and min_pileup as `pyatac peaks` makes them at mlog10p 2 (of the whole case, with or without the tail)."""
    n, n0 = 100_000, GRID_RECORDS
    pos = np.arange(n0, dtype=np.int64) * 98_020 // n0 - 20
    for c in (5_000, 21_013, 40_000, 55_555, 70_001, 90_000):
        pos[(pos >= c - 13) & (pos < c + 5)] = c - 4
    tlen = np.random.RandomState(4).randint(30, 221, n0).astype(np.int64)
    assert pos[-1] + tlen.max() - 5 < 99_500 - 20 - 2
    pos = np.concatenate([pos, np.full(1000, 99_496, np.int64)])
    tlen = np.concatenate([tlen, 10 + np.arange(1000, dtype=np.int64) % 3])
    tables_ = real_tables(pos, tlen, n, 2, 5, 20, 2)
    if not tail:
        pos, tlen = pos[:n0], tlen[:n0]
    return (pos, tlen, n, (2, 5, 20, 3, 1)) + tables_


# -- 5. the far end of the coordinates and the widest window
def shifted(case, d):
    """the same chromosome d bases further on; with no insertion (kept or dropped) before base `large` the answer moves by d as well"""
    pos, tlen, n, geom = case[:4]
    assert (pos + 4).min() > geom[2] and d >= 0
    return (pos + d, tlen, n + d) + tuple(case[3:])


def shift_answer(ans, d):
    return tuple(a + d for a in ans[:3]) + tuple(ans[3:])


def far_end_case():
    """40,000 bases at the default geometry: hotspots, the last one flush against the end, and nothing before base 5,075"""
    n = 40_000
    pos, tlen = hotspot_chromosome(7, n=n, n_uniform=2000)
    keep = pos + 4 > 5075
    pos, tlen = pos[keep], tlen[keep]
    return (pos, tlen, n, (75, 500, 5000, 75, 150)) + real_tables(pos, tlen, n, 75, 500, 5000, 5)


def wide_window_cases():
    """120,000 bases (less than 2 * MAX_WINDOW) with hotspots, large = MAX_WINDOW.  With small = half_width no Poisson table admits
    anything, so the tables are made by hand from the chromosome's own counts:
      0  (1, 1, large): open thr_small, every thr_large[k] = T, the median count within large of the bases with p >= 3
      1  the same with a table of two entries, the smallest allowed
      2  (large, large, large), two entries: significant where min_pileup = the median p <= p <= its ninth decile"""
    n, L = 120_000, MAX_WINDOW
    pos, tlen = hotspot_chromosome(8, n=n, n_uniform=3000)
    cum = np.concatenate([[0], np.cumsum(np.bincount(insertions(pos, tlen, n), minlength=n))]).astype(np.int64)
    p, g = window_counts(cum, n, 1), window_counts(cum, n, L)
    T = int(np.median(g[p >= 3]))
    lo, hi = int(np.median(g)), int(np.percentile(g, 90))
    i32 = lambda v: np.asarray(v, np.int32)
    return [(pos, tlen, n, (1, 1, L, 3, 1), 3, OPEN, np.full(64, T, np.int32)),
            (pos, tlen, n, (1, 1, L, 3, 1), 3, i32([0, 2 ** 31 - 1]), i32([0, T])),
            (pos, tlen, n, (L, L, L, 0, 1), lo, i32([0, hi]), i32([0, hi]))]
