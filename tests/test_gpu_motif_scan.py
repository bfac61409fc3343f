"""The motif scan of one chromosome on the GPU (natac_motif_scan, csrc/natac_motifs.hpp; `pyatac motifs`) against the NumPy restatement
of tests/motifs_ref.py.  Everything the device decides is integer arithmetic, so every case is equality of all five arrays, dtypes
included, without a tolerance.

The constructed cases use consensus motifs: a count matrix with all 20 sites on one base per column scores 196 for the consensus base and
-470 for another (pseudocount 0.8, uniform background), so T = 196 W admits the perfect match alone, and a poly-A chromosome holds no
match but the planted ones."""
import ctypes as C
import functools

import numpy as np
import pytest

import motifs_ref as R

pytestmark = pytest.mark.gpu

MATCH, MISS = 196, -470


def _ctx():
    from nucleoatac_amd import get_context
    return get_context()


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def assert_same(got, want):
    assert len(got) == len(want) == 5
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), "array %d: %s != %s" % (k, a[:8], b[:8])


def both(seq, start, end, widths, S, T, want=None, **kw):
    """the device's answer, checked equal to the restatement's -> the restatement's"""
    want = R.scan(seq, start, end, widths, S, T) if want is None else want
    got = _ctx().motif_scan(seq, start, end, widths, S, T, **kw)
    assert_same(got, want)
    return want


def consensus(word):
    S = R.scores(np.array([[20.0 if b == c else 0.0 for b in "ACGT"] for c in word]))
    assert sorted(set(S.ravel().tolist())) == [MISS, MATCH]
    return S


def revcomp(word):
    return word[::-1].translate(str.maketrans("ACGT", "TGCA"))


def poly_a(n, plants):
    seq = bytearray(b"A" * n)
    for x, word in plants:
        seq[x:x + len(word)] = word.encode()
    return np.frombuffer(bytes(seq), np.uint8)


def one(word, T=None):
    S = consensus(word)
    return np.array([len(word)], np.int32), S, np.array([MATCH * len(word) if T is None else T], np.int32)


def test_constants():
    from nucleoatac_amd import _lib as L
    assert (L.MOTIF_MAX_WIDTH, L.MOTIF_MAX_MOTIFS, L.MOTIF_SCALE) == (R.MAX_WIDTH, R.MAX_MOTIFS, R.SCALE)
    assert (L.MOTIF_TILE, L.MOTIF_RUN_TILES, L.MOTIF_GROUP, L.MOTIF_FIRST_CAPACITY) == (R.TILE, R.RUN_TILES, R.GROUP, R.FIRST_CAPACITY)
    import os
    import re
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "natac.h")).read()
    for name in ("MAX_WIDTH", "MAX_MOTIFS", "SCALE", "TILE", "RUN_TILES", "GROUP", "FIRST_CAPACITY"):
        assert int(re.search(r"#define NATAC_MOTIF_%s (\d+)" % name, h).group(1)) == getattr(L, "MOTIF_" + name)


# ---- random chromosomes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(seed):
    n = 60000 - 7001 * seed
    seq = R.random_chromosome(seed, n)
    rng = np.random.default_rng(3000 + seed)
    widths = [1, 2, 31, 32, 33, 63, 64] + rng.integers(5, 33, 33).tolist()
    widths, S, T, thr = R.random_motifs(seed, widths, p=1e-3)
    assert thr[0][1] is None and thr[1][1] is None          # the two shortest motifs are unreachable at 1e-3
    length = rng.integers(50, 2001, 200)
    start = rng.integers(0, n - length)
    start[150:] = start[:50]                                  # repeated starts, some with another length
    length[150:175] = length[:25]                             # ... and 25 windows twice over
    windows = (start.astype(np.int64), (start + length).astype(np.int64))
    whole = R.scan(seq, None, None, widths, S, T)
    some = R.scan(seq, windows[0], windows[1], widths, S, T)
    return seq, widths, S, T, windows, whole, some


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_chromosome_whole(seed):
    seq, widths, S, T, _, whole, _ = random_case(seed)
    assert len(whole[0]) >= 1000 and set(whole[2].tolist()) == {0, 1}
    assert np.isin(seq, np.frombuffer(b"acgt", np.uint8)).sum() > 1000 and (seq == ord("N")).sum() >= 40
    both(seq, None, None, widths, S, T, want=whole)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_chromosome_windows(seed):
    seq, widths, S, T, (start, end), _, some = random_case(seed)
    assert len(some[0]) >= 1000 and some[4].shape == (200, 40) and some[4].sum() > len(some[0])      # overlapping windows count a site twice
    both(seq, start, end, widths, S, T, want=some)


# ---- constructed cases ------------------------------------------------------------------------------------------------------------
WORD = "GATTACAGGC"


def test_hits_flush_against_both_ends():
    n = 500
    seq = poly_a(n, [(0, WORD), (n - len(WORD), WORD), (200, revcomp(WORD))])
    want = both(seq, None, None, *one(WORD))
    assert want[1].tolist() == [0, 200, n - len(WORD)] and want[2].tolist() == [0, 1, 0] and want[3].tolist() == [MATCH * len(WORD)] * 3
    assert want[4].tolist() == [[3]]


def test_window_shorter_than_the_motif_and_empty_window():
    seq = poly_a(400, [(100, WORD)])
    want = both(seq, [100, 50, 399, 400], [100 + len(WORD) - 1, 50, 400, 400], *one(WORD))
    assert len(want[0]) == 0 and want[4].tolist() == [[0]] * 4
    want = both(seq, [100, 50], [100 + len(WORD), 50], *one(WORD))       # the window that just holds it
    assert want[1].tolist() == [100] and want[4].tolist() == [[1], [0]]


def test_hit_across_the_border_of_abutting_windows():
    seq = poly_a(400, [(100, WORD)])
    want = both(seq, [90, 103], [103, 130], *one(WORD))
    assert want[1].tolist() == [100] and want[4].tolist() == [[0], [0]]       # a site of the scan interval, inside neither window
    want = both(seq, [90, 104], [103, 130], *one(WORD))                       # one base between them: two scan intervals, no site
    assert len(want[0]) == 0


def test_hit_inside_two_overlapping_windows():
    seq = poly_a(400, [(100, WORD)])
    want = both(seq, [90, 95, 90], [120, 300, 120], *one(WORD))
    assert want[1].tolist() == [100] and want[4].tolist() == [[1], [1], [1]]


def test_n_inside_a_match_and_lower_case():
    bad = WORD[:4] + "N" + WORD[5:]
    seq = poly_a(600, [(100, bad), (200, WORD.lower()), (300, WORD[:5] + WORD[5:].lower()), (400, WORD[:4] + "R" + WORD[5:])])
    want = both(seq, None, None, *one(WORD))
    assert want[1].tolist() == [200, 300]
    want = both(seq, None, None, *one(WORD, T=MATCH * 9 + MISS))              # one mismatch admitted: still nothing over the N or the R
    assert want[1].tolist() == [200, 300]


def test_palindrome_hits_both_strands_plus_first():
    word = "GAATTC"
    assert revcomp(word) == word
    seq = poly_a(300, [(64, word), (130, word)])
    want = both(seq, None, None, *one(word))
    assert want[1].tolist() == [64, 64, 130, 130] and want[2].tolist() == [0, 1, 0, 1] and want[4].tolist() == [[4]]


def test_threshold_at_and_above_the_maximum():
    seq = poly_a(300, [(10, WORD), (100, WORD)])
    top = MATCH * len(WORD)
    assert both(seq, None, None, *one(WORD, T=top))[1].tolist() == [10, 100]
    assert len(both(seq, None, None, *one(WORD, T=top + 1))[0]) == 0


def test_threshold_at_the_minimum_hits_everywhere():
    n = 300
    seq = R.random_chromosome(7, n, n_N=0)
    widths, S, T = one(WORD, T=MISS * len(WORD))
    want = both(seq, None, None, widths, S, T)
    assert len(want[0]) == 2 * (n - len(WORD) + 1) and want[4].tolist() == [[2 * (n - len(WORD) + 1)]]


@functools.lru_cache(maxsize=None)
def dense_case(n=5000, n_motifs=6, p=0.05):
    """many hits per tile: loose thresholds on a random chromosome"""
    seq = R.random_chromosome(11, n, n_N=20)
    widths, S, T, _ = R.random_motifs(11, [6, 9, 12, 17, 33, 40][:n_motifs], p=p)
    return seq, widths, S, T


def test_window_starts_on_both_sides_of_every_border():
    seq, widths, S, T = dense_case()
    starts, ends = [], []
    for border in (R.TILE, 2 * R.TILE, R.TILE * R.RUN_TILES, 2 * R.TILE * R.RUN_TILES, 3 * R.TILE * R.RUN_TILES + R.TILE):
        for d in (-1, 0, 1):
            starts += [border + d, border + d - 45]
            ends += [border + d + 70, border + d]              # windows that begin there and windows that end there
    want = both(seq, starts, ends, widths, S, T)
    assert len(want[0]) > 200
    want = both(seq, None, None, widths, S, T)                  # every tile and run border inside one interval
    assert len(want[0]) > 2000 and want[1].max() > 3 * R.TILE * R.RUN_TILES


def test_sparse_windows_runs_of_scattered_tiles():
    seq, widths, S, T = dense_case()
    starts = np.arange(7, 4900, 150)                            # 33 windows of 30 bases, 150 apart: the listed tiles are not neighbours
    want = both(seq, starts, starts + 30, widths, S, T)
    assert len(want[0]) > 50


@pytest.mark.parametrize("max_counters", [13, 8, 1])
def test_longer_runs_when_the_counters_would_be_too_many(monkeypatch, max_counters):
    # 79 tiles and 6 motifs: 5 runs of 16 tiles are 30 counters; a bound of 13 doubles the run twice (2 runs of 64), 8 and 1 make one run
    seq, widths, S, T = dense_case()
    want = R.scan(seq, None, None, widths, S, T)
    monkeypatch.setenv("NATAC_MOTIF_MAX_COUNTERS", str(max_counters))
    both(seq, None, None, widths, S, T, want=want)
    starts = np.arange(7, 4900, 150)
    both(seq, starts, starts + 30, widths, S, T)


def test_one_more_motif_than_a_group():
    seq = R.random_chromosome(12, 3000)
    rng = np.random.default_rng(5)
    widths, S, T, _ = R.random_motifs(12, rng.integers(6, 11, R.GROUP + 1).tolist(), p=1e-2)
    want = both(seq, None, None, widths, S, T)
    assert len(want[0]) > 1000 and (want[0] == R.GROUP).sum() > 0 and (want[0] == R.GROUP - 1).sum() > 0


def test_tables_past_one_group_of_lds():
    # 20 motifs of 64 columns with int32 accumulators are 20 * 512 dwords: more than the 8,192 a group's tables may take
    seq = R.random_chromosome(13, 2000)
    rng = np.random.default_rng(6)
    S = np.where(rng.random((20 * 64, 4)) < 0.25, 200, -1500).astype(np.int32)
    S[np.arange(20 * 64), rng.integers(0, 4, 20 * 64)] = 200
    T = np.full(20, -60000, np.int32)
    want = both(seq, None, None, np.full(20, 64, np.int32), S, T)
    assert len(want[0]) > 500 and len(set(want[0].tolist())) == 20


def test_both_accumulator_arms_in_one_call():
    seq = R.random_chromosome(14, 4000)
    rng = np.random.default_rng(7)
    big = np.full((64, 4), -1500, np.int32)
    big[np.arange(64), rng.integers(0, 4, 64)] = 200
    assert int(big.min(axis=1).sum()) < -32768 and int((big.max(axis=1) - big.min(axis=1)).sum()) > 65535       # needs int32 sums
    small = consensus(WORD)
    edge_fits = np.array([[0, 30000, 1, 2], [0, 30000, 5, 6], [0, 5535, 3, 4]], np.int32)      # spreads sum to 65,535: the halves' limit
    edge_over = np.array([[0, 30000, 1, 2], [0, 30000, 5, 6], [0, 5536, 3, 4]], np.int32)      # 65,536: one too many
    neg = np.array([[-20000, -1, -7, -3]] * 3, np.int32)                                       # sums far below zero, spread 59,997
    widths = np.array([64, len(WORD), 3, 3, 3], np.int32)
    S = np.concatenate([big, small, edge_fits, edge_over, neg])
    T = np.array([-62000, MATCH * 4 + MISS * 6, 60000, 60000, -20010], np.int32)
    want = both(seq, None, None, widths, S, T)
    per = np.bincount(want[0], minlength=5)
    assert per.min() > 20, per
    assert want[3][want[0] == 0].min() < -32768 and want[3][want[0] == 2].max() == 65535 and want[3][want[0] == 3].max() == 65536


def raw_scan(seq, n, nw, start, end, nm, widths, S, T, capacity, outs, counts, n_hits, ms):
    from nucleoatac_amd import _lib as L
    return L.load().natac_motif_scan(_ctx()._h, _vp(seq), n, nw, _vp(start), _vp(end), nm, _vp(widths), _vp(S), _vp(T),
                                     None if n_hits is None else C.byref(n_hits), capacity, *[_vp(o) for o in outs], _vp(counts),
                                     None if ms is None else C.byref(ms))


def sentinels(cap, shape):
    outs = [np.full(cap, -7, np.int32), np.full(cap, -7, np.int64), np.full(cap, 7, np.uint8), np.full(cap, -7, np.int32)]
    return outs, np.full(shape, -7, np.int32), C.c_int64(-7), C.c_double(-7.0)


def test_more_hits_than_the_capacity(monkeypatch):
    seq, widths, S, T = dense_case()
    want = R.scan(seq, [0, 100], [5000, 900], widths, S, T)
    total = len(want[0])
    assert total > 2000
    st, en = np.array([0, 100], np.int64), np.array([5000, 900], np.int64)
    # the raw call with too little room: the count and the matrix are written, the four arrays stay as they were
    outs, counts, n_hits, ms = sentinels(1000, (2, len(widths)))
    assert raw_scan(seq, len(seq), 2, st, en, len(widths), widths, S, T, 1000, outs, counts, n_hits, ms) == 0
    assert n_hits.value == total and np.array_equal(counts, want[4]) and ms.value > 0
    assert all((o == (7 if o.dtype == np.uint8 else -7)).all() for o in outs)
    # with exactly enough room
    outs, counts, n_hits, ms = sentinels(total, (2, len(widths)))
    assert raw_scan(seq, len(seq), 2, st, en, len(widths), widths, S, T, total, outs, counts, n_hits, None) == 0
    assert_same(tuple(outs) + (counts,), want)
    # the binding comes again: a small first capacity as an argument, and as the environment's first guess
    both(seq, st, en, widths, S, T, want=want, capacity=10)
    both(seq, st, en, widths, S, T, want=want, capacity=0)
    monkeypatch.setenv("NATAC_MOTIF_FIRST_CAPACITY", "64")
    got = _ctx().motif_scan(seq, st, en, widths, S, T, with_kernel_ms=True)
    assert_same(got[:5], want)
    assert got[5] > 0


def test_two_calls_give_the_same_bytes():
    seq, widths, S, T, (start, end), _, _ = random_case(1)
    a = _ctx().motif_scan(seq, start, end, widths, S, T)
    b = _ctx().motif_scan(seq, start, end, widths, S, T)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_nothing_to_do():
    seq = poly_a(200, [(50, WORD)])
    widths, S, T = one(WORD)
    got = _ctx().motif_scan(seq, [], [], widths, S, T)
    assert [len(x) for x in got[:4]] == [0] * 4 and got[4].shape == (0, 1)
    got = _ctx().motif_scan(seq, [0, 10], [200, 100], [], np.zeros((0, 4), np.int32), [])
    assert [len(x) for x in got[:4]] == [0] * 4 and got[4].shape == (2, 0)
    got = _ctx().motif_scan(seq, [60, 0], [60, 0], widths, S, T)              # only empty windows: no scan interval
    assert [len(x) for x in got[:4]] == [0] * 4 and got[4].tolist() == [[0], [0]]


# ---- refusals: operand checks on the host, every output untouched, the context usable afterwards ---------------------------------------
def test_refusals():
    from nucleoatac_amd import _lib as L
    seq = poly_a(300, [(50, WORD)])
    widths, S, T = one(WORD)
    st, en = np.array([0], np.int64), np.array([300], np.int64)
    wide65 = (np.array([65], np.int32), np.zeros((65, 4), np.int32), np.array([0], np.int32))
    zero_w = (np.array([0], np.int32), np.zeros((1, 4), np.int32), np.array([0], np.int32))
    many = (np.ones(R.MAX_MOTIFS + 1, np.int32), np.zeros((R.MAX_MOTIFS + 1, 4), np.int32), np.zeros(R.MAX_MOTIFS + 1, np.int32))
    over = (np.array([2], np.int32), np.array([[2 ** 31 - 1, 0, 0, 0], [1, 0, 0, 0]], np.int32), np.array([0], np.int32))
    under = (np.array([2], np.int32), np.array([[-2 ** 31, 0, 0, 0], [-1, 0, 0, 0]], np.int32), np.array([0], np.int32))
    cases = {
        "width 65": dict(m=wide65), "width 0": dict(m=zero_w), "4097 motifs": dict(m=many),
        "sums above int32": dict(m=over), "sums below int32": dict(m=under),
        "null seq": dict(seq=None), "null start": dict(st=None), "null end": dict(en=None),
        "null widths": dict(m=(None, S, T)), "null scores": dict(m=(widths, None, T)), "null thresholds": dict(m=(widths, S, None)),
        "null hit arrays": dict(null_out=True), "null counts": dict(null_counts=True),
        "window past the end": dict(en=np.array([301], np.int64)), "negative start": dict(st=np.array([-1], np.int64)),
        "end before start": dict(st=np.array([20], np.int64), en=np.array([19], np.int64)),
        "n = 0": dict(n=0), "n = 2^31": dict(n=2 ** 31), "negative capacity": dict(cap=-1), "negative windows": dict(nw=-1),
    }
    for name, kw in cases.items():
        w, s, t = kw.get("m", (widths, S, T))
        outs, counts, n_hits, ms = sentinels(16, (1, 1))
        use_outs = [None] * 4 if kw.get("null_out") else outs
        rc = raw_scan(kw.get("seq", seq), kw.get("n", 300), kw.get("nw", 1), kw.get("st", st), kw.get("en", en),
                      len(w) if w is not None else 1, w, s, t, kw.get("cap", 16), use_outs, None if kw.get("null_counts") else counts,
                      n_hits, ms)
        assert rc == -1, name          # NATAC_E_ARG
        assert len(L.load().natac_last_error()) > 0
        assert n_hits.value == -7 and ms.value == -7.0 and (counts == -7).all(), name
        assert all((o == (7 if o.dtype == np.uint8 else -7)).all() for o in outs), name
    # a NULL n_hits is refused too
    outs, counts, _, ms = sentinels(16, (1, 1))
    assert raw_scan(seq, 300, 1, st, en, 1, widths, S, T, 16, outs, counts, None, ms) == -1 and (counts == -7).all()
    # the context is as usable as before
    assert both(seq, None, None, widths, S, T)[1].tolist() == [50]
