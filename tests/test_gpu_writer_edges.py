"""GPU: the device track writer where the pipeline's own tracks never take it (inputs: tests/writer_cases.py, fed through
DeviceBatch.set_track; no fragments, no model beyond the context).

A. natac_store_adopt (natac_text::round12 / tz_as_written) against the text round trip, bit for bit, on values at the edges of the
   twelve-digit rounding; the values it must refuse.
B. the stored-member arm of tz_emit_members: members whose Huffman payload would pass 64 KiB.
C. member borders at every column of a line, texts of chosen lengths, degenerate texts."""
import gzip
import io
import zlib

import numpy as np
import pytest

import writer_cases as W
from nucleoatac_amd import _lib as L
from nucleoatac_amd.pyatac.tracks import _py2_float_str as f2s
from nucleoatac_amd.writer import BGZF_EOF, TbiBuilder, bgzf_lines_host, tabix_index, write_bedgraph

pytestmark = pytest.mark.gpu

BLK = W.BLK
MODES = ((True, False), (False, False), (True, True), (False, True))      # (write_zero, keep_runs_before_nan)


@pytest.fixture(scope="module")
def ctx():
    from nucleoatac_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _native_text(tmp_path, chroms, pk, vals, **kw):
    p = str(tmp_path / "native.bedgraph")
    write_bedgraph(p, chroms, pk.chunk_start, pk.out_off, vals, compress=0, **kw)
    return open(p, "rb").read()


def _inflate(z):
    return gzip.GzipFile(fileobj=io.BytesIO(z + BGZF_EOF)).read()


def _check_writer(b, tmp_path, pk, chroms, vals, track=L.T_SMOOTH):
    """the checks of every case of part C: device text == native writer's text in every mode; members == host restatement;
    gzip inflates them to the text.  Returns (default-mode text, its members)."""
    for wz, keep in MODES:
        text, info = b.format_track(track, chroms, pk.chunk_start, write_zero=wz, keep_runs_before_nan=keep, compress=False)
        want = _native_text(tmp_path, chroms, pk, vals, write_zero=wz, keep_runs_before_nan=keep)
        assert info["hard"] == 0 and text.tobytes() == want, (wz, keep)
        assert info["text_bytes"] == len(want) and info["lines"] == want.count(b"\n")
    text = _native_text(tmp_path, chroms, pk, vals)
    z, zi = b.format_track(track, chroms, pk.chunk_start, compress=True)
    z = z.tobytes()
    assert zi["text_bytes"] == len(text)
    assert z == bgzf_lines_host(text)
    assert _inflate(z) == text
    return text, z


# ---- A -------------------------------------------------------------------------------------------------------------------
def test_adopted_values_are_the_text_round_trip_at_the_rounding_edges(ctx):
    """~200,000 values whose twelve-digit decimal exponent lies in [-11, 33] (writer_cases.in_range_values): every power of ten from 1e-11
    to 1e33 and k x 10^j (k = 1..9) with both neighbouring doubles; exact ties in the 13th digit below 1e12 with an odd and with an even
    12th digit; 9.999999999995 x 10^j (the rounding carries into the next exponent; 999999999999.5 -> 1e12, 9.999999999995e-12 ->
    1e-11); 9.99999999999e33; integers up to 2^53; random mantissas over every binary exponent of the range; all negated; runs that mix
    +0.0 and -0.0; +-inf; NaN runs of 1..60 bases inside chunks, at chunk starts, at chunk ends, whole chunks; equal runs directly
    before a NaN.  For all four write_zero x keep_runs_before_nan modes the adopted array equals, bit for bit (-0.0 != +0.0, NaN exactly where
    no line is), (1) the parse of the device's own text and (2) Track.write_track's run rule restated in numpy over float('%.12g' % v)."""
    from nucleoatac_amd.device import TrackStore
    assert "%.12g" % 9.999999999995e-12 == "1e-11" and "%.12g" % 999999999999.5 == "1e+12"
    pk, chroms, v, meta = W.as_written_case()
    assert meta["heads"] >= set(range(1, 61)) and meta["tails"] >= set(range(1, 61))
    rounded = W.text_round_trip(v)
    fin = np.isfinite(rounded) & (rounded != 0)
    decade = np.full(len(v), 99)
    decade[fin] = [W.exp12(x) for x in rounded[fin]]
    assert decade[fin].min() == -11 and decade[fin].max() == 33
    b = ctx.upload(pk)
    b.set_track(L.T_OCC, v)
    store = TrackStore()
    for wz, keep in MODES:
        seg = store.adopt(b, (L.T_OCC,), write_zero=wz, keep_runs_before_nan=keep)
        assert seg is not None, (wz, keep)
        got = store.read(ctx, [seg], [0], [pk.total_bp], 0)
        text, info = b.format_track(L.T_OCC, chroms, pk.chunk_start, write_zero=wz, keep_runs_before_nan=keep, compress=False)
        assert info["hard"] == 0
        assert W.same_bits(got, W.as_read_back(text.tobytes(), pk, chroms)), (wz, keep)
        want = W.as_written_expected(pk, v, rounded, wz, keep)
        bad = np.flatnonzero((np.isnan(got) != np.isnan(want)) | (~np.isnan(want) & (got.view(np.int64) != want.view(np.int64))))
        assert len(bad) == 0, (wz, keep, [(float(v[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]])
        m = ~np.isnan(want)
        print("write_zero=%s keep=%s: %d bases with a line compared, %d without" % (wz, keep, m.sum(), (~m).sum()))
        assert m.sum() >= 150000 and (~m).sum() > 10000
        assert set(np.unique(decade[m & fin])) == set(range(-11, 34))                 # every decade has a written base
        assert np.isinf(want[m]).any() and (not wz or (np.signbit(want[m]) & (want[m] == 0)).any())      # -0.0 was written as such
    assert store.info()["segments"] == 4 and store.info()["declined"] == 0
    store.close()
    b.free()


HARD_VALUES = (9.99999999999e-12, 1e-12, 5e-324, 1e34, 9.999999999995e33, 1.7976931348623157e308) + W.NAMED_TIES
EDGE_VALUES = (1e-11, 9.999999999995e-12, 9.99999999999e33, 999999999999.5, 1234567890124.0, 875485468971499.9)


@pytest.fixture(scope="module")
def small(ctx):
    from nucleoatac_amd.device import TrackStore
    rng = np.random.default_rng(8)
    lens = [121, 700, 333, 257]
    pk = W.packed(np.cumsum([100] + [l + 50 for l in lens[:-1]]), lens)
    base = W.in_range_values(4)[:pk.total_bp].copy()
    base[rng.integers(0, pk.total_bp, 40)] = 0.0
    base[130:137] = np.nan
    b = ctx.upload(pk)
    store = TrackStore()
    yield pk, base, b, store
    store.close()
    b.free()


@pytest.mark.parametrize("value", HARD_VALUES + EDGE_VALUES, ids=lambda x: "%r" % x)
def test_adopt_refuses_exactly_the_values_it_cannot_round(ctx, small, value):
    """one value in an otherwise adoptable batch.  The verdict comes from CPython and the two named ties, never from the library: '%.11e' gives
    the exponent of the TWELVE-digit decimal ('%.12e' would print thirteen digits: 9.999999999995e-12, written as 1e-11, would count as
    too small and 9.999999999995e33, written as 1e+34, as small enough).  Refused:
    nothing is kept, the store stays open and counts no decline.  The same value where no line is written -- in a run lost before a NaN --
    refuses nothing; zero runs without write_zero (no value but zero can sit there) read back as NaN."""
    pk, base, b, store = small
    hard = W.is_hard(value)
    assert hard == (value in HARD_VALUES)
    v = base.copy()
    v[500] = value
    b.set_track(L.T_OCC_LOWER, v)
    before = store.info()
    for wz, keep in MODES:
        seg = store.adopt(b, (L.T_OCC_LOWER,), write_zero=wz, keep_runs_before_nan=keep)
        if hard:
            assert seg is None and store.info() == before, (wz, keep)
        else:
            assert seg is not None
            got = store.read(ctx, [seg], [0], [pk.total_bp], 0)
            assert W.same_bits(got, W.as_written_expected(pk, v, W.text_round_trip(v), wz, keep))
            assert got[500] == float("%.12g" % value)
    # the store is not closed and has counted nothing: an adoptable track is taken
    b.set_track(L.T_OCC_LOWER, base)
    n = store.info()["segments"]
    assert store.adopt(b, (L.T_OCC_LOWER,)) == n and store.info()["declined"] == 0
    # the value only inside a run that is lost before a NaN: no line, no verdict
    v = base.copy()
    v[500:503] = value
    v[503:506] = np.nan
    b.set_track(L.T_OCC_LOWER, v)
    rounded = W.text_round_trip(np.where(v == value, 1.0, v))
    for wz in (True, False):
        seg = store.adopt(b, (L.T_OCC_LOWER,), write_zero=wz, keep_runs_before_nan=False)
        assert seg is not None, wz
        got = store.read(ctx, [seg], [0], [pk.total_bp], 0)
        assert np.isnan(got[500:506]).all() and (wz or np.isnan(got[v == 0]).all())
        assert W.same_bits(got, W.as_written_expected(pk, v, rounded, wz, False))
    seg = store.adopt(b, (L.T_OCC_LOWER,), write_zero=True, keep_runs_before_nan=True)       # and with the run written, the verdict is back
    assert (seg is None) == hard
    assert store.info()["declined"] == 0


# ---- B -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["table", "indexable"])
def test_stored_members_on_the_device(ctx, tmp_path, layout):
    """a text of 73 members whose unsampled members are full of characters the Huffman sample never saw
    (writer_cases.stored_member_case; tests/test_deflate_host.py shows without a device that 63 of them must be stored): the
    kernel's stored arm -- LEN / NLEN, the payload copy, the plain-store trailer, sizes[] -- gives the host restatement's bytes,
    nothing is written past the result, and (layout "indexable": every chromosome in one stretch) the file is a valid tabix-indexed
    bedGraph whose index from the device's records equals the one built from the file."""
    import struct
    from nucleoatac_amd.device import pinned_empty
    from nucleoatac_amd.pyatac.tracks import Track
    indexable = layout == "indexable"
    pk, chroms, v = W.stored_member_case(indexable=indexable)
    b = ctx.upload(pk)
    b.set_track(L.T_SMOOTH, v)
    text, ti = b.format_track(L.T_SMOOTH, chroms, pk.chunk_start, compress=False)
    text = text.tobytes()
    assert ti["hard"] == 0 and text == _native_text(tmp_path, chroms, pk, v)
    host = bgzf_lines_host(text)
    slot = pinned_empty(len(host) + 65536, np.uint8)
    slot[:] = 0xee
    z, zi = b.format_track(L.T_SMOOTH, chroms, pk.chunk_start, compress=True, out=lambda n: slot[:n])
    assert (slot[len(z):] == 0xee).all()                  # nothing written past the result
    z = z.tobytes()
    assert zi["bytes"] == len(z) and zi["text_bytes"] == len(text) and zi["lines"] == ti["lines"]
    assert z == host
    assert _inflate(z) == text
    ms = W.members(z)
    assert len(ms) == (len(text) + BLK - 1) // BLK >= 72
    stored = [i for i, m in enumerate(ms) if m[2] == 1]
    dynamic = [i for i, m in enumerate(ms) if m[2] & 7 == 5]
    assert len(stored) + len(dynamic) == len(ms)
    assert (stored == list(W.INDEXABLE_ODD)) if indexable else (len(stored) >= 40 and len(dynamic) >= 8)
    for i in stored:
        o, size, _, crc, isz = ms[i]
        part = text[i * BLK:(i + 1) * BLK]
        ln, nln = struct.unpack_from("<HH", z, o + 19)
        assert isz == len(part) == ln and nln == ln ^ 0xffff and size == 18 + 5 + isz + 8
        assert z[o + 23:o + 23 + isz] == part and crc == zlib.crc32(part)
    assert np.array_equal(zi["index"]["member_pos"], [m[0] for m in ms] + [len(z)])
    if indexable:
        path = str(tmp_path / "stored.bedgraph.gz")
        with open(path, "wb") as fh:
            fh.write(z + BGZF_EOF)
        tb = TbiBuilder()
        tb.push(zi["index"], 0)
        assert tb.write(path + ".dev.tbi") == tabix_index(path) == ti["lines"]
        assert open(path + ".dev.tbi", "rb").read() == open(path + ".tbi", "rb").read()
        for i, kind in ((stored[1], "stored"), (8, "dynamic")):      # one region inside a member of either kind, through the index
            assert (i in stored) == (kind == "stored")
            part = text[i * BLK:(i + 1) * BLK]
            first = part.index(b"\n") + 1
            name, s0, e0, _ = part[first:part.index(b"\n", first)].split(b"\t")
            name, s0, e0 = name.decode(), int(s0), int(e0)
            k = [j for j in range(pk.n_chunks) if chroms[j] == name and pk.chunk_start[j] <= s0 < pk.chunk_start[j] + pk.chunk_len[j]]
            assert len(k) == 1
            k = k[0]
            e0 = min(s0 + 5, int(pk.chunk_start[k] + pk.chunk_len[k])) if kind == "dynamic" else e0
            tr = Track(name, s0, e0)
            tr.read_track(path)
            o = int(pk.out_off[k] + s0 - pk.chunk_start[k])
            assert np.array_equal(tr.vals, np.array([float(f2s(float(x))) for x in v[o:o + e0 - s0]])), kind
    b.free()


# ---- C -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_line", [False, True], ids=["line_of_33", "line_of_96"])
def test_member_border_at_every_column_of_a_line(ctx, tmp_path, long_line):
    """one batch, a text a little over one member; only the names of the one-line chunks in front grow, one character per step, so
    the first member border moves through the line it cuts one column per step: offset 0 (a line starts exactly at the border;
    otherwise the piece that starts the member has no previous line, and the first columns behind the border take eq_mask's slow path)
    up to the last column -- for a 96-character line on both sides of the 64 columns matches are searched in"""
    pk, v, chroms_of, line_len, n_steps = W.border_sweep_case(long_line)
    b = ctx.upload(pk)
    b.set_track(L.T_SMOOTH, v)
    seen = set()
    for step in range(n_steps):
        chroms = chroms_of(step)
        text, z = _check_writer(b, tmp_path, pk, chroms, v)
        assert BLK < len(text) < 2 * BLK and len(W.members(z)) == 2
        off, ln = W.first_border_offset(text)
        assert ln == line_len
        seen.add(off)
    assert seen == set(range(line_len))
    assert not long_line or (line_len > 64 and {1, 63, 64, 65, line_len - 1} <= seen)
    b.free()


@pytest.mark.parametrize("n_text", [BLK - 1, BLK, BLK + 1, 2 * BLK])
def test_text_lengths_around_the_member_size(ctx, tmp_path, n_text):
    pk, chroms, v = W.text_length_case(n_text)
    b = ctx.upload(pk)
    b.set_track(L.T_SMOOTH, v)
    text, z = _check_writer(b, tmp_path, pk, chroms, v)
    assert len(text) == n_text
    ms = W.members(z)
    assert len(ms) == (n_text + BLK - 1) // BLK
    assert all(m[4] > 0 for m in ms) and sum(m[4] for m in ms) == n_text
    b.free()


def test_degenerate_texts(ctx, tmp_path):
    """a one-line text; the shortest line there is; negative chunk starts (the writer sizes its line buffer for the '-')"""
    cases = [("one line", W.packed([123456], [300]), ["chr7"], np.full(300, 0.25), b"chr7\t123456\t123756\t0.25\n"),
             ("shortest", W.packed([0], [121]), ["c"], np.zeros(121), b"c\t0\t121\t0.0\n")]
    rng = np.random.default_rng(3)
    starts, lens = [-3000000000, -1000, -60, 70], [200, 121, 121, 500]
    neg = np.concatenate([W.plain_values(rng, 150), np.full(50, 2.0), W.plain_values(rng, 121), np.full(61, -1.5), np.full(60, 3.0),
                          W.plain_values(rng, 500)])
    cases.append(("negative starts", W.packed(starts, lens), ["n", "n", "n", "p"], neg, None))
    for name, pk, chroms, v, want in cases:
        b = ctx.upload(pk)
        b.set_track(L.T_SMOOTH, v)
        text, z = _check_writer(b, tmp_path, pk, chroms, v)
        assert want is None or text == want, name
        assert len(W.members(z)) == 1
        b.free()
    assert b"n\t-3000000000\t-2999999999\t" in text and b"n\t-60\t1\t-1.5\n" in text and b"n\t1\t61\t3.0\n" in text
