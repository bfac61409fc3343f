"""The per-call device scope of the library (DeviceCall, csrc/natac_runtime.hpp: temporaries, copies, error latch, kernel timing, one finishing step)
through the entry points built on it, at the smallest shapes where the scope rather than a kernel can go wrong: empty and one-element
inputs (the one-element allocation of an empty upload, skipped launches, the early returns), a call that fails after its device work
followed at once by a call of another size on the same context (pool blocks recycled across the failure), kernel_ms with and without
the timer, the profile event of a call that launches and of one that does not, and two contexts taking turns on one device.

References: oracle/natac_oracle.py; tests/sites_ref.py for the two counting rules the oracle does not restate.  Counts are compared
exactly; float64 results in the TIGHT tier of tests/helpers.py (1e-10 relative + 1e-12): a handful of float64 operations per value,
exp() and log() within a few ulp of numpy's.  No test provokes a HIP error: the latch's failure branch is covered by reading."""
import ctypes as C
import math

import numpy as np
import pytest

import sites_ref as R
from helpers import TIGHT_ATOL, TIGHT_RTOL

pytestmark = pytest.mark.gpu

NUC = ["A", "C", "G", "T"]
EMPTY = np.zeros(0, np.int64)
ONE_L, ONE_N = np.array([10], np.int64), np.array([1], np.int64)      # one fragment: l = 10, n = 1


def close(got, ref):
    np.testing.assert_allclose(got, ref, rtol=TIGHT_RTOL, atol=TIGHT_ATOL)


def seq_bytes(text):
    return np.frombuffer(text.encode("ascii"), np.uint8)


@pytest.fixture(scope="module")
def model():
    from nucleoatac_amd.synth import synth_occ_distributions
    return synth_occ_distributions(251)


def check_one_fragment_calls(ctx, O):
    """the three fragment drop-ins over the one-base region [10, 11) with one fragment, against the oracle and its known values"""
    mat = ctx.make_fragment_mat(ONE_L, ONE_N, 10, 11, 0, 2)
    assert np.array_equal(mat, O.make_fragment_mat(ONE_L, ONE_N, 10, 11, 0, 2)) and mat.tolist() == [[0.0], [1.0]]
    ins = ctx.get_insertions(ONE_L, ONE_N, 10, 11)
    assert np.array_equal(ins, O.get_insertions(ONE_L, ONE_N, 10, 11)) and ins.tolist() == [2.0]
    plus, minus = ctx.get_stranded_insertions(ONE_L, ONE_N, 10, 11)
    ref = O.get_stranded_insertions(ONE_L, ONE_N, 10, 11)
    assert np.array_equal(plus, ref[0]) and np.array_equal(minus, ref[1]) and (plus.tolist(), minus.tolist()) == ([1.0], [1.0])


def test_empty_and_minimal_inputs_on_one_context():
    from nucleoatac_amd.device import Context
    from oracle import natac_oracle as O
    with Context(0) as ctx:
        # no fragments over a one-base region: the launches that read fragments are skipped, the zeroed outputs come back
        assert ctx.make_fragment_mat(EMPTY, EMPTY, 10, 11, 0, 2).tolist() == [[0.0], [0.0]]
        assert ctx.get_insertions(EMPTY, EMPTY, 10, 11).tolist() == [0.0]
        plus, minus = ctx.get_stranded_insertions(EMPTY, EMPTY, 10, 11)
        assert plus.tolist() == [0.0] and minus.tolist() == [0.0]
        check_one_fragment_calls(ctx, O)
        # the size histogram: fragments but no chunk, chunks but no fragment
        assert np.array_equal(ctx.fragment_sizes(ONE_L, ONE_N, EMPTY, EMPTY, 0, 5), O.fragment_sizes_from_chunks(ONE_L, ONE_N, [], [], 0, 5))
        assert not ctx.fragment_sizes(EMPTY, EMPTY, [0], [100], 0, 5).any()
        assert np.array_equal(ctx.fragment_sizes(ONE_L, ONE_N, [0], [100], 0, 5), O.fragment_sizes_from_chunks(ONE_L, ONE_N, [0], [100], 0, 5))
        # three values under a three-tap window
        sig = np.array([1.0, 4.0, -2.5])
        for mode in ("valid", "same"):
            got = ctx.smooth(sig, 3, mode=mode)
            assert got.shape == ((1,) if mode == "valid" else (3,))
            close(got, O.smooth(sig, 3, mode=mode))
        # one (p, v) pair
        p, v = np.array([0.25]), np.array([3.0])
        close(ctx.calculate_cov(p, v, 4), O.calculate_cov_closed(p, v, 4))
        close(ctx.calculate_cov(p, v, 4, literal=True), O.calculate_cov_literal(p, v, 4))
        # a matrix as wide as the template: one output
        sub, vm = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, 4.0]]), np.array([[2.0, 0.0, 1.0], [1.0, 1.0, -3.0]])
        got = ctx.correlate_valid(sub, vm)
        assert got.shape == (1,)
        close(got, O.correlate_valid(sub, vm))
        # a bias matrix of one column
        bias_log = np.linspace(-0.6, 0.9, 7)
        got = ctx.make_bias_mat(bias_log, 0, 3, 4, 1, 4)
        assert got.shape == (3, 1)
        close(got, O.make_bias_mat(bias_log, 0, 3, 4, 1, 4))
        # a one-column PWM on one base
        pwm = np.array([[0.4], [0.1], [0.2], [0.3]])
        got = ctx.pwm_bias("A", pwm, NUC)
        assert got.shape == (1,)
        close(got, O.compute_bias_pwm("A", pwm, NUC))
        # base content: no range (the early return), one range of one base
        assert ctx.base_counts(seq_bytes("ACGT"), [], []).tolist() == [0, 0, 0, 0]
        assert ctx.base_counts(seq_bytes("ACGT"), [2], [3]).tolist() == [0, 0, 1, 0]
        # one record, one region; one site
        pos, tlen = np.array([100], np.int64), np.array([58], np.int64)
        got = ctx.region_counts(pos, tlen, [100], [110])
        assert got.tolist() == R.region_counts_brute(pos, tlen, [100], [110], 0, 500, 1).tolist() == [1]
        seq = seq_bytes("ACGTA")
        got, n_used = ctx.site_seq_counts(seq, [2], None, 1, 1)
        want, want_n = R.site_counts_ref(seq, [2], None, 1, 1, 1)
        assert np.array_equal(got, want) and n_used == want_n == 1
        # one formatted value
        assert ctx.format_doubles([0.1]) == (["%.12g" % 0.1], 0)
        # and the first calls again: every temporary of the calls in between has gone back to the pool
        check_one_fragment_calls(ctx, O)


def test_a_failed_call_leaves_the_context_usable(model):
    """make_bias_mat over a track that does not cover the region and calculate_occupancy where no alpha passes both fail with
    NATAC_E_ARG AFTER their kernel ran and their result words came back; the next call, of another size, must be right"""
    from nucleoatac_amd import _lib as L
    from nucleoatac_amd.device import Context
    from oracle import natac_oracle as O
    nucp, nfrp = model
    nuc0, nfr0 = nucp.copy(), nfrp.copy()
    nuc0[7] = nfr0[7] = 0.0                   # a size bin of probability 0 in both distributions: every log-likelihood is -inf
    nuc0, nfr0 = nuc0 / nuc0.sum(), nfr0 / nfr0.sum()
    inserts = np.zeros(251)
    inserts[[40, 90, 180]] = [2.0, 1.0, 3.0]
    bias = np.ones(251)
    alphas = np.linspace(0, 1, 101)
    with pytest.raises(ValueError):
        O.calculate_occupancy(inserts, bias, nuc0, nfr0, alphas, O.CHI2_90_DF1)
    want_occ = tuple(O.calculate_occupancy(inserts, bias, nucp, nfrp, alphas, O.CHI2_90_DF1))
    rng = np.random.default_rng(11)
    with Context(0) as ctx:
        for rnd in range(4):
            short = rng.normal(0, 0.5, 3 + rnd)                     # covers [0, 3 + rnd): columns [3, 6) with sizes below 4 reach [2, 7)
            with pytest.raises(L.NatacError) as e:
                ctx.make_bias_mat(short, 0, 3, 6, 1, 4)
            assert e.value.code == -1 and "does not cover" in str(e.value)
            nf = 40 * (rnd + 1) + 3
            l = rng.integers(-20, 320, nf).astype(np.int64)
            n = rng.integers(1, 60, nf).astype(np.int64)
            end = 257 + 64 * rnd
            assert np.array_equal(ctx.get_insertions(l, n, 0, end), O.get_insertions(l, n, 0, end))
            track = rng.normal(0, 0.5, 40 + 8 * rnd)
            close(ctx.make_bias_mat(track, 0, 10, 30 + 8 * rnd, 1, 12), O.make_bias_mat(track, 0, 10, 30 + 8 * rnd, 1, 12))
            ctx.set_occ_model(nuc0, nfr0, alphas=alphas, cutoff=O.CHI2_90_DF1)
            with pytest.raises(ValueError):
                ctx.calculate_occupancy(inserts, bias)
            sig = rng.normal(0, 1, 50 * (rnd + 1) + 1)
            close(ctx.smooth(sig, 5, mode="same"), O.smooth(sig, 5, mode="same"))
            ctx.set_occ_model(nucp, nfrp, alphas=alphas, cutoff=O.CHI2_90_DF1)
            assert ctx.calculate_occupancy(inserts, bias) == want_occ


def test_kernel_ms_does_not_change_the_results():
    from nucleoatac_amd import _lib as L
    from nucleoatac_amd.device import Context
    rng = np.random.default_rng(3)

    def timed(ms):
        return isinstance(ms, float) and math.isfinite(ms) and ms >= 0

    with Context(0) as ctx:
        # window counts: one chunk of 20 bases, two fragments with all four ends inside, flank 2
        cl, fo, lpos, ilen, so = [20], [0, 2], [3, 8], [5, 9], [0, 24]
        seq = rng.choice(seq_bytes("ACGT"), 24)
        M0, n0 = ctx.insertion_seq_counts(cl, fo, lpos, ilen, so, seq, 2)
        M1, n1, ms = ctx.insertion_seq_counts(cl, fo, lpos, ilen, so, seq, 2, with_kernel_ms=True)
        assert n0 == n1 == 4 and np.array_equal(M0, M1) and M0.sum(axis=0).tolist() == [4] * 5 and timed(ms)
        assert ctx.insertion_seq_counts([], [0], [], [], [0], [], 2, with_kernel_ms=True)[2] == 0.0          # no chunk
        assert ctx.insertion_seq_counts(cl, [0, 0], [], [], so, seq, 2, with_kernel_ms=True)[1:] == (0, 0.0)  # no fragment
        # region counts
        pos = np.sort(rng.integers(0, 3000, 200)).astype(np.int64)
        tlen = rng.integers(20, 400, 200).astype(np.int64)
        s = np.sort(rng.integers(0, 3000, 70)).astype(np.int64)
        e = s + rng.integers(0, 300, 70)
        want = R.region_counts_brute(pos, tlen, s, e, 0, 500, 1)
        c0 = ctx.region_counts(pos, tlen, s, e)
        c1, ms = ctx.region_counts(pos, tlen, s, e, with_kernel_ms=True)
        assert np.array_equal(c0, want) and np.array_equal(c1, want) and timed(ms)
        c2 = np.full(70, -1, np.int64)          # the C call without a timing pointer
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        L.check(L.load().natac_region_counts(ctx._h, 200, vp(pos), vp(tlen), 70, vp(s), vp(e), 0, 500, 1, vp(c2), None))
        assert np.array_equal(c2, want)
        c3, ms = ctx.region_counts(pos[:0], tlen[:0], s, e, with_kernel_ms=True)
        assert not c3.any() and ms == 0.0
        # word counts around sites
        chrom = rng.choice(seq_bytes("ACGTNacgt"), 500)
        cen = rng.integers(0, 500, 40).astype(np.int64)
        minus = (rng.random(40) < 0.5).astype(np.uint8)
        want, want_n = R.site_counts_ref(chrom, cen, minus, 7, 5, 2)
        m0, k0 = ctx.site_seq_counts(chrom, cen, minus, 7, 5, 2)
        m1, k1, ms = ctx.site_seq_counts(chrom, cen, minus, 7, 5, 2, with_kernel_ms=True)
        assert np.array_equal(m0, want) and np.array_equal(m1, want) and k0 == k1 == want_n and timed(ms)
        m2, k2, ms = ctx.site_seq_counts(chrom, cen[:0], None, 7, 5, 2, with_kernel_ms=True)
        assert not m2.any() and k2 == 0 and ms == 0.0


def test_profile_counts_the_launch_and_only_the_launch():
    from nucleoatac_amd.device import Context
    from oracle import natac_oracle as O
    rng = np.random.default_rng(5)
    l = rng.integers(0, 900, 300).astype(np.int64)
    n = rng.integers(1, 250, 300).astype(np.int64)
    cs, ce = np.array([0, 400], np.int64), np.array([500, 1000], np.int64)
    with Context(0) as ctx:
        ctx.profile_enable(True)
        ctx.profile_reset()
        assert ctx.profile()["size_hist"][1] == 0
        assert np.array_equal(ctx.fragment_sizes(l, n, cs, ce, 0, 250), O.fragment_sizes_from_chunks(l, n, cs, ce, 0, 250))
        ms, launches = ctx.profile()["size_hist"]
        assert launches == 1 and math.isfinite(ms) and ms >= 0
        assert not ctx.fragment_sizes(l, n, EMPTY, EMPTY, 0, 250).any()          # no chunk: no launch
        assert not ctx.fragment_sizes(EMPTY, EMPTY, cs, ce, 0, 250).any()        # no fragment: no launch
        assert ctx.profile()["size_hist"][1] == 1
        ctx.profile_enable(False)


def test_two_contexts_alternating_on_one_device():
    """a block one context's call gives back may be the next block the other context's call takes: every result must still be
    the oracle's (a smoke check of the scope's drain-before-free rule, not a proof of it)"""
    from nucleoatac_amd.device import Context
    from oracle import natac_oracle as O
    with Context(0) as a, Context(0) as b:
        for _ in range(36):
            check_one_fragment_calls(a, O)
            check_one_fragment_calls(b, O)
