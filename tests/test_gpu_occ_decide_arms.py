"""GPU: the arms of the occupancy decision that ordinary models never select, against a high-precision reference (tests/occ_ref.py).

natac_occ_decide<STEP, RN, ZF> exists in 20 forms (five steps, RN = 16 or 4 factors between two renormalisations, with / without sizes of
nfr probability zero), each reading a tile's fragments from LDS (up to OD_FM = 512 valid ones) or from global memory.  The host picks RN = 4
only for models whose probability ratios span more than 2^50 or whose alpha grid comes within 2^-50 of 0 / 1, which no other test's model
does.  Here synth_occ_distributions(251) is raised to a power p (element by element, then zeroed and renormalised) to stretch the range:

    p     variant     log2(rmax/rmin)  log2(pmin)   route asserted through Context.occ_route()
    1     none / nfr  25.8 / 24.1      -26.4        fast, RN 16, flags 0 / 2
    2.2   none / nfr  56.8 / 53.1      -50.9        fast, RN 4,  flags 0 / 2
    4     none        103.3            -88.0        fast, RN 4
    7     none        180.8            -150.2       fast, RN 4 (close to the 2^200 limit of the fast path)
    7     nfr / both  169.0 / 165.7    -150.2       fast, RN 4,  flags 2 / 3
    7     mirrored    180.8            -150.2       fast, RN 4   (the two distributions exchanged; with nfr[215:] = 0: flags 2)
    8     none        206.7            -171.0       natac_occ_mle for every tile
    10    none        258.3            -212.6       natac_occ_mle, rescale after every factor (a probability < 2^-200)

The mirrored models are what makes the RN = 4 cases sensitive to the renormalisation period.  In the p = 7 model the ratios nuc / nfr span
2^-145 .. 2^35: sixteen factors of at most 2^36 stay inside fp64, and a build that renormalised every 16 factors regardless passed every case
above (measured on the MI355X).  Mirrored, the ratios reach 2^145 at the sizes short fragments have, sixteen factors overflow, and that build
fails the mirrored cases at every step and in both ZF modes (65 .. 428 decided points wrong per case).

Two alpha grids select RN = 4 under the p = 1 models: one whose last value is 1 - 2^-52 (no exact 1 beside it), one with
alphas[1] = 2^-60 under the nfr-zero model.  Every case asserts its route first: a later change of the host's thresholds that moves a case
off its arm fails here instead of passing on another arm.

Batches: per (step, flank) three chunks of 64 step + 2 step + 1 bases (two tiles, a few live lanes in the second) -- an ordinary one, a dense
one whose first tile holds more than 512 valid fragments (global-memory arm; asserted from the input with occ_ref.tile_fragments) and a sparse
one with fragment-free windows (NaN) --; at step 5 the whole table on six chunks of 643 bases; and a hand-built batch whose first tiles hold
exactly 512 and exactly 513 valid fragments among more than 100 of invalid size (the staged arm compacts those away, the global arm multiplies
them in as the factor 1).

Per case, at EVERY grid point of EVERY chunk, the NaN pattern of G_OCC / G_LOWER / G_UPPER equals the reference's and the values are
bit-equal to alphas[index] of the high-precision reference wherever the point is decided (occ_ref: margin > 1e-10 (1 + |llmax|)); at most
1 % of a case's non-NaN points may be undecided.  The fp64 oracle must agree with the high-precision reference at the decided points (a guard
of the reference itself), the fast path with NATAC_OCC_GENERAL=1 bit for bit in grids and smoothed tracks, and the dense RN = 4 cases with
NATAC_OCC_ORDER=0.

Undecided points and differences between the fp64 oracle and long double, from a CPU check of every input below (x86-64, 80-bit long double)
-- the 1 % cap was never close to binding:

    input                                   models / alpha grids                        grid points  non-NaN  undecided  fp64 != long double
    step 5, six chunks of 643               the 14 rows of TABLE                        774          644      0          0
    step 1 / flank 20, three chunks of 67   p 2.2, 2.2 nfr, 7 nfr, 7 mirrored (+ nfr)   201          154      0          0
    step 3 / flank 61, three chunks of 199  the same five                               198          186      0          0
    step 5 / flank 60, three chunks of 331  the same five                               198          186      0          0
    step 7 / flank 62, three chunks of 463  the same five                               198          192      0          0
    step 9 / flank 44, three chunks of 595  the same five                               198          165      0          0
    512 / 513 edge, two chunks of 643       p 1, p 7 nfr                                258          258      0          0
    tiny alphas, ordinary chunk of 331      p 1 nfr                                     66           66       0          0
"""
import os

import numpy as np
import pytest

import occ_ref
from nucleoatac_amd import _lib as L
from nucleoatac_amd.packing import PackedChunks, sort_by_centre
from nucleoatac_amd.synth import make_synthetic_chunks, synth_occ_distributions, synth_sizes

pytestmark = pytest.mark.gpu

UPPER = 251
GEOMETRIES = [(1, 20), (3, 61), (5, 60), (7, 62), (9, 44)]


def cutoff():
    from oracle import natac_oracle as O
    return O.CHI2_90_DF1


def model(p, zeros):
    """synth_occ_distributions(251) ** p, zeroed like test_fast_occupancy_path_for_any_odd_step_and_flank, renormalised"""
    nucp, nfrp = synth_occ_distributions(UPPER)
    nucp, nfrp = nucp ** p, nfrp ** p
    if zeros in ("nfr", "both"):
        nfrp[170:] = 0.0
    if zeros in ("nuc", "both"):
        nucp[:90] = 0.0
    if zeros in ("mirrored", "mirrored nfr"):        # the two distributions exchanged: the large ratios sit at the sizes short fragments have
        nucp, nfrp = nfrp, nucp
    if zeros == "mirrored nfr":
        nfrp[215:] = 0.0
    return nucp / nucp.sum(), nfrp / nfrp.sum()


def alpha_grid(name):
    a = np.linspace(0, 1, 101)
    if name == "last 1-2^-52":
        a[-1] = 1 - 2.0 ** -52
    elif name == "second 2^-60":
        a[1] = 2.0 ** -60
    elif name == "tiny":
        a = np.array([0.0, 2.0 ** -300, 2.0 ** -299, 2.0 ** -298])
    else:
        assert name == "linspace"
    return a


_batches = {}


def step_batch(step, flank):
    """ordinary / dense / sparse chunk of 64 step + 2 step + 1 bases"""
    key = ("step", step, flank)
    if key not in _batches:
        Lc = 64 * step + 2 * step + 1
        counts = np.array([max(40, Lc // 3), 700 + 2 * Lc, 8], dtype=np.int64)
        # fragments out to the model's flank on both sides: the ones further out belong to no window
        _batches[key] = make_synthetic_chunks(3, Lc, 0, seed=700000 + 1000 * step + flank, flank=flank, counts=counts)
    return _batches[key]


def full_batch():
    if "full" not in _batches:
        _batches["full"] = make_synthetic_chunks(6, 643, 0, seed=643, counts=np.array([200, 1500, 30, 200, 1500, 0], dtype=np.int64))
    return _batches["full"]


def edge_batch():
    """step 5 / flank 60, two chunks of 643 bases: tile 0 covers the centres [-58, 377], tile 1 [262, 697].  Chunk 0 has exactly 512 valid
    fragments in tile 0, chunk 1 exactly 513; each also 120 of invalid size (251 .. 699) among them and a thin second tile."""
    if "edge" in _batches:
        return _batches["edge"]
    rng = np.random.default_rng(512513)
    Lc = 643
    ls, ns, offs, bias = [], [], [0], []
    for target in (512, 513):
        sizes = synth_sizes(rng, 4000).astype(np.int64)
        valid = sizes[sizes < UPPER]
        shared, right = 60, 40
        c = np.concatenate([rng.integers(-58, 262, size=target - shared), rng.integers(262, 378, size=shared),
                            rng.integers(378, 698, size=right), rng.integers(-58, 378, size=120), rng.integers(378, 698, size=20)])
        n = np.concatenate([valid[:target + right], rng.integers(UPPER, 700, size=140)])
        l = c - (n - 1) // 2
        o = sort_by_centre(l, n)
        ls.append(l[o])
        ns.append(n[o])
        offs.append(offs[-1] + len(l))
        bias.append(rng.normal(0.0, 0.8, size=Lc + 246 + 247))
    _batches["edge"] = PackedChunks(chunk_start=np.array([10000, 20000]), chunk_len=np.array([Lc, Lc]), frag_off=np.array(offs),
                                    frag_lpos=np.concatenate(ls), frag_ilen=np.concatenate(ns),
                                    bias_off=np.arange(3) * (Lc + 246 + 247), bias_log=np.concatenate(bias))
    return _batches["edge"]


_refs = {}


def reference(bkey, pk, mkey, akey, step, flank):
    """per chunk: occ_ref.chunk_reference + the fp64 oracle's indices at every live grid point (computed once per input, read-only)"""
    key = (bkey, mkey, akey)
    if key in _refs:
        return _refs[key]
    from oracle import natac_oracle as O
    nucp, nfrp = model(*mkey)
    alphas = alpha_grid(akey)
    out = []
    for k in range(pk.n_chunks):
        l, n = pk.chunk_frags(k)
        Lk = int(pk.chunk_len[k])
        oc = O.occ_chunk_tracks(l.astype(np.int64), n.astype(np.int64), 0, Lk, pk.chunk_bias(k), -pk.bias_left, model(1, "none")[0],
                                model(1, "none")[1], upper=UPPER, flank=flank, step=step, cutoff=cutoff(), n_alpha=3)
        r = occ_ref.chunk_reference(oc["mat"], oc["b0"], nucp, nfrp, alphas, cutoff(), Lk, step, flank)
        W = 2 * flank + 1
        fp64 = np.full_like(r["idx"], -1)
        for j, i in enumerate(range((step - 1) // 2, Lk, step)):
            if r["live"][j]:
                vals = O.calculate_occupancy(oc["mat"][:, i:i + W].sum(axis=1), oc["b0"][:, i:i + W].sum(axis=1), nucp, nfrp, alphas, cutoff())
                fp64[j] = [int(np.flatnonzero(alphas == v)[0]) for v in vals]
        r["fp64"] = fp64
        for v in r.values():
            v.setflags(write=False)
        out.append(r)
    _refs[key] = out
    return out


def run_device(pk, mkey, akey, step, flank, env=None):
    from nucleoatac_amd.device import Context
    nucp, nfrp = model(*mkey)
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        with Context(0) as c:
            c.set_occ_model(nucp, nfrp, alphas=alpha_grid(akey), cutoff=cutoff(), step=step, flank=flank)
            route = c.occ_route()
            b = c.upload(pk)
            b.run_occ()
            out = dict(route=route, status=b.status(), grids=[b.grid(g) for g in (L.G_OCC, L.G_LOWER, L.G_UPPER)],
                       tracks=[b.track(t) for t in (L.T_OCC, L.T_OCC_LOWER, L.T_OCC_UPPER, L.T_OCC_COV)])
            b.free()
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)
    return out


def check_against_reference(what, dev, ref, akey):
    """assertions 1-3 of the module docstring; returns (non-NaN points, undecided points)"""
    alphas = alpha_grid(akey)
    idx = np.concatenate([r["idx"] for r in ref])
    decided = np.concatenate([r["decided"] for r in ref])
    fp64 = np.concatenate([r["fp64"] for r in ref])
    live = idx[:, 0] >= 0
    n_live, n_undecided = int(live.sum()), int((live & ~decided).sum())
    print("occ-arms %s: grid points %d, non-NaN %d, undecided %d, fp64 oracle != high precision at %d, route %s" % (
        what, len(idx), n_live, n_undecided, int((fp64 != idx).any(axis=1).sum()), dev["route"]))
    assert np.array_equal(fp64[decided], idx[decided]), "%s: the fp64 oracle leaves the high-precision reference at a decided point" % what
    assert n_undecided <= 0.01 * n_live, "%s: %d of %d points undecided" % (what, n_undecided, n_live)
    for gi, name in enumerate(("G_OCC", "G_LOWER", "G_UPPER")):
        g = dev["grids"][gi]
        assert g.shape == (len(idx),), "%s %s: %s grid points, reference %d" % (what, name, g.shape, len(idx))
        assert np.array_equal(np.isnan(g), ~live), "%s %s: NaN pattern differs from the reference" % (what, name)
        want = alphas[idx[decided, gi]]
        bad = np.flatnonzero(g[decided] != want)
        assert bad.size == 0, "%s %s: %d decided points differ, first at %d: %r, reference %r (margin %g)" % (
            what, name, bad.size, np.flatnonzero(decided)[bad[0]], g[decided][bad[0]], want[bad[0]],
            np.concatenate([r["margin"] for r in ref])[decided][bad[0]])
    return n_live, n_undecided


def check_same(what, a, b):
    for x, y in zip(a["grids"] + a["tracks"], b["grids"] + b["tracks"]):
        assert np.array_equal(x, y, equal_nan=True), what
    assert not a["status"].any() and not b["status"].any(), what


def check_case(what, bkey, pk, mkey, akey, step, flank, route, dense):
    ref = reference(bkey, pk, mkey, akey, step, flank)
    fast = run_device(pk, mkey, akey, step, flank)
    assert fast["route"] == route, "%s: route %s, this case is written for %s" % (what, fast["route"], route)
    check_against_reference(what, fast, ref, akey)
    assert not fast["status"].any()
    if not route[0]:
        return
    general = run_device(pk, mkey, akey, step, flank, env={"NATAC_OCC_GENERAL": "1"})
    assert general["route"] == (False, 0, route[2])
    check_same("%s: block-sum kernels vs NATAC_OCC_GENERAL=1" % what, fast, general)
    if dense and route[1] == 4:
        in_order = run_device(pk, mkey, akey, step, flank, env={"NATAC_OCC_ORDER": "0"})
        assert in_order["route"] == route
        check_same("%s: heavy tiles first vs NATAC_OCC_ORDER=0" % what, fast, in_order)


def assert_dense(pk, chunk, step, flank):
    l, n = pk.chunk_frags(chunk)
    nv = occ_ref.tile_fragments(l, n, 0, step, flank, UPPER)[2]
    assert nv > 512, "chunk %d: %d valid fragments in its first tile, the global-memory arm needs more than 512" % (chunk, nv)


TABLE = [  # p, zeros, alpha grid, (fast, rn, flags)
    (1, "none", "linspace", (True, 16, 0)), (1, "nfr", "linspace", (True, 16, 2)),
    (2.2, "none", "linspace", (True, 4, 0)), (2.2, "nfr", "linspace", (True, 4, 2)),
    (4, "none", "linspace", (True, 4, 0)), (7, "none", "linspace", (True, 4, 0)),
    (7, "nfr", "linspace", (True, 4, 2)), (7, "both", "linspace", (True, 4, 3)),
    (7, "mirrored", "linspace", (True, 4, 0)), (7, "mirrored nfr", "linspace", (True, 4, 2)),
    (1, "none", "last 1-2^-52", (True, 4, 0)), (1, "nfr", "second 2^-60", (True, 4, 2)),
    (8, "none", "linspace", (False, 0, 0)), (10, "none", "linspace", (False, 0, 0))]


@pytest.mark.parametrize("p,zeros,akey,route", TABLE)
def test_step5_model_table(p, zeros, akey, route):
    """the whole table at step 5 / flank 60 on six chunks of 643 bases (counts 200, 1500, 30, 200, 1500, 0): both dense chunks take the
    global-memory arm in both of their tiles, the 30-fragment chunk has fragment-free windows, the last chunk is empty.  p = 8 and p = 10
    leave the block-sum kernels (the reference comparison alone, run once)."""
    pk = full_batch()
    for chunk in (1, 4):
        assert_dense(pk, chunk, 5, 60)
    check_case("step 5 table p=%g zeros=%s alphas=%s" % (p, zeros, akey), "full", pk, (p, zeros), akey, 5, 60, route, dense=True)


@pytest.mark.parametrize("p,zeros,route", [(2.2, "none", (True, 4, 0)), (2.2, "nfr", (True, 4, 2)), (7, "nfr", (True, 4, 2)),
                                           (7, "mirrored", (True, 4, 0)), (7, "mirrored nfr", (True, 4, 2))])
@pytest.mark.parametrize("step,flank", GEOMETRIES)
def test_rn4_at_every_step(step, flank, p, zeros, route):
    """natac_occ_decide<STEP, 4, false> and <STEP, 4, true> for every STEP, staged (ordinary and sparse chunk) and from global memory (dense
    chunk); the sparse chunk's fragment-free windows must come back NaN"""
    pk = step_batch(step, flank)
    assert_dense(pk, 1, step, flank)
    l, n = pk.chunk_frags(0)
    assert occ_ref.tile_fragments(l, n, 0, step, flank, UPPER)[2] <= 512
    bkey = ("step", step, flank)
    check_case("step %d flank %d p=%g zeros=%s" % (step, flank, p, zeros), bkey, pk, (p, zeros), "linspace", step, flank, route, dense=True)
    assert not reference(bkey, pk, (p, zeros), "linspace", step, flank)[2]["live"].all()


@pytest.mark.parametrize("p,zeros,route", [(1, "none", (True, 16, 0)), (7, "nfr", (True, 4, 2))])
def test_staging_edge_512_and_513_valid_fragments(p, zeros, route):
    """a tile with exactly OD_FM = 512 valid fragments is staged, one with 513 reads global memory; both carry more than 100 fragments of
    invalid size between the valid ones, which the staged arm drops while compacting and the global arm multiplies in as the factor 1"""
    pk = edge_batch()
    for chunk, want in ((0, 512), (1, 513)):
        l, n = pk.chunk_frags(chunk)
        t0, t1, nv = occ_ref.tile_fragments(l, n, 0, 5, 60, UPPER)
        assert nv == want and (t1 - t0) - nv >= 100
        u0, u1, nv1 = occ_ref.tile_fragments(l, n, 1, 5, 60, UPPER)
        assert 0 < nv1 <= 512 and u0 < t1            # the second tile shares fragments with the first and stays staged
    check_case("512 / 513 edge p=%g zeros=%s" % (p, zeros), "edge", pk, (p, zeros), "linspace", 5, 60, route, dense=False)


def test_tiny_alpha_grid_with_zero_nfr_sizes():
    """a fragment of a zero-nfr size contributes the factor alpha: four factors of an alpha below 2^-256 underflow between two renormalisations
    of natac_occ_decide (the likelihood read 0 = -inf, and a grid of nothing but such alphas returned alphas[0] with a clean status).  The host
    sends a zero-nfr model whose smallest positive alpha is below 2^-250 to natac_occ_mle, which renormalises after every such factor, and
    refuses alphas below 2^-500 with an argument error that names the bound."""
    from nucleoatac_amd.device import Context
    # the ordinary chunk: each of its windows holds a fragment of a zero-nfr size, so log L rises by a multiple of log 2 from one alpha to the
    # next and the largest alpha wins.  (A window without one has log L = const + O(2^-298): undecided in any arithmetic.)
    pk = step_batch(5, 60).subset(0, 1)
    bkey = ("step", 5, 60, "ordinary chunk")
    check_case("tiny alphas, nfr-zero p=1", bkey, pk, (1, "nfr"), "tiny", 5, 60, (False, 0, 0), dense=False)
    ref = reference(bkey, pk, (1, "nfr"), "tiny", 5, 60)
    assert ref[0]["decided"].all() and (ref[0]["idx"][:, 0] == 3).all()
    nucp, nfrp = model(1, "nfr")
    with Context(0) as c:
        with pytest.raises(L.NatacError, match=r"2\^-500"):
            c.set_occ_model(nucp, nfrp, alphas=np.array([0.0, 2.0 ** -600, 0.5, 1.0]), cutoff=cutoff(), step=5, flank=60)
        # without a zero nfr probability the factor is 1 + alpha t: any alpha is fine, on the block-sum kernels
        c.set_occ_model(*model(1, "none"), alphas=np.array([0.0, 2.0 ** -600, 0.5, 1.0]), cutoff=cutoff(), step=5, flank=60)
        assert c.occ_route() == (True, 16, 0)
