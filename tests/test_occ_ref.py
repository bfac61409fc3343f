"""CPU: tests/occ_ref.py, the high-precision occupancy reference of tests/test_gpu_occ_decide_arms.py, against the fp64 oracle and itself."""
import numpy as np

import occ_ref
from nucleoatac_amd.synth import make_synthetic_chunks, synth_occ_distributions
from oracle import natac_oracle as O


def _windows():
    pk = make_synthetic_chunks(1, 331, 110, seed=9)
    l, n = pk.chunk_frags(0)
    nucp, nfrp = synth_occ_distributions(251)
    oc = O.occ_chunk_tracks(l.astype(np.int64), n.astype(np.int64), 0, 331, pk.chunk_bias(0), -pk.bias_left, nucp, nfrp, n_alpha=3)
    return pk, oc, nucp, nfrp


def test_decided_points_are_the_fp64_oracles():
    pk, oc, nucp, nfrp = _windows()
    alphas = np.linspace(0, 1, 101)
    r = occ_ref.chunk_reference(oc["mat"], oc["b0"], nucp, nfrp, alphas, O.CHI2_90_DF1, 331, 5, 60)
    assert r["idx"].shape == (66, 3) and r["live"].all() and r["decided"].sum() >= 60
    full = O.occ_chunk_tracks(*[x.astype(np.int64) for x in pk.chunk_frags(0)], 0, 331, pk.chunk_bias(0), -pk.bias_left, nucp, nfrp)
    for gi, key in enumerate(("occ", "occ_lower", "occ_upper")):
        assert np.array_equal(alphas[r["idx"][r["decided"], gi]], full[key][2::5][r["decided"]])


def test_zero_rule_and_margin():
    """0 * log 0 = NaN -> -inf: a zero nfr_prob shuts out alpha = 0 even for a window without a fragment of that size, a zero nuc_prob
    alpha = 1; a window whose log-likelihood is flat in alpha is undecided"""
    nucp, nfrp = np.array([0.0, 0.5, 0.5]), np.array([0.5, 0.5, 0.0])
    alphas = np.array([0.0, 0.25, 0.75, 1.0])
    ins, bias = np.array([0.0, 3.0, 0.0]), np.ones(3)
    imax, ilo, ihi, margin, llmax = occ_ref.grid_point(ins, bias, nucp, nfrp, alphas, 2.7)
    assert (imax, ilo, ihi) == (1, 1, 2) and margin == 0.0 and llmax == 3 * np.log(0.5)
    imax, ilo, ihi, margin, llmax = occ_ref.grid_point(np.array([0.0, 0.0, 2.0]), bias, nucp, nfrp, alphas, 2.7)
    assert (imax, ilo, ihi) == (2, 2, 2)               # log L = 2 log(alpha / 2): the ratio of 0.25 is 4 log 3 > 2.7
    assert abs(margin - (4 * np.log(3) - 2.7)) < 1e-12


def test_mpmath_backend_agrees_with_long_double():
    _, oc, nucp, nfrp = _windows()
    alphas = np.linspace(0, 1, 11)
    ins, bias = oc["mat"][:, 100:221].sum(axis=1), oc["b0"][:, 100:221].sum(axis=1)
    a = occ_ref._logliks_mpmath(ins, bias, nucp, nfrp, alphas)
    b = occ_ref._logliks_longdouble(ins, bias, nucp, nfrp, alphas)
    assert ins.sum() > 0
    for x, y in zip(a, b):
        assert abs(float(x) - float(y)) <= 1e-15 * abs(float(x))


def test_tile_fragments():
    lpos = np.array([-70, -58, 0, 300, 377, 378, 600])
    ilen = np.array([1, 1, 300, 2, 1, 1, -3])
    # tile 0 of step 5 / flank 60: centres in [-58, 377]; ilen 300 is not below upper
    assert occ_ref.tile_fragments(lpos, ilen, 0, 5, 60, 251) == (1, 5, 3)
    assert occ_ref.tile_fragments(lpos, ilen, 1, 5, 60, 251) == (3, 7, 3)
