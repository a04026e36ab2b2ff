"""The high-precision reference (tests/hp_ref.py) checked on the CPU, before any device is held to it.

Measured on sweep() (811 probabilities) with SciPy 1.15.3 / mpmath 1.3.0:
    SciPy's worst relative error against ndtri_hp   s   = 4.498e-16  (hp_ref.S_SCIPY = 4.5e-16)
    tau = 2 * (1.1e-15 + s)                         tau = 3.1e-15     (hp_ref.TAU)
"""
import mpmath as mp
import numpy as np
import pytest
from scipy.special import ndtri

import hp_ref as H


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps <= 2.0**-60


def test_ndtri_hp_roundtrip_and_scipy_error():
    """ncdf(ndtri_hp(p)) = p to 1e-30 relative over the whole sweep (for p > 1/2: of 1 - p, the side that carries
    the information), and SciPy's ndtri -- the host function, and the yardstick of the accuracy figures in
    csrc/problem.h -- within 1e-15 relative of it; hp_ref.S_SCIPY records that figure for tau."""
    p = H.sweep()
    assert len(p) == 811
    worst = mp.mpf(0)
    zs = []
    with mp.workdps(H.DPS):
        for x in p:
            z = H.ndtri_mp(x)
            zs.append(z)
            pm = mp.mpf(float(x))
            if pm > 0.5:
                err = abs(mp.ncdf(-z) - (1 - pm)) / (1 - pm)
            else:
                err = abs(mp.ncdf(z) - pm) / pm
            worst = max(worst, err)
        assert worst < mp.mpf(10)**-30, worst
        zsp = ndtri(p)
        s = max(abs(mp.mpf(float(a)) - z) / abs(z) for a, z in zip(zsp, zs) if z != 0)
        s = float(s)
    print(f"scipy ndtri against ndtri_hp on the sweep: s = {s:.3e}; tau = {2 * (1.1e-15 + s):.3e}")
    assert s <= 1e-15, s
    # the recorded figure is the one tau is built from
    assert s <= H.S_SCIPY * (1 + 1e-9), (s, H.S_SCIPY)
    # the longdouble the tests use is the same number
    zl = H.ndtri_hp(p)
    with mp.workdps(H.DPS):
        for a, z in zip(zl, zs):
            assert abs(mp.mpf(np.format_float_scientific(a, precision=25, unique=False)) - z) <= abs(z) * mp.mpf(2)**-62


def _u_for(prob, k, seed):
    if prob.prior_id == H.PR.PRIOR_NORMAL:
        return H.sweep_matrix(k, prob.ndim, seed)
    return np.random.default_rng(seed).random((k, prob.ndim))


@pytest.mark.parametrize("ndim", [1, 7, 25, 40])
@pytest.mark.parametrize("like,prior", H.PAIRS)
def test_host_twin_meets_every_bound(like, prior, ndim):
    """problems.Problem -- a correct fp64 evaluation in NumPy's operation order -- against the reference, all nine
    pairs: a bound it fails would be a wrong bound.  Nothing is excluded.  GAUSS_PREC takes an asymmetric P: the host
    twin forms the full v^T P v, as the reference does."""
    prob = H.make_problem(like, prior, ndim, seed=100 + ndim, asym=0.1)
    k = 811 if prior == "normal" else 300
    u = _u_for(prob, k, 7 * ndim + 1)
    v = prob.prior_transform_many(u)
    logl = prob.loglikelihood_many(v)
    H.check(prob, u, v, logl, what=f"host {prob.name}")
    # the scalar forms are the ones the oracle calls
    l1 = np.array([prob.loglikelihood(prob.prior_transform(x)) for x in u[:40]])
    H.check(prob, u[:40], v[:40], l1, what=f"host scalar {prob.name}")


def test_asymmetric_part_does_not_change_the_reference():
    """v^T A v = 0 for an antisymmetric A: the reference with P and with (P + P^T) / 2 agree to the last bits of
    the extended type, so symmetrising on upload changes no likelihood."""
    prob = H.make_problem("prec", "affine", 7, seed=3, asym=0.1)
    P = prob.like_par[1:].reshape(7, 7)
    assert np.abs(P - P.T).max() > 0.05
    sym = H.PR.Problem(7, prob.like_id, np.concatenate([[prob.like_par[0]], (0.5 * (P + P.T)).ravel()]),
                       prob.prior_id, prob.prior_par)
    v = prob.prior_transform_many(np.random.default_rng(0).random((50, 7)))
    a, b = H.loglike_hp(prob, v), H.loglike_hp(sym, v)
    assert np.max(np.abs(a - b)) <= 64 * np.finfo(np.longdouble).eps * np.max(np.abs(a))
    # a symmetric matrix is stored as given: (a + a) / 2 == a
    S = 0.5 * (P + P.T)
    np.testing.assert_array_equal(0.5 * (S + S.T), S)


def test_gradient_matches_finite_differences():
    rng = np.random.default_rng(2)
    for like in H.LIKES:
        prob = H.make_problem(like, "identity", 4, seed=9, asym=0.1)
        v = rng.uniform(0.1, 0.9, (5, 4))
        g = H.loglike_grad_abs(prob, v)
        for i in range(4):
            h = np.zeros(4); h[i] = 1e-6
            fd = (H.loglike_hp(prob, v + h) - H.loglike_hp(prob, v - h)) / np.longdouble(2e-6)
            np.testing.assert_allclose(g[:, i], np.abs(fd.astype(float)), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("prior", ["identity", "normal"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_checks_refuse_nan_and_inf(prior, bad):
    """An evaluator that takes a wrong branch returns NaN or inf sooner than a slightly wrong number: one such value
    in v or in logl fails check() and check_from_u(), and the worst ratio reported for it is inf."""
    prob = H.make_problem("iid", prior, 3)
    u = np.random.default_rng(1).uniform(0.05, 0.95, (6, 3))
    v = prob.prior_transform_many(u)
    logl = prob.loglikelihood_many(v)
    assert max(H.check(prob, u, v, logl)) < 1.0 and H.check_from_u(prob, u, logl) < 1.0
    vb, lb = v.copy(), logl.copy()
    vb[2, 1] = bad
    lb[4] = bad
    with pytest.raises(AssertionError, match="v outside its bound"):
        H.check(prob, u, vb, logl)
    with pytest.raises(AssertionError, match="logl outside its bound"):
        H.check(prob, u, v, lb)
    with pytest.raises(AssertionError, match="logl outside its bound"):
        H.check_from_u(prob, u, lb)
    assert H.worst_ratio([0.0, abs(bad)], [1.0, 1.0]) == np.inf
    assert H.worst_ratio([0.0, 1e-300], [0.0, 0.0]) == np.inf and H.worst_ratio([0.0], [0.0]) == 0.0


def test_checks_refuse_a_value_just_outside_its_bound():
    prob = H.make_problem("iid", "affine", 3)
    u = np.random.default_rng(1).uniform(0.05, 0.95, (6, 3))
    v = prob.prior_transform_many(u)
    logl = prob.loglikelihood_many(v)
    lb = logl.copy()
    lb[0] += 3.0 * H.loglike_bound(prob, v)[0]
    with pytest.raises(AssertionError, match="logl outside its bound"):
        H.check(prob, u, v, lb)
    with pytest.raises(AssertionError, match="logl outside its bound"):
        H.check_from_u(prob, u, lb)
