"""DH_PRIOR_TABLE / DH_LIKE_GAUSS_MIX on the host: the callables of dynesty_amd/problems.py against the high-precision
reference of tests/problem_ext_hp_ref.py within its bounds, the reference against hp_ref's where the two describe the
same problem, logz_truth against a quadrature, and the constructors' refusals."""
import math

import numpy as np
import pytest

import hp_ref as H
import problem_ext_hp_ref as X
from dynesty_amd import problems as PR

K = 130
LD = np.longdouble


@pytest.mark.parametrize("ndim", [1, 2, 5, 9, 33])
def test_table_prior_callables_hold_to_the_reference(ndim):
    prob = PR.gauss_general(np.zeros(ndim), np.eye(ndim), prior=X.mixed_rows(ndim))
    u = H.sweep_matrix(K, ndim, 500 + ndim)
    v = prob.prior_transform_many(u)
    err = np.abs(v.astype(LD) - X.prior_hp(prob, u)).astype(np.float64)
    r = H.worst_ratio(err, X.prior_bound(prob, u))
    print(f"host table prior D={ndim}: err/bound {r:.3f}")
    assert r <= 1.0
    np.testing.assert_array_equal(prob.prior_transform(u[7]), v[7])
    if ndim >= 3:  # twelve decades
        assert v[:, 2].min() < 1e-5 and v[:, 2].max() > 1e5


@pytest.mark.parametrize("case", X.MIX_CASES)
@pytest.mark.parametrize("m", [1, 2, 4, 5, 8])
def test_mixture_callables_hold_to_the_reference(case, m):
    ndim = 5
    prob = X.mixture_problem(case, ndim, m, seed=100 + m)
    u = X.near_component_u(prob, K, 700 + m)
    v = prob.prior_transform_many(u)
    many = prob.loglikelihood_many(v)
    one = np.array([prob.loglikelihood(x) for x in v])
    bound = X.loglike_bound(prob, v)
    ref = X.loglike_hp(prob, v)
    for got in (many, one):
        r = H.worst_ratio(np.abs(got.astype(LD) - ref).astype(np.float64), bound)
        print(f"host mixture {prob.name}: err/bound {r:.3f}")
        assert r <= 1.0
    assert np.all(bound < 1e-10)  # the bound is a rounding bound, not a loose one
    a = X._components_hp(prob, v).astype(np.float64)
    if case == "separated" and m > 1:  # one component is all there is: the result is a* to the bound
        assert np.all(np.abs(many - a.max(axis=1)) <= bound)
        assert np.all(np.sort(a, axis=1)[:, -2] - a.max(axis=1) < -745.0)
    if case == "identical" and m == 2:
        assert np.all(np.abs(many - (a[:, 0] + math.log(2.0))) <= bound + 4 * H.EPS * np.abs(many))


def test_one_zero_mean_component_is_gauss_prec():
    """M = 1, mu = 0: the reference value, the bound's leading term and the host value are GAUSS_PREC's."""
    n = 7
    P = H.spd_plus_antisym(n, 3)
    c = -1.25
    mix = PR.Problem(n, PR.LIKE_GAUSS_MIX, np.concatenate([[1.0, c], np.zeros(n), P.ravel()]), PR.PRIOR_IDENTITY, [])
    prec = PR.Problem(n, PR.LIKE_GAUSS_PREC, np.concatenate([[c], P.ravel()]), PR.PRIOR_IDENTITY, [])
    v = np.random.default_rng(1).standard_normal((K, n))
    np.testing.assert_array_equal(X.loglike_hp(mix, v), H.loglike_hp(prec, v))
    # (the gradient is an fp64 helper of the bounds, summed in another order here: equal to rounding)
    np.testing.assert_allclose(X.loglike_grad_abs(mix, v), H.loglike_grad_abs(prec, v), rtol=1e-12, atol=1e-13)
    assert np.all(X.loglike_bound(mix, v) >= H.loglike_bound(prec, v))
    assert np.all(np.abs(mix.loglikelihood_many(v) - prec.loglikelihood_many(v)) <= 2 * H.loglike_bound(prec, v))


def test_all_uniform_table_is_affine():
    """Rows (lo, hi) = (b - a, b + a): the same prior as AFFINE [a, b], the same reference value."""
    n, a, b = 6, 4.0, 0.5
    tab = PR.Problem(n, PR.LIKE_GAUSS_IID, [0.0], PR.PRIOR_TABLE, PR.prior_table([("uniform", b - a, b + a)] * n).ravel())
    aff = PR.Problem(n, PR.LIKE_GAUSS_IID, [0.0], PR.PRIOR_AFFINE, [a, b])
    u = np.random.default_rng(2).random((K, n))
    d = np.abs(X.prior_hp(tab, u) - H.prior_hp(aff, u)).astype(np.float64)
    assert d.max() <= 2.0**-60 * (a + abs(b))  # the same real number, to the rounding of the extended type
    assert np.all(np.abs(tab.prior_transform_many(u) - aff.prior_transform_many(u)) <= X.prior_bound(tab, u) + H.prior_bound(aff, u))


def _quad_logz(prob, means, covs):
    """ln of the integral of L(v) pi(v) dv at D = 2 by a tensor Gauss-Legendre rule (400 nodes a side over the box /
    over mu0 +- 12 sigma of a normal row: the integrand is a sum of Gaussians, the rule converges geometrically)."""
    tab = prob.prior_par.reshape(2, 3)
    xs, ws, dens = [], [], []
    g, gw = np.polynomial.legendre.leggauss(400)
    for kind, p0, p1 in tab:
        lo, hi = (p0, p0 + p1) if kind == PR.TABLE_UNIFORM else (p0 - 12 * p1, p0 + 12 * p1)
        x = 0.5 * (hi - lo) * g + 0.5 * (hi + lo)
        xs.append(x)
        ws.append(0.5 * (hi - lo) * gw)
        dens.append(np.full_like(x, 1.0 / p1) if kind == PR.TABLE_UNIFORM else
                    np.exp(-0.5 * ((x - p0) / p1)**2) / (p1 * math.sqrt(2 * math.pi)))
    v = np.stack(np.meshgrid(xs[0], xs[1], indexing="ij"), axis=-1).reshape(-1, 2)
    like = np.exp(prob.loglikelihood_many(v)).reshape(400, 400)
    return math.log(np.einsum("i,j,ij->", ws[0] * dens[0], ws[1] * dens[1], like))


@pytest.mark.parametrize("rows", [[("uniform", -12.0, 14.0), ("uniform", -9.0, 11.0)],
                                  [("uniform", -12.0, 14.0), ("normal", 0.5, 2.0)],
                                  [("normal", -1.0, 3.0), ("normal", 0.5, 2.0)]])
def test_logz_truth_against_quadrature(rows):
    """Tolerance 1e-6: the truth neglects < 2e-9 of mass per side of a uniform row (6 sigma), the rule's own error is
    below 1e-10 here (nodes 0.07 sigma apart at the widest), and fp64 sums of 160 000 terms add ~1e-13."""
    means = np.array([[-2.0, 1.0], [3.0, -1.5]])
    covs = np.array([[[1.0, 0.3], [0.3, 0.5]], [[0.4, -0.1], [-0.1, 0.8]]])
    prob = PR.gauss_mixture(means, covs, [0.3, 0.7], prior=rows)
    assert prob.logz_truth is not None
    assert abs(prob.logz_truth - _quad_logz(prob, means, covs)) < 1e-6
    one = PR.gauss_general(means[0], covs[0], prior=rows)
    assert abs(one.logz_truth - _quad_logz(one, means[:1], covs[:1])) < 1e-6


def test_logz_truth_is_none_where_it_is_not_analytic():
    eye = np.eye(2)
    assert PR.gauss_general([1.0, 1.0], eye, prior=[("uniform", -9, 9), ("loguniform", 0.1, 10.0)]).logz_truth is None
    assert PR.gauss_general([1.0, 1.0], eye, prior=[("uniform", -9, 9), ("uniform", 0.0, 10.0)]).logz_truth is None  # cut


def test_constructors_refuse_what_the_library_refuses():
    eye = np.eye(2)
    ok_rows = [("uniform", -1.0, 1.0), ("normal", 0.0, 1.0)]
    for rows in ([("uniform", 1.0, 1.0)], [("uniform", 2.0, 1.0)], [("normal", 0.0, 0.0)], [("normal", 0.0, -1.0)],
                 [("loguniform", 0.0, 1.0)], [("loguniform", 2.0, 1.0)], [("cauchy", 0.0, 1.0)],
                 [("uniform", float("nan"), 1.0)], [("normal", 0.0, float("inf"))], []):
        with pytest.raises(ValueError):
            PR.prior_table(rows)
    with pytest.raises(ValueError):  # nine components
        PR.gauss_mixture(np.zeros((9, 2)), eye, prior=ok_rows)
    with pytest.raises(ValueError):  # a table of another length
        PR.gauss_mixture(np.zeros((2, 2)), eye, prior=ok_rows + ok_rows)
    with pytest.raises(ValueError):  # not positive definite
        PR.gauss_general([0.0, 0.0], [[1.0, 2.0], [2.0, 1.0]], prior=ok_rows)
    with pytest.raises(ValueError):
        PR.gauss_general([0.0, float("nan")], eye, prior=ok_rows)
    with pytest.raises(ValueError):
        PR.gauss_mixture(np.zeros((2, 2)), eye, weights=[1.0, 0.0], prior=ok_rows)
    tab = PR.prior_table(ok_rows).ravel()
    good = np.concatenate([[1.0, 0.0], np.zeros(2), eye.ravel()])
    PR.Problem(2, PR.LIKE_GAUSS_MIX, good, PR.PRIOR_TABLE, tab)
    for lp, pp in ((np.concatenate([[0.0], good[1:]]), tab), (np.concatenate([[9.0], good[1:]]), tab),
                   (np.concatenate([[1.5], good[1:]]), tab), (good[:-1], tab), (np.append(good, 0.0), tab),
                   (good, tab[:-1]), (good, np.append(tab, 0.0)),
                   (good, np.array([3.0, 0, 1, 0, 0, 1])), (good, np.array([-1.0, 0, 1, 0, 0, 1])),
                   (good, np.array([0.0, 0, 0, 1, 0, 1])), (good, np.array([0.0, 0, 1, 1, 0, -1.0])),
                   (np.concatenate([good[:4], [0.0, 0, 0, 1]]), tab), (np.concatenate([good[:4], [1.0, 0, 0, -1]]), tab),
                   (np.concatenate([[1.0, float("inf")], good[2:]]), tab)):
        with pytest.raises(ValueError):
            PR.Problem(2, PR.LIKE_GAUSS_MIX, lp, PR.PRIOR_TABLE, pp)


@pytest.mark.parametrize("kind,m,ndim", [("mix", 1, 2), ("mix", 2, 5), ("mix", 4, 9), ("mix", 5, 25), ("mix", 8, 32),
                                         ("mix", 1, 40), ("mixed", 2, 2), ("mixed", 2, 5), ("mixed", 2, 9),
                                         ("mixed", 4, 16), ("mixed", 2, 40)])
def test_sampler_starts_are_decidable_on_the_host(kind, m, ndim):
    """The start points the GPU tests use (problem_ext_hp_ref.sampler_case, the same seeds): an accept decision
    logl > loglstar can be compared between two evaluators only where |logl - loglstar| exceeds both bounds
    (DESIGN 3.1c); with the host callables alone at most 2 % of a case's walkers may fall inside that band."""
    prob = X.mixture_problem("random", ndim, m, seed=60 + ndim) if kind == "mix" else X.mixed_problem(ndim, m)
    for seed in (2000 + ndim, 2100 + ndim):
        case = X.sampler_case(prob, seed)
        u = case["u0"]
        assert u.shape == (X.K, ndim)
        logl = prob.loglikelihood_many(prob.prior_transform_many(u))
        band = 2.0 * X.logl_bound_from_u(prob, u)
        assert np.mean(np.abs(logl - case["loglstar"]) <= band) <= 0.02
        assert np.all(np.abs(logl - case["logl0"].astype(np.float64)) <= X.logl_bound_from_u(prob, u))
