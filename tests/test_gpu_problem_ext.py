"""DH_PRIOR_TABLE / DH_LIKE_GAUSS_MIX on the device: every evaluator and every evaluating entry point against the
high-precision reference of tests/problem_ext_hp_ref.py within its bounds, the C ABI of dh_problem_create_ex, the form
rule, and the resident loop on problems with an analytic evidence.

The device is never its own reference: v is held to prior_hp(u), logl to loglike_hp(v_device).  Each check prints its
worst error / bound ratio (pytest -s); the module prints the table per (evaluator, id) when it is done."""
import ctypes as C
import math

import numpy as np
import pytest

import hp_ref as H
import problem_ext_hp_ref as X
from dynesty_amd import problems as PR

pytestmark = pytest.mark.gpu

K = X.K  # two full wavefronts + two live lanes
LD = np.longdouble
RATIOS = {}


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    c = _lib.Context(0)
    yield c
    print("\nworst error / bound per (evaluator, id): v, logl")
    for (ev, what), (rv, rl) in sorted(RATIOS.items()):
        print(f"RATIO {ev:18s} {what:8s} {rv:6.3f} {rl:6.3f}")
    c.close()


def note(evaluator, what, r):
    old = RATIOS.get((evaluator, what), (0.0, 0.0))
    RATIOS[(evaluator, what)] = (max(old[0], r[0]), max(old[1], r[1]))


def eval_and_check(ctx, prob, u, evaluator, what):
    v, logl = ctx.problem_eval(prob, u)
    note(evaluator, what, X.check(prob, u, v, logl, what=f"eval {prob.name}"))
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(logl))
    for k in (1, 64, 65):  # partial last wavefronts: the same walkers, bit for bit
        vk, lk = ctx.problem_eval(prob, u[:k])
        np.testing.assert_array_equal(vk, v[:k])
        np.testing.assert_array_equal(lk, logl[:k])
    return v, logl


# ---------------------------------------------------------------------------------------------------------
# a. dh_problem_eval
# ---------------------------------------------------------------------------------------------------------
LANE_DIMS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 25, 32]
WIDE_DIMS = [33, 65, 200]


@pytest.mark.parametrize("ndim", LANE_DIMS + WIDE_DIMS)
def test_problem_eval_table(ctx, ndim):
    """All three kinds, adjacent coordinates different, the unit-cube points from hp_ref's sweep (tails, centre, the
    AS 241 switch points), the log-uniform rows over twelve decades; under the iid likelihood (an old id: the pair goes
    through dh_problem_create_ex like every other)."""
    tab = PR.prior_table(X.mixed_rows(ndim, offset=ndim))
    prob = PR.Problem(ndim, PR.LIKE_GAUSS_IID, [-0.5 * ndim * math.log(2 * math.pi)], PR.PRIOR_TABLE, tab.ravel(),
                      name=f"iid+table/{ndim}")
    u = H.sweep_matrix(K, ndim, 1000 + ndim)
    eval_and_check(ctx, prob, u, "problem_eval" if ndim <= 32 else "problem_eval/wide", "table")


def mixture_eval_params():
    out = []
    for d in LANE_DIMS + WIDE_DIMS:  # every dimension: two random components
        out.append(("random", 2, d))
    for case in X.MIX_CASES:  # every case at every M: a FULL (5) and a padded (9) lane kernel
        for m in (1, 2, 4, 5, 8):
            out.append((case, m, 5 if m % 2 else 9))
    out += [("far_means", 1, 40), ("separated", 5, 33), ("tiny_weight", 8, 65), ("identical", 4, 40)]  # wide
    return sorted(set(out))


@pytest.mark.parametrize("case,m,ndim", mixture_eval_params())
def test_problem_eval_mixture(ctx, case, m, ndim):
    prob = X.mixture_problem(case, ndim, m, seed=300 + 7 * m + ndim)
    u = X.near_component_u(prob, K, 1300 + ndim)
    v, logl = eval_and_check(ctx, prob, u, "problem_eval" if ndim <= 32 else "problem_eval/wide", f"mix{m}")
    a = X._components_hp(prob, v).astype(np.float64)
    bound = X.loglike_bound(prob, v)
    if case == "separated" and m > 1:  # every other exp underflows: the largest a_m to its bound
        assert np.all(np.abs(logl - a.max(axis=1)) <= bound)
    if m == 1:  # no exp, no log: the quadratic form's own bound
        assert np.all(np.abs(logl - a[:, 0]) <= bound)


def test_old_ids_pair_with_the_new(ctx):
    """A mixture under the AFFINE prior and the correlated Normal / eggbox under a table."""
    n = 6
    means, covs, w = X.mixture_parts("random", n, 3, 11)
    base = PR.gauss_mixture(means, covs, w, prior=X.uniform_rows(n))
    prob = PR.Problem(n, PR.LIKE_GAUSS_MIX, base.like_par, PR.PRIOR_AFFINE, [4.0, 0.5], name="mix3+affine/6")
    u = np.random.default_rng(5).random((K, n))
    eval_and_check(ctx, prob, u, "problem_eval", "mix+old")
    for n in (6, 40):
        P = H.spd_plus_antisym(n, 9, 0.1)
        tab = PR.prior_table(X.uniform_rows(n, -3.0, 3.0))
        prob = PR.Problem(n, PR.LIKE_GAUSS_PREC, np.concatenate([[-1.0], P.ravel()]), PR.PRIOR_TABLE, tab.ravel(),
                          name=f"prec+table/{n}")
        eval_and_check(ctx, prob, np.random.default_rng(6).random((K, n)), "problem_eval", "old+table")
    tab = PR.prior_table([("uniform", 0.0, 1.0), ("uniform", 0.25, 0.75)])
    prob = PR.Problem(2, PR.LIKE_EGGBOX, [H.TMAX], PR.PRIOR_TABLE, tab.ravel(), name="eggbox+table/2")
    eval_and_check(ctx, prob, np.random.default_rng(7).random((K, 2)), "problem_eval", "old+table")


# ---------------------------------------------------------------------------------------------------------
# b. samplers
# ---------------------------------------------------------------------------------------------------------
mixed_problem, sampler_case = X.mixed_problem, X.sampler_case


def check_sampler(name, what, prob, case, out, moved):
    u, v, logl = out["u"], out["v"], out["logl"]
    assert np.all((u > 0.0) & (u < 1.0))
    note(name, what, X.check(prob, u, v, logl, what=f"{name} {prob.name}"))
    assert np.all(logl[moved] > case["loglstar"])
    if case.get("u0") is not None and not np.all(moved):
        still = np.flatnonzero(~moved)
        np.testing.assert_array_equal(u[still], case["u0"][still])
        err = np.abs(logl[still].astype(LD) - case["logl0"][still]).astype(np.float64)
        assert np.all(err <= X.logl_bound_from_u(prob, case["u0"][still]))
    frac = float(np.mean(moved))
    print(f"{name} {prob.name}: {frac:.2f} of the walkers moved")
    assert frac >= 0.25, frac


def run_rwalk(ctx, prob, case, form=0, philox=False):
    if philox:
        out = ctx.rwalk_batch_philox(prob, case["u0"], case["axes"], case["scale"], case["loglstar"], 8, seed=31,
                                     sequence0=5, offset=0)
    else:
        ctx.set_rwalk_form(form)
        try:
            st = ctx.seed_children([3, prob.ndim], 0, K)
            out = ctx.rwalk_batch(prob, case["u0"], case["axes"], case["scale"], case["loglstar"], 8, st)
        finally:
            ctx.set_rwalk_form(0)
    assert np.all(out["accept"] + out["reject"] == 8)
    return out, out["accept"] > 0


def run_slice(ctx, prob, case, principal=False):
    st = ctx.seed_children([4, prob.ndim], 0, K)
    out = ctx.slice_batch(prob, case["u0"], case["axes"], case["scale"], case["loglstar"], 2, st, principal=principal)
    return out, np.any(out["u"] != case["u0"], axis=1)


def run_unif(ctx, prob, case):
    best = int(np.argmax(case["logl0"]))
    out = ctx.unif_batch(prob, case["loglstar"], ctx.seed_children([5, prob.ndim], 0, K), ctrs=case["u0"][best],
                         axes=np.eye(prob.ndim) * (0.05 * case["spread"]), max_tries=100000)
    assert np.all(out["ncalls"] >= 1)
    return out, np.ones(K, dtype=bool)


QUAD_DIMS = [2, 4, 8, 16, 27, 32, 5, 9, 13, 25, 29]  # plain forms, then n = 4 (NR - 1) + 1 (test_gpu_evaluators.py)
ENTRIES = {
    # name: (runner, [(ndim, M)]); rwalk/quad: M <= 4 is the four-lane kernel at every NR = 1..8 and both MT
    "rwalk/quad": (lambda c, p, s: run_rwalk(c, p, s, form=0), [(d, (1, 2, 4)[i % 3]) for i, d in enumerate(QUAD_DIMS)]),
    "rwalk/lane": (lambda c, p, s: run_rwalk(c, p, s, form=1), [(3, 2), (7, 4), (25, 5), (32, 1)]),
    "rwalk/form0-M>4": (lambda c, p, s: run_rwalk(c, p, s, form=0), [(9, 5), (25, 8)]),  # the rule: the lane kernel
    "rwalk/philox": (lambda c, p, s: run_rwalk(c, p, s, philox=True), [(5, 4), (25, 2)]),  # four-lane, Philox items
    "rwalk/wide": (lambda c, p, s: run_rwalk(c, p, s, form=0), [(40, 1)]),
    "rslice": (lambda c, p, s: run_slice(c, p, s), [(3, 2), (25, 4)]),
    "slice": (lambda c, p, s: run_slice(c, p, s, principal=True), [(2, 1), (5, 2)]),
    "rslice/wide": (lambda c, p, s: run_slice(c, p, s), [(40, 2)]),
    "unif": (run_unif, [(2, 8), (7, 1)]),
}
MIXED_DIMS = {"rwalk/quad": [2, 5, 9, 16], "rwalk/lane": [3], "rwalk/philox": [5], "rwalk/wide": [40], "rslice": [3],
              "slice": [2], "rslice/wide": [40], "unif": [2]}


def sampler_params():
    out = []
    for name, (_, cases) in ENTRIES.items():
        for d, m in cases:
            out.append(pytest.param(name, "mix", m, d, id=f"{name}-mix{m}-{d}"))
        for d in MIXED_DIMS.get(name, []):  # adjacent coordinates of different kinds: different kinds over the sub-lanes
            out.append(pytest.param(name, "mixed", 2, d, id=f"{name}-mixed-{d}"))
    out.append(pytest.param("rslice/wide", "iid+table", 0, 40, id="rslice/wide-iid+table-40"))  # beside the regF gate
    out.append(pytest.param("rwalk/quad", "iid+table", 0, 9, id="rwalk/quad-iid+table-9"))
    return out


def iid_table_problem(ndim):
    tab = PR.prior_table(X.uniform_rows(ndim, -6.0, 6.0))
    return PR.Problem(ndim, PR.LIKE_GAUSS_IID, [-0.5 * ndim * math.log(2 * math.pi)], PR.PRIOR_TABLE, tab.ravel(),
                      name=f"iid+table/{ndim}")


def iid_table_case(prob, seed):
    rng = np.random.default_rng(seed)
    d, spread = prob.ndim, 0.05
    u0 = np.clip(0.5 + spread * rng.standard_normal((K + 24, d)), 1e-3, 1 - 1e-3)
    l0 = X.loglike_hp(prob, X.prior_hp(prob, u0))
    loglstar = float(np.quantile(l0.astype(np.float64), 0.05))
    keep = np.flatnonzero(l0 > LD(loglstar))[:K]
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    return dict(u0=np.ascontiguousarray(u0[keep]), logl0=l0[keep], loglstar=loglstar,
                axes=q * (0.3 * spread * rng.uniform(0.8, 1.6, size=d)), scale=0.7, spread=spread)


@pytest.mark.parametrize("name,kind,m,ndim", sampler_params())
def test_sampler_returns(ctx, name, kind, m, ndim):
    """The (u, v, logl) an entry point returns: v and logl within bound of the reference at the returned u / v, the
    threshold beaten wherever the walker moved, the start returned untouched where it did not."""
    if kind == "iid+table":
        prob = iid_table_problem(ndim)
        case = iid_table_case(prob, 2000 + ndim)
    else:
        prob = X.mixture_problem("random", ndim, m, seed=60 + ndim) if kind == "mix" else mixed_problem(ndim, m)
        case = sampler_case(prob, 2000 + ndim)
    out, moved = ENTRIES[name][0](ctx, prob, case)
    if name.startswith("unif"):
        case = dict(case, u0=None)
    check_sampler(name, kind if kind != "mix" else f"mix{m}", prob, case, out, moved)


def test_rwalk_propose_points_evaluate_within_bound(ctx):
    """dh_rwalk_propose carries no problem; its proposals inside the cube go through dh_problem_eval."""
    prob = mixed_problem(5)
    case = sampler_case(prob, 2005)
    up, inside, _ = ctx.rwalk_propose(case["u0"], case["axes"], case["scale"], ctx.seed_children([6, 5], 0, K))
    assert inside.mean() > 0.9
    v, logl = ctx.problem_eval(prob, up[inside])
    note("rwalk_propose", "mixed", X.check(prob, up[inside], v, logl, what="rwalk_propose mixed"))


def two_forms(ctx, prob, seed):
    case = sampler_case(prob, seed)
    a, _ = run_rwalk(ctx, prob, case, form=0)
    b, _ = run_rwalk(ctx, prob, case, form=1)
    return a, b


@pytest.mark.parametrize("ndim", QUAD_DIMS)
def test_four_lane_and_lane_forms_agree(ctx, ndim):
    """M <= 4: rwalk form 0 is the four-lane kernel, form 1 the lane kernel -- the same walk on the same streams.
    Generator end states equal exactly for every walker (a step draws its items whatever it decides); accept counts
    equal and coordinates equal to 1e-13 for every walker whose decisions were decidable: a proposal within rounding of
    loglstar may be taken by one form only, and at most 2 % of a case's walkers may be set aside for
    that.  That form 0 ran other code shows in the last bits of logl: the four-lane kernel sums P_m d by matrix
    instructions over four lanes (test_gpu_evaluators.py::test_form0_takes_the_quad_kernel argues the same way)."""
    for m in (1, 2, 4):
        for prob in (X.mixture_problem("random", ndim, m, seed=60 + ndim), mixed_problem(ndim, m)):
            a, b = two_forms(ctx, prob, 2100 + ndim)
            np.testing.assert_array_equal(a["rng_out"], b["rng_out"])
            np.testing.assert_array_equal(a["accept"] + a["reject"], b["accept"] + b["reject"])
            same = np.all(np.abs(a["u"] - b["u"]) <= 1e-13, axis=1) & (a["accept"] == b["accept"])
            print(f"forms {prob.name}: {int((~same).sum())} of {K} walkers set aside")
            assert (~same).sum() <= int(0.02 * K), np.flatnonzero(~same)
            # each form's logl within its bound at its own v, plus the gradient times whatever last bits the v differ in
            tol = X.loglike_bound(prob, a["v"]) + X.loglike_bound(prob, b["v"]) + \
                np.sum(X.loglike_grad_abs(prob, a["v"]) * np.abs(a["v"] - b["v"]), axis=1)
            assert np.all(np.abs(a["logl"] - b["logl"])[same] <= tol[same])
            assert np.all(np.isfinite(a["logl"])) and np.all(np.isfinite(b["logl"]))
            if ndim >= 8 and prob.like_id == PR.LIKE_GAUSS_MIX:
                assert np.any(a["logl"] != b["logl"])


@pytest.mark.parametrize("m,ndim", [(5, 8), (8, 32), (5, 25), (8, 2)])
def test_form_rule_larger_mixtures_take_the_lane_kernel(ctx, m, ndim):
    """the four-lane kernel stages at most four components; a mixture of M > 4 runs the lane-per-walker
    kernel at every ndim -- a function of (ndim, M) alone -- so for it form 0 and form 1 are one and the same kernel,
    equal bit for bit in everything, while M = 4 (the test above) differs in the last bits of logl."""
    prob = X.mixture_problem("random", ndim, m, seed=60 + ndim)
    a, b = two_forms(ctx, prob, 2100 + ndim)
    for key in ("accept", "reject", "rng_out", "u", "v", "logl"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert np.all(np.isfinite(a["logl"]))


# ---------------------------------------------------------------------------------------------------------
# c. dh_problem_create_ex
# ---------------------------------------------------------------------------------------------------------
def _create(ctx, fn, ndim, lid, lp, pid, pp, nl=None, npp=None):
    lp = None if lp is None else np.ascontiguousarray(lp, dtype=np.float64)
    pp = None if pp is None else np.ascontiguousarray(pp, dtype=np.float64)
    return getattr(ctx.lib, fn)(ctx.handle, ndim, lid, None if lp is None else lp.ctypes.data_as(C.c_void_p),
                                (0 if lp is None else lp.size) if nl is None else nl, pid,
                                None if pp is None or pp.size == 0 else pp.ctypes.data_as(C.c_void_p),
                                (0 if pp is None else pp.size) if npp is None else npp)


def test_problem_create_ex_refusals(ctx):
    from dynesty_amd import _lib
    eye = np.eye(2).ravel()
    good = np.concatenate([[1.0, 0.0], np.zeros(2), eye])
    two = np.concatenate([[2.0], good[1:], good[1:]])
    tab = PR.prior_table([("uniform", -1.0, 1.0), ("normal", 0.0, 1.0)]).ravel()
    nan, inf = float("nan"), float("inf")
    bad = [(2, 3, np.concatenate([[0.0], good[1:]]), 3, tab), (2, 3, np.concatenate([[9.0], good[1:]]), 3, tab),  # M
           (2, 3, np.concatenate([[1.5], good[1:]]), 3, tab), (2, 3, np.concatenate([[-1.0], good[1:]]), 3, tab),
           (2, 3, good[:-1], 3, tab), (2, 3, np.append(good, 0.0), 3, tab), (2, 3, two[:-1], 3, tab),  # 1 + M (1 + n + n^2)
           (2, 3, good, 3, tab[:-1]), (2, 3, good, 3, np.append(tab, 0.0)), (2, 0, [0.5], 3, tab[:3]),  # 3 n
           (2, 3, good, 3, [3.0, 0, 1, 0, 0, 1]), (2, 3, good, 3, [-1.0, 0, 1, 0, 0, 1]), (2, 3, good, 3, [0.5, 0, 1, 0, 0, 1]),
           (2, 3, np.concatenate([[1.0, nan], good[2:]]), 3, tab), (2, 3, np.concatenate([good[:3], [inf], good[4:]]), 3, tab),
           (2, 3, good, 3, [0.0, nan, 1, 0, 0, 1]), (2, 0, [inf], 3, tab), (2, 3, good, 1, [inf, 0.0]),  # not finite
           (2, 3, good, 3, [0.0, 0, 0, 1, 0, 1]), (2, 3, good, 3, [0.0, 0, -1, 1, 0, 1]), (2, 3, good, 3, [0.0, 0, 1, 1, 0, 0]),
           (2, 3, good, 3, [0.0, 0, 1, 1, 0, -2.0]),  # p1 <= 0, kinds 0 and 1
           (2, 3, np.concatenate([good[:4], [0.0, 0, 0, 1]]), 3, tab), (2, 3, np.concatenate([good[:4], [1.0, 0, 0, -1]]), 3, tab),
           (2, 3, np.concatenate([two[:-1], [-1.0]]), 3, tab),  # a diagonal entry of a P_m
           (0, 3, good, 3, tab), (2, 4, good, 3, tab), (2, 3, good, 4, tab), (2, -1, good, 3, tab), (2, 3, good, -1, tab),
           (2, 3, good, 1, [1.0]), (3, 1, np.zeros(9), 3, np.tile([0.0, 0, 1], 3))]  # old ids: their own counts
    for args in bad:
        assert _create(ctx, "dh_problem_create_ex", *args) == _lib.ERR_ARG, args
        assert ctx.lib.dh_last_error(ctx.handle)
    assert _create(ctx, "dh_problem_create_ex", 2, 3, None, 3, tab, nl=9) == _lib.ERR_ARG  # null pointers
    assert _create(ctx, "dh_problem_create_ex", 2, 3, good, 3, None, npp=6) == _lib.ERR_ARG
    # a log-uniform row with p1 <= 0 is not refused (the list names kinds 0 and 1), and what is accepted is destroyed
    for args in [(2, 3, good, 3, tab), (2, 3, two, 3, [2.0, 0, -1, 2.0, 0, 1]), (2, 3, good, 0, None), (2, 2, [H.TMAX], 3, tab)]:
        h = _create(ctx, "dh_problem_create_ex", *args)
        assert h >= 0, (args, ctx.lib.dh_last_error(ctx.handle))
        assert ctx.lib.dh_problem_destroy(ctx.handle, h) == 0
    # dh_problem_create still refuses the new ids
    assert _create(ctx, "dh_problem_create", 2, 3, good, 0, None) == _lib.ERR_ARG
    assert _create(ctx, "dh_problem_create", 2, 0, [0.5], 3, tab) == _lib.ERR_ARG


@pytest.mark.parametrize("like,prior", H.PAIRS)
@pytest.mark.parametrize("ndim", [5, 40])
def test_old_pairs_through_both_entry_points_evaluate_the_same_bits(ctx, like, prior, ndim):
    prob = H.make_problem(like, prior, ndim, seed=8, asym=0.1 if like == "prec" else 0.0)
    u = H.sweep_matrix(K, ndim, 77)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    got = []
    for fn in ("dh_problem_create", "dh_problem_create_ex"):
        h = _create(ctx, fn, ndim, prob.like_id, prob.like_par, prob.prior_id, prob.prior_par)
        assert h >= 0
        v, logl = np.empty_like(u), np.empty(K)
        assert ctx.lib.dh_problem_eval(ctx.handle, h, K, ptr(u), ptr(v), ptr(logl)) == 0
        assert ctx.lib.dh_problem_destroy(ctx.handle, h) == 0
        got.append((v, logl))
    np.testing.assert_array_equal(got[0][0], got[1][0])
    np.testing.assert_array_equal(got[0][1], got[1][1])


# ---------------------------------------------------------------------------------------------------------
# d. resident loop
# ---------------------------------------------------------------------------------------------------------
RUNS, NLIVE = 16, 400


def two_mode_problem():
    """5-D, weights 0.3 / 0.7, unit-covariance components 6 sigma apart along the first axis, under a mixed uniform /
    normal table (the normal rows wide against the likelihood)."""
    means = np.zeros((2, 5))
    means[0, 0], means[1, 0] = -3.0, 3.0
    rows = [("uniform", -12.0, 12.0), ("normal", 0.5, 4.0), ("uniform", -10.0, 11.0), ("normal", -0.5, 3.0),
            ("uniform", -9.0, 9.0)]
    return PR.gauss_mixture(means, np.eye(5), [0.3, 0.7], prior=rows, name="two_mode5"), means


def run_fractions(prob, r, means):
    """Per run: the posterior mass nearer means[0], by the rectangle rule on the run's own dead and live points."""
    out = []
    for run in range(RUNS):
        n = int(r["niter"][run])
        u = np.concatenate([r["dead_u"][run, :n], r["live_u"][run]])
        logl = np.concatenate([r["dead_logl"][run, :n], r["live_logl"][run]])
        x = np.exp(-np.arange(1, n + 1) / NLIVE)
        dx = np.concatenate([-np.diff(np.concatenate([[1.0], x])), np.full(NLIVE, x[-1] / NLIVE)])
        w = np.exp(logl - logl.max()) * dx
        v = prob.prior_transform_many(u)
        near0 = np.sum((v - means[0])**2, axis=1) < np.sum((v - means[1])**2, axis=1)
        out.append(float(np.sum(w[near0]) / np.sum(w)))
    return np.array(out)


def logz_gate(r, truth, what):
    lz = r["logz"]
    mean, se = lz.mean(), lz.std(ddof=1) / math.sqrt(len(lz))
    print(f"[{what}] ln Z {mean:.4f} +- {se:.4f} (se), analytic {truth:.4f}, gate {max(0.05, 3.0 * se):.4f}")
    assert np.all(r["status"] == 0), r["status"]
    assert abs(mean - truth) <= max(0.05, 3.0 * se), (mean, se, truth)


@pytest.mark.parametrize("sample", ["rwalk", "rslice"])
def test_resident_loop_two_modes(ctx, sample):
    """ln Z against the analytic value within max(0.05, 3 se) (the form of test_gpu_logz_gate.py with the ensemble's
    own standard error and zero on the analytic side); the merged posterior mass nearer each mean against its weight
    within three standard errors of the per-run fractions; the merged samples are dh_problem_eval's, bit for bit."""
    prob, means = two_mode_problem()
    assert prob.logz_truth is not None
    kw = dict(walks=25) if sample == "rwalk" else dict(slices=8)
    r = ctx.ns_ensemble(prob, RUNS, NLIVE, 32, bound="multi", entropy=[2027, 5], dlogz=0.01, sample=sample,
                        max_iter=20000, want_samples=True, keep=True, **kw)
    logz_gate(r, prob.logz_truth, f"two_mode5/{sample}")
    frac = run_fractions(prob, r, means)
    se = frac.std(ddof=1) / math.sqrt(RUNS)
    d = ctx.merge_kept(prob)
    m = d.to_merged_run()
    w = d.importance_weights()
    near0 = np.sum((m.samples - means[0])**2, axis=1) < np.sum((m.samples - means[1])**2, axis=1)
    f0 = float(np.sum(w[near0]) / np.sum(w))
    print(f"[two_mode5/{sample}] merged mass nearer mean 0: {f0:.4f} (weight 0.3), per-run {frac.mean():.4f} +- {se:.4f}")
    assert abs(f0 - 0.3) <= 3.0 * se and abs((1.0 - f0) - 0.7) <= 3.0 * se, (f0, se)
    v, _ = ctx.problem_eval(prob, m.samples_u)
    np.testing.assert_array_equal(m.samples, v)
    worst = X.check_from_u(prob, m.samples_u[::37], m.logl[::37], what=f"merged two_mode5/{sample}")
    note(f"ns/{sample}", "mix2", (0.0, worst))


def test_resident_loop_general_gaussian_wide(ctx):
    """An M = 1 general Gaussian at D = 40 (mean off the origin, correlated) under a uniform table: the wide path."""
    n = 40
    rng = np.random.default_rng(40)
    mean = rng.uniform(-2.0, 2.0, n)
    cov = X.spd(n, 41)
    sd = np.sqrt(np.diag(cov))
    rows = [("uniform", mean[i] - 8.0 * sd[i] - 0.1 * i, mean[i] + 8.0 * sd[i] + 0.05 * i) for i in range(n)]
    prob = PR.gauss_general(mean, cov, prior=rows, name="general40")
    assert prob.logz_truth is not None
    # slices: a slice along one random direction renews about 1 / D of a point's coordinates, so independence of the
    # start takes a few times D of them (the reference's default, 3 + D, is known to leave ln Z high at this D)
    r = ctx.ns_ensemble(prob, RUNS, NLIVE, 64, bound="single", entropy=[2027, 40], dlogz=0.1, sample="rslice",
                        slices=3 * n, max_iter=60000, want_samples=True)
    print(f"[general40/rslice] iterations per run {r['niter'].mean():.0f}, calls {r['ncall'].mean():.3g}")
    logz_gate(r, prob.logz_truth, "general40/rslice")
    run = 3
    nit = int(r["niter"][run])
    worst = X.check_from_u(prob, r["dead_u"][run, :nit:97], r["dead_logl"][run, :nit:97], what="ns general40")
    note("ns/rslice/wide", "mix1", (0.0, worst))


def test_resident_loop_two_modes_equals_its_host_mirror(ctx):
    """tests/resident_mirror.py takes the problem as it is: one mirrored run of the two-mode case at K = 4 agrees with
    the device loop death for death over the first 300 deaths (tolerances: tests/test_gpu_resident_mirror.py)."""
    from resident_mirror import mirror_run
    prob, _ = two_mode_problem()
    ent, fills = [2027, 4, 5], 200
    r = ctx.ns_ensemble(prob, 2, NLIVE, 4, walks=25, bound="multi", dlogz=0.01, entropy=ent, rebuild_every=1,
                        want_samples=True, max_fills=fills, max_iter=20000)
    m = mirror_run(ctx, prob, NLIVE, 4, 25, "multi", ent, 1, 0.01, max_fills=fills)
    n = 300
    assert int(r["niter"][1]) >= n and m["niter"] >= n, (r["niter"], m["niter"])
    np.testing.assert_array_equal(r["dead_id"][1, :n], np.array(m["dead_slot"])[:n])
    np.testing.assert_allclose(r["dead_logl"][1, :n], np.array(m["dead_logl"])[:n], rtol=1e-6, atol=0)
    X.check_from_u(prob, r["dead_u"][1, :n:7], r["dead_logl"][1, :n:7], what="mirror two_mode5")
