"""Every device evaluator of prior_transform / loglikelihood against the high-precision reference of
tests/hp_ref.py, entry point by entry point, all nine (likelihood, prior) pairs, within derived error bounds.

The device is never its own reference here: v is held to prior_hp(u), logl to loglike_hp(v_device).
Each check prints its worst error / bound ratio (pytest -s); the module prints the table of worst ratios per
(evaluator, pair) when it is done."""
import ctypes as C

import numpy as np
import pytest

import hp_ref as H
from dynesty_amd import problems as PR

pytestmark = pytest.mark.gpu

K = 130  # two full wavefronts + two live lanes; two quad workgroups + a partial one
LD = np.longdouble
STRIDE = np.r_[0:8, K - 8:K]  # NORMAL priors after a sampler: the first wavefront's first 8 and the last 8 walkers
RATIOS = {}


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    c = _lib.Context(0)
    yield c
    print("\nworst error / bound per (evaluator, pair): v, logl")
    for (ev, pair), (rv, rl) in sorted(RATIOS.items()):
        print(f"RATIO {ev:16s} {pair:16s} {rv:6.3f} {rl:6.3f}")
    c.close()


def note(evaluator, prob, r):
    pair = prob.name.split("/")[0]
    old = RATIOS.get((evaluator, pair), (0.0, 0.0))
    RATIOS[(evaluator, pair)] = (max(old[0], r[0]), max(old[1], r[1]))


# ---------------------------------------------------------------------------------------------------------
# a. dh_problem_eval
# ---------------------------------------------------------------------------------------------------------
EVAL_DIMS = [1, 2, 3, 4, 5, 7, 8, 13, 25, 26, 32, 33, 64, 65, 200]


def eval_inputs(prob, seed):
    d = prob.ndim
    if prob.prior_id != PR.PRIOR_NORMAL:
        return np.random.default_rng(seed).random((K, d))
    u = H.sweep_matrix(K, d, seed)
    if d >= 64:
        # full and empty compaction of the wide evaluator's tail route: one walker all tails, one with none
        p = H.sweep()
        tail = p[np.abs(p - 0.5) > 0.425]
        mid = p[np.abs(p - 0.5) <= 0.425]
        u[K - 2] = tail[np.arange(d) % len(tail)]
        u[K - 1] = mid[np.arange(d) % len(mid)]
    return u


@pytest.mark.parametrize("ndim", EVAL_DIMS)
@pytest.mark.parametrize("like,prior", H.PAIRS)
def test_problem_eval(ctx, like, prior, ndim):
    prob = H.make_problem(like, prior, ndim, seed=40 + ndim)
    u = eval_inputs(prob, 1000 + ndim)
    v, logl = ctx.problem_eval(prob, u)
    note("problem_eval" if ndim <= 32 else "problem_eval/wide", prob, H.check(prob, u, v, logl, what=f"eval {prob.name}"))
    # a launch of fewer walkers computes the same walkers: partial last wavefronts, bit for bit (assert_array_equal
    # takes NaN for equal to NaN: the check above has already refused any)
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(logl))
    for k in (1, 64, 65):
        vk, lk = ctx.problem_eval(prob, u[:k])
        np.testing.assert_array_equal(vk, v[:k])
        np.testing.assert_array_equal(lk, logl[:k])


# ---------------------------------------------------------------------------------------------------------
# b. samplers
# ---------------------------------------------------------------------------------------------------------
_pool = {}


def normal_pools():
    """Start coordinates under a Normal prior come from two fixed pools (centre, tails), so that the reference's
    ndtri is computed once per distinct value and every start's exact likelihood is affordable."""
    if not _pool:
        rng = np.random.default_rng(77)
        _pool["mid"] = np.clip(0.5 + 0.05 * rng.standard_normal(256), 0.08, 0.92)
        lo = rng.uniform(1e-3, 0.075, 64)
        _pool["tail"] = np.concatenate([lo, 1.0 - rng.uniform(1e-3, 0.075, 64)])
    return _pool["mid"], _pool["tail"]


def spread_of(prob):
    if prob.prior_id == PR.PRIOR_NORMAL:
        return 0.05
    if prob.like_id == PR.LIKE_EGGBOX:
        return 0.012 if prob.prior_id == PR.PRIOR_IDENTITY else 0.003
    return 0.1 if prob.prior_id == PR.PRIOR_IDENTITY else 0.5 / (2.0 * prob.prior_par[0])


def sampler_case(prob, seed):
    """Start points, threshold and frame in the style of inputs.walker_case: K starts above the 5 % quantile of the
    starts' exact log-likelihoods; under a Normal prior a quarter of the coordinates sit in the tails."""
    d = prob.ndim
    rng = np.random.default_rng(seed)
    n0 = K + 24
    spread = spread_of(prob)
    if prob.prior_id == PR.PRIOR_NORMAL:
        mid, tail = normal_pools()
        u0 = np.where(rng.random((n0, d)) < 0.25, tail[rng.integers(len(tail), size=(n0, d))],
                      mid[rng.integers(len(mid), size=(n0, d))])
    else:
        u0 = np.clip(0.5 + spread * rng.standard_normal((n0, d)), 1e-3, 1 - 1e-3)
    v0 = H.prior_hp(prob, u0)
    l0 = H.loglike_hp(prob, v0)
    loglstar = float(np.quantile(l0.astype(np.float64), 0.05))
    keep = np.flatnonzero(l0 > LD(loglstar))[:K]
    assert len(keep) == K
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    # steps a fraction of the start cloud's width: about every second proposal stays above the threshold
    axes = q * (0.3 * spread * rng.uniform(0.8, 1.6, size=d))
    return dict(u0=np.ascontiguousarray(u0[keep]), v0=v0[keep], logl0=l0[keep], loglstar=loglstar, axes=axes,
                scale=0.7, spread=spread)


def start_bound(prob, case, rows):
    """|device logl at an unmoved start - exact logl of the start|: the likelihood bound at the exact v plus the prior's
    bound carried through |d logl / d v_i|."""
    v0 = case["v0"][rows].astype(np.float64)
    return H.loglike_bound(prob, v0) + np.sum(H.loglike_grad_abs(prob, v0) * H.prior_bound(prob, case["u0"][rows]), axis=1)


def check_sampler(name, prob, case, out, moved):
    u, v, logl = out["u"], out["v"], out["logl"]
    assert np.all((u > 0.0) & (u < 1.0))
    rows = STRIDE if prob.prior_id == PR.PRIOR_NORMAL else np.arange(K)
    note(name, prob, H.check(prob, u, v, logl, rows=rows, what=f"{name} {prob.name}"))
    assert np.all(logl[moved] > case["loglstar"])
    if case.get("u0") is not None and not np.all(moved):
        still = np.flatnonzero(~moved)
        np.testing.assert_array_equal(u[still], case["u0"][still])
        sr = np.intersect1d(still, rows)
        if len(sr):
            err = np.abs(logl[sr].astype(LD) - case["logl0"][sr]).astype(np.float64)
            assert np.all(err <= start_bound(prob, case, sr)), (err, start_bound(prob, case, sr))
    frac = float(np.mean(moved))
    print(f"{name} {prob.name}: {frac:.2f} of the walkers moved")
    assert frac >= 0.25, frac


def run_rwalk(ctx, prob, case, form=None, philox=False):
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


def run_slice(ctx, prob, case, principal=False, philox=False):
    if philox:
        out = ctx.slice_batch_philox(prob, case["u0"], case["axes"], case["scale"], case["loglstar"], 2, seed=32,
                                     sequence0=9, offset=0, principal=principal)
    else:
        st = ctx.seed_children([4, prob.ndim], 0, K)
        out = ctx.slice_batch(prob, case["u0"], case["axes"], case["scale"], case["loglstar"], 2, st,
                              principal=principal)
    return out, np.any(out["u"] != case["u0"], axis=1)


def run_unif(ctx, prob, case, philox=False):
    # a small ball around the best start: nearly every draw beats the threshold (max_tries guards the rest)
    best = int(np.argmax(case["logl0"]))
    kw = dict(ctrs=case["u0"][best], axes=np.eye(prob.ndim) * (0.05 * case["spread"]), max_tries=100000)
    if philox:
        out = ctx.unif_batch_philox(prob, case["loglstar"], K, seed=33, sequence0=2, offset=0, **kw)
    else:
        out = ctx.unif_batch(prob, case["loglstar"], ctx.seed_children([5, prob.ndim], 0, K), **kw)
    assert np.all(out["ncalls"] >= 1)
    return out, np.ones(K, dtype=bool)


QUAD_DIMS = [2, 4, 8, 16, 27, 32, 5, 9, 13, 25, 29]  # plain forms, then the R1 forms n = 4 (NR - 1) + 1
LANE_DIMS = [1, 3, 7, 25, 26, 32]
ENTRIES = {
    # name: (runner, the dimensions the entry point distinguishes)
    "rwalk/quad": (lambda c, p, s: run_rwalk(c, p, s, form=0), QUAD_DIMS),
    "rwalk/lane": (lambda c, p, s: run_rwalk(c, p, s, form=1), LANE_DIMS),
    "rwalk/philox": (lambda c, p, s: run_rwalk(c, p, s, philox=True), [3, 7, 25]),
    "rwalk/wide": (lambda c, p, s: run_rwalk(c, p, s, form=0), [33, 65]),
    "rwalk/philox/wide": (lambda c, p, s: run_rwalk(c, p, s, philox=True), [33, 65]),
    "rslice": (lambda c, p, s: run_slice(c, p, s), [3, 25]),
    "slice": (lambda c, p, s: run_slice(c, p, s, principal=True), [2, 5]),
    "rslice/wide": (lambda c, p, s: run_slice(c, p, s), [7, 33, 65]),  # 7: no register form -> wide kernels
    "slice/wide": (lambda c, p, s: run_slice(c, p, s, principal=True), [33, 65]),
    "rslice/philox": (lambda c, p, s: run_slice(c, p, s, philox=True), [2, 5]),
    "rslice/philox/wide": (lambda c, p, s: run_slice(c, p, s, philox=True), [33, 65]),
    "slice/philox": (lambda c, p, s: run_slice(c, p, s, principal=True, philox=True), [3, 7]),
    "slice/philox/wide": (lambda c, p, s: run_slice(c, p, s, principal=True, philox=True), [33, 65]),
    "unif": (run_unif, [2, 7, 25]),
    "unif/wide": (run_unif, [33, 65]),
    "unif/philox": (lambda c, p, s: run_unif(c, p, s, philox=True), [3, 26]),
    "unif/philox/wide": (lambda c, p, s: run_unif(c, p, s, philox=True), [33, 65]),
}


def sampler_params():
    out = []
    for name, (_, dims) in ENTRIES.items():
        for i, (like, prior) in enumerate(H.PAIRS):
            # two or three dimensions per (entry point, pair), rotated so that every listed dimension is met
            pick = dims if len(dims) <= 3 else [dims[(3 * i + j) % len(dims)] for j in range(3)]
            for d in pick:
                out.append(pytest.param(name, like, prior, d, id=f"{name}-{like}+{prior}-{d}"))
    for name in ("rwalk/wide", "rslice/wide", "unif/wide"):
        out.append(pytest.param(name, "iid", "normal", 200, id=f"{name}-iid+normal-200"))
    return out


@pytest.mark.parametrize("name,like,prior,ndim", sampler_params())
def test_sampler_returns(ctx, name, like, prior, ndim):
    """The (u, v, logl) an entry point returns: v and logl within bound of the reference at the returned u / v, the
    threshold beaten wherever the walker moved, the start returned untouched where it did not."""
    prob = H.make_problem(like, prior, ndim, seed=60 + ndim)
    case = sampler_case(prob, 2000 + ndim)
    out, moved = ENTRIES[name][0](ctx, prob, case)
    if name.startswith("unif"):
        case = dict(case, u0=None)
    check_sampler(name, prob, case, out, moved)


@pytest.mark.parametrize("ndim", [16, 25])  # a plain and an R1 quad form
def test_form0_takes_the_quad_kernel(ctx, ndim):
    """rwalk form 0 at ndim == ncdim in 2..32 is the four-lane kernel, form 1 the lane kernel: same streams, same
    accept counts, coordinates equal to rounding but not a copy of each other.

    That form 0 ran other code is inferred from the rounding alone: the quad kernel sums P v by matrix instructions
    over four lanes, the lane kernel by a column sweep in one, so some of the 130 log-likelihoods differ in their last
    bits.  Should the two kernels ever share a summation order, the last assertion stops holding and this test needs
    another witness (a launch counter, say); it cannot pass by mistake."""
    prob = H.make_problem("prec", "affine", ndim, seed=60 + ndim)
    case = sampler_case(prob, 2000 + ndim)
    a, _ = run_rwalk(ctx, prob, case, form=0)
    b, _ = run_rwalk(ctx, prob, case, form=1)
    np.testing.assert_array_equal(a["accept"], b["accept"])
    np.testing.assert_array_equal(a["rng_out"], b["rng_out"])
    np.testing.assert_allclose(a["u"], b["u"], rtol=0, atol=1e-13)
    assert np.all(np.isfinite(a["logl"])) and np.all(np.isfinite(b["logl"]))
    assert np.any(a["logl"] != b["logl"])


# ---------------------------------------------------------------------------------------------------------
# c. asymmetric precision matrix
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [5, 7, 25, 26, 40])  # FULL, padded, R1-quad, padded, wide
@pytest.mark.parametrize("prior", ["affine", "identity"])
def test_asymmetric_precision_matrix(ctx, prior, ndim):
    """DH_LIKE_GAUSS_PREC with P = S + 0.1 A (A antisymmetric): every evaluator computes -v^T P v / 2 + c with the
    FULL quadratic form, whichever triangle of P it reads, and they agree with each other."""
    prob = H.make_problem("prec", prior, ndim, seed=70 + ndim, asym=0.1)
    P = prob.like_par[1:].reshape(ndim, ndim)
    assert np.abs(P - P.T).max() > 0.05
    case = sampler_case(prob, 3000 + ndim)
    v, logl = ctx.problem_eval(prob, case["u0"])
    note("asym/eval", prob, H.check(prob, case["u0"], v, logl, what=f"asym eval {prob.name}"))
    outs = {}
    for form in (0, 1):
        out, moved = run_rwalk(ctx, prob, case, form=form)
        note(f"asym/rwalk{form}", prob, H.check(prob, out["u"], out["v"], out["logl"], what=f"asym rwalk form {form} {prob.name}"))
        assert moved.mean() >= 0.25
        # the evaluator of dh_problem_eval at the same points: within twice the bound (plus the priors' own, carried)
        v2, l2 = ctx.problem_eval(prob, out["u"])
        tol = 2.0 * H.loglike_bound(prob, out["v"]) + \
            2.0 * np.sum(H.loglike_grad_abs(prob, out["v"]) * H.prior_bound(prob, out["u"]), axis=1)
        assert np.all(np.abs(l2 - out["logl"]) <= tol)
        outs[form] = out
    # the two kernel forms against each other, walker by walker: they draw the same proposals, so they end at the same
    # point unless one proposal fell within rounding of loglstar and was accepted by one form only (a handful of
    # ulps wide: not expected, but no error either -- at most one such walker is set aside, not the comparison).
    # Twice the bound, plus the gradient times whatever last bits the two v differ in.
    a, b = outs[0], outs[1]
    same = np.all(np.abs(a["u"] - b["u"]) <= 1e-13, axis=1) & (a["accept"] == b["accept"])
    assert same.sum() >= K - 1, np.flatnonzero(~same)
    tol = H.loglike_bound(prob, a["v"]) + H.loglike_bound(prob, b["v"]) + \
        np.sum(H.loglike_grad_abs(prob, a["v"]) * np.abs(a["v"] - b["v"]), axis=1)
    d = np.abs(a["logl"] - b["logl"])
    print(f"asym {prob.name}: form 0 against form 1, worst difference / tolerance {H.worst_ratio(d[same], tol[same]):.3f}")
    assert np.all(d[same] <= tol[same])


# ---------------------------------------------------------------------------------------------------------
# d. resident loop
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("like,prior,ndim,sample", [("prec", "normal", 5, "rwalk"), ("eggbox", "affine", 2, "unif"),
                                                    ("iid", "identity", 3, "rslice")])
def test_resident_loop_non_baseline_pairs(ctx, like, prior, ndim, sample):
    """dh_ns_ensemble on pairs outside the BASELINE four: every stored log-likelihood is the reference's at the
    stored unit-cube point (bound: the likelihood's at the exact v plus the prior's carried through the gradient),
    and the dead points come in order."""
    prob = H.make_problem(like, prior, ndim, seed=90 + ndim)
    kw = dict(walks=8) if sample == "rwalk" else dict(slices=2) if sample == "rslice" else {}
    r = ctx.ns_ensemble(prob, 2, nlive=64, queue_size=16, bound="single", entropy=[17, ndim], dlogz=0.01,
                        sample=sample, maxiter=200, max_iter=400, want_samples=True, **kw)
    assert np.all(r["status"] == 0), r["status"]
    worst = 0.0
    for run in range(2):
        n = int(r["niter"][run])
        assert 150 <= n <= 400
        dl = r["dead_logl"][run, :n]
        assert np.all(np.diff(dl) >= 0)
        u = np.concatenate([r["dead_u"][run, :n], r["live_u"][run]])
        got = np.concatenate([dl, r["live_logl"][run]])
        assert np.all((u > 0) & (u < 1))
        worst = max(worst, H.check_from_u(prob, u, got, what=f"ns_ensemble/{sample} run {run} {prob.name}"))
    note(f"ns/{sample}", prob, (0.0, worst))


# ---------------------------------------------------------------------------------------------------------
# dh_problem_create / destroy: argument handling
# ---------------------------------------------------------------------------------------------------------
def test_problem_create_refuses_bad_arguments(ctx):
    from dynesty_amd import _lib
    lib, h = ctx.lib, ctx.handle
    one = np.array([0.5])
    two = np.array([1.0, 0.0])
    p9 = np.zeros(10)

    def create(ndim, lid, lp, nl, pid, pp, npp):
        return lib.dh_problem_create(h, ndim, lid, None if lp is None else lp.ctypes.data_as(C.c_void_p), nl, pid,
                                     None if pp is None else pp.ctypes.data_as(C.c_void_p), npp)
    bad = [(0, 0, one, 1, 0, None, 0), (-3, 0, one, 1, 0, None, 0),  # ndim < 1
           (2, -1, one, 1, 0, None, 0), (2, 3, one, 1, 0, None, 0),  # likelihood id
           (2, 0, one, 1, -1, None, 0), (2, 0, one, 1, 3, two, 2),  # prior id
           (2, 0, one, 0, 0, None, 0),  # GAUSS_IID without c
           (3, 1, p9, 9, 1, two, 2),  # GAUSS_PREC: 1 + 9 parameters needed
           (2, 2, one, 0, 0, None, 0),  # EGGBOX without tmax
           (2, 0, one, 1, 1, two, 1), (2, 0, one, 1, 2, two, 0),  # AFFINE / NORMAL with fewer than two parameters
           (2, 0, None, 1, 0, None, 0), (2, 0, one, 1, 1, None, 2)]  # null pointers
    for args in bad:
        assert create(*args) == _lib.ERR_ARG, args
        assert lib.dh_last_error(h)
    # a destroyed handle is refused, its slot is the next create's
    a = create(3, 1, p9, 10, 1, two, 2)
    b = create(2, 0, one, 1, 0, None, 0)
    assert a >= 0 and b >= 0 and a != b
    assert lib.dh_problem_destroy(h, a) == 0
    u = np.full((1, 3), 0.5); v = np.empty((1, 3)); l = np.empty(1)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    assert lib.dh_problem_eval(h, a, 1, ptr(u), ptr(v), ptr(l)) == _lib.ERR_ARG
    assert b"bad problem handle" in lib.dh_last_error(h)
    assert lib.dh_problem_destroy(h, a) == _lib.ERR_ARG
    assert lib.dh_problem_eval(h, -1, 1, ptr(u), ptr(v), ptr(l)) == _lib.ERR_ARG
    assert lib.dh_problem_eval(h, 10**6, 1, ptr(u), ptr(v), ptr(l)) == _lib.ERR_ARG
    c = create(2, 2, one, 1, 0, None, 0)
    assert c == a
    assert lib.dh_problem_destroy(h, b) == 0 and lib.dh_problem_destroy(h, c) == 0
