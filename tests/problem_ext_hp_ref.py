"""High-precision reference and forward error bounds of DH_PRIOR_TABLE and DH_LIKE_GAUSS_MIX (include/dynhip.h), in the
style of tests/hp_ref.py, which serves the ids 0..2 and to which every function here hands those on -- so a problem may
pair a new id with an old one.  Plain Python: no device code, nothing taken from the operation order of the evaluators.

  prior_hp(prob, u)    np.longdouble; exp and ndtri from mpmath at 50 digits
  loglike_hp(prob, v)  np.longdouble sums; max / exp / log of the mixture in mpmath at 50 digits

Bounds (eps = 2^-53; counts of roundings, nothing fitted to an evaluator's output).  Granted and named as such: exp and
log at 3 ulp each -- the OpenCL full-profile limits, as hp_ref grants the cosine 4 ulp -- and the fp64 ndtri at hp_ref's
TAU.  An ulp of x is at most 2 eps |x|, so 3 ulp = 6 eps |x| below.
"""
import mpmath as mp
import numpy as np

import hp_ref as H
from dynesty_amd import problems as PR

LD = H.LD
EPS, TAU, DPS = H.EPS, H.TAU, H.DPS
ULP3 = 6.0 * EPS  # 3 ulp, relative


def _mpf(x):
    """A np.longdouble (or float) as an mpf, exactly: its fp64 head plus the remainder."""
    x = LD(x)
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


def _ld(x):
    return LD(mp.nstr(x, 30))


def _table(prob):
    return np.asarray(prob.prior_par, dtype=np.float64).reshape(prob.ndim, 3)


def _mix(prob):
    n = prob.ndim
    m = int(prob.like_par[0])
    blocks = np.asarray(prob.like_par[1:], dtype=np.float64).reshape(m, 1 + n + n * n)
    return blocks[:, 0], blocks[:, 1:1 + n], blocks[:, 1 + n:].reshape(m, n, n)


# ---------------------------------------------------------------------------------------------------------
# the functions
# ---------------------------------------------------------------------------------------------------------
def prior_hp(prob, u):
    if prob.prior_id != PR.PRIOR_TABLE:
        return H.prior_hp(prob, u)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    out = np.empty(u.shape, dtype=LD)
    for i, (kind, p0, p1) in enumerate(_table(prob)):
        if kind == PR.TABLE_UNIFORM:
            out[:, i] = u[:, i].astype(LD) * LD(p1) + LD(p0)
        elif kind == PR.TABLE_NORMAL:
            out[:, i] = LD(p0) + LD(p1) * H.ndtri_hp(u[:, i])
        else:
            with mp.workdps(DPS):  # the argument exactly (106 bits fit), then exp
                out[:, i] = [_ld(mp.exp(mp.mpf(float(x)) * mp.mpf(float(p1)) + mp.mpf(float(p0)))) for x in u[:, i]]
    return out


def _components_hp(prob, v):
    """(k, M) np.longdouble a_m = c_m - (v - mu_m)^T P_m (v - mu_m) / 2 with the full matrices as given."""
    c, mu, prec = _mix(prob)
    v = np.atleast_2d(np.asarray(v)).astype(LD)
    d = v[:, None, :] - mu.astype(LD)[None, :, :]
    q = np.sum(d[:, :, :, None] * prec.astype(LD)[None, :, :, :] * d[:, :, None, :], axis=(2, 3))
    return c.astype(LD)[None, :] - LD(0.5) * q


def loglike_hp(prob, v):
    if prob.like_id != PR.LIKE_GAUSS_MIX:
        return H.loglike_hp(prob, v)
    a = _components_hp(prob, v)
    if a.shape[1] == 1:
        return a[:, 0].copy()
    out = np.empty(len(a), dtype=LD)
    with mp.workdps(DPS):
        for k, row in enumerate(a):
            am = [_mpf(x) for x in row]
            top = max(am)
            out[k] = _ld(top + mp.log(mp.fsum(mp.exp(x - top) for x in am)))
    return out


# ---------------------------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------------------------
def prior_bound(prob, u):
    """Elementwise bound on |fp64 prior_transform(u) - prior_hp(u)| for the STORED rows [kind, p0, p1].

    uniform      u p1 + p0: one rounding with a fused multiply-add (the device), two without (the host), each at most
                 eps times a magnitude that |u p1| + |p0| bounds: 2 eps (|u p1| + |p0|).
    normal       hp_ref's NORMAL: TAU |p1 z| + 2 eps (|p0| + |p1 z|).
    log-uniform  the argument t = u p1 + p0 as above, delta = 2 eps (|u p1| + |p0|), moves exp by the factor
                 e^delta; exp itself 3 ulp: v (expm1(delta) + 6 eps (1 + expm1(delta)))."""
    if prob.prior_id != PR.PRIOR_TABLE:
        return H.prior_bound(prob, u)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    out = np.empty(u.shape)
    for i, (kind, p0, p1) in enumerate(_table(prob)):
        mag = np.abs(u[:, i] * p1) + abs(p0)
        if kind == PR.TABLE_UNIFORM:
            out[:, i] = 2.0 * EPS * mag
        elif kind == PR.TABLE_NORMAL:
            sz = np.abs(p1 * H.ndtri_hp(u[:, i])).astype(np.float64)
            out[:, i] = TAU * sz + 2.0 * EPS * (abs(p0) + sz)
        else:
            g = np.expm1(2.0 * EPS * mag)
            out[:, i] = np.exp(u[:, i] * p1 + p0) * (1.0 + ULP3) * (g + ULP3 * (1.0 + g))
    return out


def _mix_parts(prob, v):
    """fp64 (k, M): the a_m and Q_m = sum_ij |P_ij||d_i||d_j| of every component."""
    c, mu, prec = _mix(prob)
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    ad = np.abs(v[:, None, :] - mu[None, :, :])
    return _components_hp(prob, v).astype(np.float64), np.einsum('kmi,mij,kmj->km', ad, np.abs(prec), ad), c


def loglike_bound(prob, v):
    """(k, n) -> (k,) bound on |fp64 loglikelihood(v) - loglike_hp(v)| for one and the same fp64 v.

    One component: d = v - mu is rounded once per element, |delta d_i| <= eps |d_i|, and a_m moves by at most
    sum_i |(P d)_i| |delta d_i| <= eps Q, Q = sum_ij |P_ij||d_i||d_j|.  On that d the quadratic form is hp_ref's
    GAUSS_PREC count, (2n + 4) eps (|c| + Q / 2), in any of the orders (full, upper or lower triangle):
        e_m = (2n + 4) eps (|c_m| + Q_m / 2) + eps Q_m.        M = 1: this is the bound.
    M > 1: logl = s + log(S), S = sum_m exp(b_m), b_m = a_m - s, for the evaluator's own shift s = its largest a_m (any
    s gives the same value exactly, so which component it took for the largest carries no error).  Term m has the
    relative error e_m (of a_m) + eps |b_m| (the subtraction) + 6 eps (exp, 3 ulp); a sum of M positive terms adds
    (M - 1) eps; d log(S) = dS / S, so the terms weigh in with w_m = exp(b_m) / S (they sum to 1); log itself 3 ulp of
    |log S| <= log M; the final addition one rounding of |logl|; two spare for the second order:
        sum_m w_m (e_m + eps |b_m| + 6 eps) + (M - 1) eps + 6 eps log(S) + eps |logl| + 2 eps.
    (A term that underflows is below 1e-323 of S >= 1 absolutely: nothing to add.)"""
    if prob.like_id != PR.LIKE_GAUSS_MIX:
        return H.loglike_bound(prob, v)
    n = prob.ndim
    a, q, c = _mix_parts(prob, v)
    e = (2 * n + 4) * EPS * (np.abs(c)[None, :] + 0.5 * q) + EPS * q
    m = a.shape[1]
    if m == 1:
        return e[:, 0]
    b = a - a.max(axis=1, keepdims=True)
    t = np.exp(b)
    s = t.sum(axis=1)
    w = t / s[:, None]
    logl = a.max(axis=1) + np.log(s)
    return np.sum(w * (e + EPS * np.abs(b) + ULP3), axis=1) + (m - 1) * EPS + ULP3 * np.log(s) + EPS * np.abs(logl) + 2 * EPS


def loglike_grad_abs(prob, v):
    """(k, n) -> (k, n): |d logl / d v_i| <= sum_m w_m |(P_m d_m)_i| (first order, as hp_ref's)."""
    if prob.like_id != PR.LIKE_GAUSS_MIX:
        return H.loglike_grad_abs(prob, v)
    c, mu, prec = _mix(prob)
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    a = _components_hp(prob, v).astype(np.float64)
    w = np.exp(a - a.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    d = v[:, None, :] - mu[None, :, :]
    sym = 0.5 * (prec + np.transpose(prec, (0, 2, 1)))
    return np.einsum('km,kmi->ki', w, np.abs(np.einsum('mij,kmj->kmi', sym, d)))


# ---------------------------------------------------------------------------------------------------------
# checks (hp_ref.check / check_from_u with the functions above)
# ---------------------------------------------------------------------------------------------------------
def check(prob, u, v, logl, rows=None, what=""):
    u, v, logl = np.atleast_2d(np.asarray(u)), np.atleast_2d(np.asarray(v)), np.atleast_1d(np.asarray(logl))
    if rows is not None:
        u, v, logl = u[rows], v[rows], logl[rows]
    ev = np.abs(v.astype(LD) - prior_hp(prob, u)).astype(np.float64)
    bv = prior_bound(prob, u)
    el = np.abs(logl.astype(LD) - loglike_hp(prob, v)).astype(np.float64)
    bl = loglike_bound(prob, v)
    rv, rl = H.worst_ratio(ev, bv), H.worst_ratio(el, bl)
    print(f"ext_hp_ref {what or prob.name}: v err/bound {rv:.3f}  logl err/bound {rl:.3f}")
    bad = np.argwhere(~(ev <= bv))  # "not <=": a NaN must fail
    assert bad.size == 0, (f"{what}: v outside its bound at {bad[:5].tolist()}: u={u[tuple(bad[0])]!r} "
                           f"v={v[tuple(bad[0])]!r} err={ev[tuple(bad[0])]:.3e} bound={bv[tuple(bad[0])]:.3e}")
    bad = np.flatnonzero(~(el <= bl))
    assert bad.size == 0, (f"{what}: logl outside its bound at {bad[:5].tolist()}: logl={logl[bad[0]]!r} "
                           f"err={el[bad[0]]:.3e} bound={bl[bad[0]]:.3e}")
    return rv, rl


def logl_bound_from_u(prob, u):
    """Bound on |fp64 logl(prior(u)) - loglike_hp(prior_hp(u))|: the likelihood's at the exact v plus the prior's
    carried through |d logl / d v_i|."""
    v64 = prior_hp(prob, u).astype(np.float64)
    return loglike_bound(prob, v64) + np.sum(loglike_grad_abs(prob, v64) * prior_bound(prob, u), axis=1)


def check_from_u(prob, u, logl, what=""):
    u, logl = np.atleast_2d(np.asarray(u, dtype=np.float64)), np.atleast_1d(np.asarray(logl))
    bound = logl_bound_from_u(prob, u)
    err = np.abs(logl.astype(LD) - loglike_hp(prob, prior_hp(prob, u))).astype(np.float64)
    r = H.worst_ratio(err, bound)
    print(f"ext_hp_ref {what or prob.name}: logl(u) err/bound {r:.3f}")
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (f"{what}: logl outside its bound at {bad[:5].tolist()}: logl={logl[bad[0]]!r} "
                           f"err={err[bad[0]]:.3e} bound={bound[bad[0]]:.3e}")
    return r


# ---------------------------------------------------------------------------------------------------------
# the cases the tests share
# ---------------------------------------------------------------------------------------------------------
def mixed_rows(ndim, offset=0):
    """Adjacent coordinates of different kinds (uniform, normal, log-uniform over twelve decades, ...)."""
    rows = []
    for i in range(ndim):
        k = (i + offset) % 3
        rows.append(("uniform", -3.0 - 0.5 * i, 4.0 + 0.25 * i) if k == 0 else
                    ("normal", 0.3 - 0.1 * i, 1.7 + 0.05 * i) if k == 1 else ("loguniform", 1e-6, 1e6))
    return rows


def uniform_rows(ndim, lo=-60.0, hi=60.0):
    return [("uniform", lo - 0.5 * (i % 3), hi + 0.25 * (i % 5)) for i in range(ndim)]


def spd(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n))
    return scale * (m @ m.T / n + np.eye(n))


MIX_CASES = ("random", "separated", "identical", "tiny_weight", "far_means")


def mixture_parts(case, ndim, m, seed):
    """(means, covs, weights) of the named mixture case."""
    rng = np.random.default_rng(seed)
    covs = np.stack([spd(ndim, seed + 10 * k) for k in range(m)])
    w = rng.uniform(0.5, 1.5, m)
    if case == "random":
        means = rng.uniform(-2.0, 2.0, (m, ndim))
    elif case == "separated":  # 40 standard deviations apart: every exp but one underflows
        means = np.zeros((m, ndim))
        means[:, 0] = 60.0 * np.arange(m) / max(m - 1, 1) - 30.0 if m > 1 else 0.0
        covs = np.stack([np.eye(ndim) * 0.01] * m)
    elif case == "identical":  # the first two components the same: ln 2 is added
        means = rng.uniform(-2.0, 2.0, (m, ndim))
        if m > 1:
            means[1], covs[1], w[1] = means[0], covs[0], w[0]
    elif case == "tiny_weight":
        means = rng.uniform(-2.0, 2.0, (m, ndim))
        w[m - 1] = 1e-12 * w.sum()
    elif case == "far_means":  # |mu| up to 50, unit width: the cancellation in v - mu
        means = rng.uniform(-50.0, 50.0, (m, ndim))
        means[0] = 50.0 * np.where(np.arange(ndim) % 2, -1.0, 1.0)
        covs = np.stack([np.eye(ndim)] * m)
    else:
        raise ValueError(case)
    return means, covs, w


def mixture_problem(case, ndim, m, seed, prior="uniform"):
    means, covs, w = mixture_parts(case, ndim, m, seed)
    rows = uniform_rows(ndim) if prior == "uniform" else mixed_rows(ndim)
    return PR.gauss_mixture(means, covs, w, prior=rows, name=f"mix{m}:{case}+{prior}/{ndim}")


def near_component_u(prob, k, seed, spread=1.0):
    """k unit-cube points whose v (uniform table) lie around the component means, a standard deviation or so off."""
    rng = np.random.default_rng(seed)
    c, mu, prec = _mix(prob)
    tab = _table(prob)
    assert np.all(tab[:, 0] == PR.TABLE_UNIFORM)
    which = rng.integers(len(mu), size=k)
    sd = np.array([np.sqrt(np.diag(np.linalg.inv(p))) for p in prec])
    v = mu[which] + spread * sd[which] * rng.standard_normal((k, prob.ndim))
    return np.clip((v - tab[:, 1]) / tab[:, 2], 1e-6, 1 - 1e-6)


K = 130  # the walkers of a GPU case: two full wavefronts + two live lanes


def mixed_problem(ndim, m=2):
    """A mixture under the mixed table whose components sit at the prior's u = 0.45 / 0.55 (/ between)."""
    tab = PR.prior_table(mixed_rows(ndim))
    probe = PR.Problem(ndim, PR.LIKE_GAUSS_IID, [0.0], PR.PRIOR_TABLE, tab.ravel())
    lo, hi = (probe.prior_transform(np.full(ndim, x)) for x in (0.45, 0.55))
    means = np.array([lo + (hi - lo) * t for t in np.linspace(0.0, 1.0, m)])
    return PR.gauss_mixture(means, np.diag((hi - lo)**2), None, prior=tab, name=f"mix{m}+mixed/{ndim}")


def sampler_case(prob, seed):
    """The start points, threshold and frame of the GPU tests' sampler cases (K = 130 walkers): K starts above the 5 % quantile of the starts' exact log-likelihoods, a random frame with steps a fraction of the
    start cloud's width (test_gpu_evaluators.sampler_case)."""
    d = prob.ndim
    rng = np.random.default_rng(seed)
    n0 = K + 24
    if np.all(_table(prob)[:, 0] == PR.TABLE_UNIFORM):
        u0 = near_component_u(prob, n0, seed)
        spread = float(np.median(np.std(u0, axis=0)))
        spread = min(spread, 1.0 / 120.0)
    else:
        spread = 0.05
        u0 = np.clip(0.5 + spread * rng.standard_normal((n0, d)), 1e-3, 1 - 1e-3)
    v0 = prior_hp(prob, u0)
    l0 = loglike_hp(prob, v0)
    loglstar = float(np.quantile(l0.astype(np.float64), 0.05))
    keep = np.flatnonzero(l0 > LD(loglstar))[:K]
    assert len(keep) == K
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    axes = q * (0.3 * spread * rng.uniform(0.8, 1.6, size=d))
    return dict(u0=np.ascontiguousarray(u0[keep]), logl0=l0[keep], loglstar=loglstar, axes=axes, scale=0.7,
                spread=spread)
