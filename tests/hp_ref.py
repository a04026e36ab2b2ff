"""High-precision reference of the device problems (include/dynhip.h: DH_LIKE_* / DH_PRIOR_*) and forward
error bounds for an fp64 evaluation of them.  Plain Python: no device code, nothing taken from the operation
order of csrc/problem.h.

  prior_hp(prob, u)    v = prior_transform(u)   sums / products in np.longdouble, ndtri from mpmath
  loglike_hp(prob, v)  loglikelihood(v)         np.longdouble; GAUSS_PREC with the FULL matrix P as given
  ndtri_hp(u)          the root of ncdf(z) = p by Newton's iteration at 50 digits (mpmath)

Bounds (eps = 2^-53, per element; derived, not measured -- the derivations stand next to each function):
  prior_bound(prob, u)       |v_fp64 - prior_hp(u)|
  loglike_bound(prob, v)     |logl_fp64(v) - loglike_hp(v)| for the SAME v (the evaluator's own returned v), so that
                             prior and likelihood errors do not compound
  loglike_grad_abs(prob, v)  |d logl / d v_i|, to carry a prior error through where only u is known
"""
import math

import mpmath as mp
import numpy as np
from scipy.special import ndtri as _scipy_ndtri

from dynesty_amd import problems as PR

LD = np.longdouble
# the extended type must carry at least 60 bits, or the sums below would have to move to mpmath
assert np.finfo(LD).eps <= 2.0**-60, "np.longdouble is not an extended type here: do the arithmetic in mpmath"

EPS = 2.0**-53
DPS = 50  # digits of the Newton iteration
NEWTON_STEPS = 3  # quadratic from SciPy's 1e-16: 1e-31 after one step; the round-trip test holds the result to 1e-30

# Relative accuracy granted to an fp64 ndtri:  tau = 2 * (1.1e-15 + S_SCIPY).
#   1.1e-15  the larger of the two figures csrc/problem.h states for the device's inverses against SciPy
#   S_SCIPY  SciPy's own worst relative error against ndtri_hp on sweep(): measured by
#            tests/test_hp_ref_cpu.py::test_ndtri_hp_roundtrip_and_scipy_error (and asserted <= 1e-15 there)
#   2        the project's figures come from sampled sweeps, not from proofs
S_SCIPY = 4.5e-16  # 4.498e-16 measured (SciPy 1.15.3, the 811 probabilities of sweep()): tau = 3.1e-15
TAU = 2.0 * (1.1e-15 + S_SCIPY)

_cache = {}


def _ndtri_mp(p):
    """ndtri of one fp64 p in (0, 1) as an mpf (call inside mp.workdps(DPS))."""
    pm = mp.mpf(p)
    if pm == mp.mpf(0.5):
        return mp.mpf(0)
    if pm > 0.5:
        # 1 - p is exact at this precision: solve in the lower tail, where ncdf keeps its relative accuracy
        lo, sign = mp.mpf(1) - pm, -1
    else:
        lo, sign = pm, 1
    z = mp.mpf(float(_scipy_ndtri(float(lo))))
    for _ in range(NEWTON_STEPS):
        z = z - (mp.ncdf(z) - lo) / mp.npdf(z)
    return sign * z


def ndtri_hp(u):
    """Inverse normal CDF of fp64 values in (0, 1), elementwise, as np.longdouble."""
    u = np.asarray(u, dtype=np.float64)
    out = np.empty(u.shape, dtype=LD)
    with mp.workdps(DPS):
        for idx, p in np.ndenumerate(u):
            p = float(p)
            z = _cache.get(p)
            if z is None:
                if not 0.0 < p < 1.0:
                    raise ValueError(f"ndtri_hp: p={p!r} is outside (0, 1)")
                z = LD(mp.nstr(_ndtri_mp(p), 30))
                _cache[p] = z
            out[idx] = z
    return out


def ndtri_mp(p):
    """The mpf itself (for the round-trip check), at DPS digits; call inside mp.workdps(DPS)."""
    return _ndtri_mp(float(p))


def sweep(seed=20240607):
    """The probabilities every ndtri check runs over: the bulk, both tails down to the smallest normal numbers, the
    cancellation zone around 1/2, and the switch points of the device's two inverses (AS 241 central / tail at
    |p - 1/2| = 0.425, hand-over to erfcinv below exp(-25))."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(0.0, 1.0, 300),
             10.0**rng.uniform(-300.0, -1.0, 200),
             1.0 - 10.0**(-rng.uniform(1.0, 15.9, 200)),
             0.5 + rng.uniform(-1e-8, 1e-8, 100)]
    edges = []
    for x in (0.075, 0.925, math.exp(-25.0)):
        edges += [np.nextafter(x, 0.0), x, np.nextafter(x, 1.0)]
    edges += [np.nextafter(1.0, 0.0), 2.3e-308]
    p = np.concatenate(parts + [np.array(edges)])
    assert np.all((p > 0.0) & (p < 1.0))
    return p


# ---------------------------------------------------------------------------------------------------------
# the functions
# ---------------------------------------------------------------------------------------------------------
def prior_hp(prob, u):
    u = np.asarray(u, dtype=np.float64)
    if prob.prior_id == PR.PRIOR_IDENTITY:
        return u.astype(LD)
    if prob.prior_id == PR.PRIOR_AFFINE:
        a, b = (LD(x) for x in prob.prior_par)
        return a * (LD(2) * u.astype(LD) - LD(1)) + b
    if prob.prior_id == PR.PRIOR_NORMAL:
        mu, sg = (LD(x) for x in prob.prior_par)
        return mu + sg * ndtri_hp(u)
    raise ValueError("unknown prior id")


def _prec(prob):
    n = prob.ndim
    return np.asarray(prob.like_par[1:1 + n * n], dtype=np.float64).reshape(n, n)


def loglike_hp(prob, v):
    """(k, n) -> (k,) np.longdouble.  v may be fp64 (a device's returned v) or longdouble (prior_hp's)."""
    v = np.atleast_2d(np.asarray(v)).astype(LD)
    if prob.like_id == PR.LIKE_GAUSS_IID:
        return LD(prob.like_par[0]) - LD(0.5) * np.sum(v * v, axis=1)
    if prob.like_id == PR.LIKE_GAUSS_PREC:
        P = _prec(prob).astype(LD)  # all of it: v^T P v = sum_ij P_ij v_i v_j
        q = np.sum(v[:, :, None] * P[None, :, :] * v[:, None, :], axis=(1, 2))
        return LD(prob.like_par[0]) - LD(0.5) * q
    if prob.like_id == PR.LIKE_EGGBOX:
        tmax = LD(prob.like_par[0])
        t = (LD(2) * tmax * v - tmax) / LD(2)
        b = LD(2) + np.prod(np.cos(t), axis=1)
        return b * b * b * b * b
    raise ValueError("unknown likelihood id")


# ---------------------------------------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------------------------------------
def prior_bound(prob, u):
    """Elementwise bound on |fp64 prior_transform(u) - prior_hp(u)|.

    IDENTITY  0: the value is copied.
    AFFINE    a (2u - 1) + b: 2u exact, one rounding each for the subtraction, the product and the sum (or two with
              a fused multiply-add); each is at most eps times a magnitude that |a||2u - 1| + |b| bounds:
              3 eps (|a||2u - 1| + |b|).
    NORMAL    mu + sigma z, z an fp64 ndtri of relative accuracy TAU: TAU |sigma z*| for z, one rounding for
              the product and one for the sum, each at most eps (|mu| + |sigma z*|) (1 + O(TAU))."""
    u = np.asarray(u, dtype=np.float64)
    if prob.prior_id == PR.PRIOR_IDENTITY:
        return np.zeros(u.shape)
    if prob.prior_id == PR.PRIOR_AFFINE:
        a, b = prob.prior_par
        return 3.0 * EPS * (abs(a) * np.abs(2.0 * u - 1.0) + abs(b))
    if prob.prior_id == PR.PRIOR_NORMAL:
        mu, sg = prob.prior_par
        sz = np.abs(sg * ndtri_hp(u)).astype(np.float64)
        return TAU * sz + 2.0 * EPS * (abs(mu) + sz)
    raise ValueError("unknown prior id")


def loglike_bound(prob, v):
    """(k, n) -> (k,) bound on |fp64 loglikelihood(v) - loglike_hp(v)| for one and the same fp64 v.

    GAUSS_IID   n products and n - 1 additions in any order (a sum of n non-negative terms: relative error
                (n - 1) eps, plus one for the products), the factor 1/2 exact, one rounding for "+ c", one spare:
                (n + 3) eps (|c| + sum v^2 / 2).
    GAUSS_PREC  a mat-vec row is a sum of n terms (n eps of sum_j |P_ij||v_j|), the outer product with v_i and the
                outer sum another n + 1, halving the diagonal or the whole is exact, "+ c" one, two spare:
                (2n + 4) eps (|c| + sum_ij |P_ij||v_i||v_j| / 2).  Holds for the full, the upper- and the
                lower-triangular order alike once P is symmetric (they sum the same magnitudes).
    EGGBOX      argument t_i = (2 tmax v_i - tmax) / 2: two roundings of magnitudes <= 2 tmax |v_i| + tmax, carried
                through |d cos| <= 1: 3 eps tmax (|v_i| + 1/2); the cosine itself 4 ulp of a value <= 1 (the OpenCL
                full-profile limit that ocml is built to): e_i = 3 eps tmax (|v_i| + 1/2) + 4 eps.
                Product of n factors of modulus <= 1: |d prod| <= sum e_i + n eps.
                b = 2 + prod, logl = b^5 by four multiplications: |d logl| <= 5 b^4 |d prod| + 4 eps b^5 with
                b = 2 + |prod| (the rounding of b itself is inside the 4)."""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    n = prob.ndim
    if prob.like_id == PR.LIKE_GAUSS_IID:
        return (n + 3) * EPS * (abs(prob.like_par[0]) + 0.5 * np.sum(v * v, axis=1))
    if prob.like_id == PR.LIKE_GAUSS_PREC:
        av = np.abs(v)
        q = np.einsum('ki,ij,kj->k', av, np.abs(_prec(prob)), av)
        return (2 * n + 4) * EPS * (abs(prob.like_par[0]) + 0.5 * q)
    if prob.like_id == PR.LIKE_EGGBOX:
        tmax = float(prob.like_par[0])
        e = 3.0 * EPS * tmax * (np.abs(v) + 0.5) + 4.0 * EPS
        dprod = np.sum(e, axis=1) + n * EPS
        prod = np.prod(np.cos((2.0 * tmax * v - tmax) / 2.0), axis=1)
        b = 2.0 + np.abs(prod)
        return 5.0 * b**4 * dprod + 4.0 * EPS * b**5
    raise ValueError("unknown likelihood id")


def loglike_grad_abs(prob, v):
    """(k, n) -> (k, n): |d logl / d v_i| at v, to first order (the second-order term is the square of a prior
    bound, ~1e-30, times a curvature of order |P| or tmax^2 b^4: below 1e-24 for every problem of the suite)."""
    v = np.atleast_2d(np.asarray(v, dtype=np.float64))
    if prob.like_id == PR.LIKE_GAUSS_IID:
        return np.abs(v)
    if prob.like_id == PR.LIKE_GAUSS_PREC:
        P = _prec(prob)
        return np.abs(v @ (0.5 * (P + P.T)))
    if prob.like_id == PR.LIKE_EGGBOX:
        tmax = float(prob.like_par[0])
        t = (2.0 * tmax * v - tmax) / 2.0
        c, s = np.cos(t), np.sin(t)
        b = 2.0 + np.prod(c, axis=1)
        others = np.empty_like(v)
        for i in range(v.shape[1]):
            others[:, i] = np.prod(np.delete(np.abs(c), i, axis=1), axis=1)
        return 5.0 * (b**4)[:, None] * tmax * np.abs(s) * others
    raise ValueError("unknown likelihood id")


# ---------------------------------------------------------------------------------------------------------
# the nine pairs, with the parameters the tests use throughout
# ---------------------------------------------------------------------------------------------------------
AFFINE_PAR = [4.0, 0.5]
NORMAL_PAR = [0.3, 1.7]
TMAX = 5.0 * math.pi
LIKES = ("iid", "prec", "eggbox")
PRIORS = ("identity", "affine", "normal")
PAIRS = [(lk, pr) for lk in LIKES for pr in PRIORS]


def spd_plus_antisym(n, seed, asym=0.1):
    """P = S + asym * A: S symmetric positive definite with unit-order entries, A antisymmetric."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n))
    s = m @ m.T / n + np.eye(n)
    a = rng.standard_normal((n, n))
    return s + asym * (a - a.T)


def make_problem(like, prior, ndim, seed=5, asym=0.0):
    """problems.Problem(...) for one (likelihood, prior) pair; c as dynesty_amd/problems.py sets it."""
    c = -0.5 * ndim * math.log(2.0 * math.pi)
    if like == "iid":
        lid, lpar = PR.LIKE_GAUSS_IID, [c]
    elif like == "prec":
        P = spd_plus_antisym(ndim, seed, asym)
        _, logdet = np.linalg.slogdet(0.5 * (P + P.T))
        lid, lpar = PR.LIKE_GAUSS_PREC, np.concatenate([[c + 0.5 * logdet], P.ravel()])
    else:
        lid, lpar = PR.LIKE_EGGBOX, [TMAX]
    pid, ppar = {"identity": (PR.PRIOR_IDENTITY, []), "affine": (PR.PRIOR_AFFINE, AFFINE_PAR),
                 "normal": (PR.PRIOR_NORMAL, NORMAL_PAR)}[prior]
    return PR.Problem(ndim, lid, lpar, pid, ppar, name=f"{like}+{prior}/{ndim}")


def sweep_matrix(k, ndim, seed):
    """(k, ndim) probabilities drawn from sweep() by an independent permutation per coordinate, so that every
    coordinate index meets the tails, the centre and the switch points."""
    rng = np.random.default_rng(seed)
    p = sweep()
    cols = [p[rng.permutation(len(p))[np.arange(k) % len(p)]] for _ in range(ndim)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def worst_ratio(err, bound):
    """max err / bound; 0 / 0 counts as 0, x / 0 as inf, and a NaN error as inf (np.max alone would carry the NaN on,
    and Python's max() would drop it)."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    pos = bound > 0
    with np.errstate(invalid="ignore"):  # inf / inf of an evaluator's inf: the NaN is turned into inf below
        r = np.where(pos, err / np.where(pos, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


def check(prob, u, v, logl, rows=None, what=""):
    """Assert one evaluator's (v, logl) at u against the reference, within the bounds; returns the worst
    error / bound ratios (v, logl).  rows: the walkers to check (None = all)."""
    u, v, logl = np.asarray(u), np.asarray(v), np.asarray(logl)
    if rows is not None:
        u, v, logl = u[rows], v[rows], logl[rows]
    ev = np.abs(v.astype(LD) - prior_hp(prob, u)).astype(np.float64)
    bv = prior_bound(prob, u)
    el = np.abs(logl.astype(LD) - loglike_hp(prob, v)).astype(np.float64)
    bl = loglike_bound(prob, v)
    rv, rl = worst_ratio(ev, bv), worst_ratio(el, bl)
    print(f"hp_ref {what or prob.name}: v err/bound {rv:.3f}  logl err/bound {rl:.3f}")
    # "not (err <= bound)", never "err > bound": a NaN from the evaluator compares False both ways and must fail
    bad = np.argwhere(~(ev <= bv))
    assert bad.size == 0, (f"{what}: v outside its bound at {bad[:5].tolist()}: u={u[tuple(bad[0])]!r} "
                           f"v={v[tuple(bad[0])]!r} err={ev[tuple(bad[0])]:.3e} bound={bv[tuple(bad[0])]:.3e}")
    bad = np.flatnonzero(~(el <= bl))
    assert bad.size == 0, (f"{what}: logl outside its bound at {bad[:5].tolist()}: logl={logl[bad[0]]!r} "
                           f"err={el[bad[0]]:.3e} bound={bl[bad[0]]:.3e}")
    return rv, rl


def check_from_u(prob, u, logl, what=""):
    """Assert stored log-likelihoods against the reference where only the unit-cube points are known: the bound is the
    likelihood's at the exact v plus the prior's carried through |d logl / d v_i|.  Returns the worst error / bound."""
    u, logl = np.atleast_2d(np.asarray(u, dtype=np.float64)), np.asarray(logl)
    vh = prior_hp(prob, u)
    v64 = vh.astype(np.float64)
    bound = loglike_bound(prob, v64) + np.sum(loglike_grad_abs(prob, v64) * prior_bound(prob, u), axis=1)
    err = np.abs(logl.astype(LD) - loglike_hp(prob, vh)).astype(np.float64)
    r = worst_ratio(err, bound)
    print(f"hp_ref {what or prob.name}: logl(u) err/bound {r:.3f}")
    bad = np.flatnonzero(~(err <= bound))  # a NaN fails: see check()
    assert bad.size == 0, (f"{what}: logl outside its bound at {bad[:5].tolist()}: logl={logl[bad[0]]!r} "
                           f"err={err[bad[0]]:.3e} bound={bound[bad[0]]:.3e}")
    return r
