"""Synthetic likelihood / prior-transform pairs of the BASELINE configs.

dynesty calls the user's ``prior_transform(u)`` and ``loglikelihood(v)`` once
per proposal, *inside* the proposal loop
(/root/reference/py/dynesty/internal_samplers.py:328-329, 957-958, 1116-1117).
For the device path those two callbacks have to live on the GPU, so the
BASELINE problems are described twice, by the same object:

* ``problem.loglikelihood`` / ``problem.prior_transform`` -- plain NumPy
  callables.  These play the role of the *user's* functions: they are what is
  handed to ``dynesty.NestedSampler`` (initial live points, generic lock-step
  path) and what the test oracle evaluates.
* ``problem.device_spec()`` -- ``(like_id, like_par, prior_id, prior_par)``,
  the description uploaded through ``dh_problem_create`` (include/dynhip.h) and
  evaluated in-kernel by ``dynesty_amd/csrc/problem.h``.

Both sides use the same operation order so that they agree to rounding.

Problem definitions:
  C1  3-D unit Gaussian, prior +-10      demos "Demo 2", tests/test_gau.py
  C2  25-D rho=0.4 correlated Normal     demos/Examples -- 25-D Correlated Normal.ipynb cell 7
  C3  2-D eggbox                         demos/Examples -- Eggbox.ipynb cell 7
  C4  200-D iid Normal, normal prior     demos/Examples -- 200-D Multivariate Normal.ipynb cell 8
"""
import math

import numpy as np
from scipy.special import ndtri

# ids shared with include/dynhip.h
LIKE_GAUSS_IID = 0  # logl = -0.5 * sum(v^2) + c                par = [c]
LIKE_GAUSS_PREC = 1  # logl = -0.5 * v^T P v + c                 par = [c, P row-major]
#   (P may be asymmetric: the host forms the full v^T P v, the device stores (P + P^T) / 2 -- the same
#   quadratic form -- because its evaluators read different triangles of the matrix)
LIKE_EGGBOX = 2  # logl = (2 + prod cos((2 tmax v - tmax)/2))^5  par = [tmax]

PRIOR_IDENTITY = 0  # v = u
PRIOR_AFFINE = 1  # v = a * (2 u - 1) + b                        par = [a, b]
PRIOR_NORMAL = 2  # v = mu + sigma * ndtri(u)                    par = [mu, sigma]

# Problems of the user's own shape (created through dh_problem_create_ex):
LIKE_GAUSS_MIX = 3  # logl = a* + log(sum_m exp(a_m - a*)), a* = max a_m, a_m = c_m - 0.5 (v - mu_m)^T P_m (v - mu_m)
#   par = [M, then per component c_m, mu_m (n), P_m (n x n row-major)], 1 <= M <= MIX_MAX; M = 1 is a_0 itself
PRIOR_TABLE = 3  # one row [kind, p0, p1] per coordinate                 par = n rows
MIX_MAX = 8
TABLE_UNIFORM = 0  # v = u * p1 + p0            p0 = lo, p1 = hi - lo   (one fused multiply-add on the device)
TABLE_NORMAL = 1  # v = p0 + p1 * ndtri(u)      p0 = mu, p1 = sigma
TABLE_LOGUNIFORM = 2  # v = exp(u * p1 + p0)    p0 = ln lo, p1 = ln(hi / lo)
_TABLE_KINDS = {"uniform": TABLE_UNIFORM, "normal": TABLE_NORMAL, "loguniform": TABLE_LOGUNIFORM}


def check_spec(ndim, like_id, like_par, prior_id, prior_par):
    """ValueError for what dh_problem_create_ex refuses in a LIKE_GAUSS_MIX / PRIOR_TABLE description."""
    n = int(ndim)
    lp, pp = np.asarray(like_par, dtype=np.float64).ravel(), np.asarray(prior_par, dtype=np.float64).ravel()
    if n < 1:
        raise ValueError(f"ndim={ndim}")
    if like_id not in (LIKE_GAUSS_IID, LIKE_GAUSS_PREC, LIKE_EGGBOX, LIKE_GAUSS_MIX):
        raise ValueError(f"unknown likelihood id {like_id}")
    if prior_id not in (PRIOR_IDENTITY, PRIOR_AFFINE, PRIOR_NORMAL, PRIOR_TABLE):
        raise ValueError(f"unknown prior id {prior_id}")
    if not np.all(np.isfinite(lp)) or not np.all(np.isfinite(pp)):
        raise ValueError("a parameter is not finite")
    if like_id == LIKE_GAUSS_MIX:
        if lp.size < 1 or not (1 <= lp[0] <= MIX_MAX) or lp[0] != int(lp[0]):
            raise ValueError(f"a Gaussian mixture has 1..{MIX_MAX} components")
        m = int(lp[0])
        if lp.size != 1 + m * (1 + n + n * n):
            raise ValueError(f"a mixture of {m} components in {n} dimensions has {1 + m * (1 + n + n * n)} "
                             f"parameters, got {lp.size}")
        blocks = lp[1:].reshape(m, 1 + n + n * n)
        for k in range(m):
            if not np.all(np.diag(blocks[k, 1 + n:].reshape(n, n)) > 0.0):
                raise ValueError(f"component {k}: a diagonal entry of the precision matrix is not positive")
    elif lp.size < (1 + n * n if like_id == LIKE_GAUSS_PREC else 1):
        raise ValueError(f"likelihood id {like_id}: {lp.size} parameters")
    if prior_id == PRIOR_TABLE:
        if pp.size != 3 * n:
            raise ValueError(f"a prior table of {n} coordinates has {3 * n} parameters, got {pp.size}")
        rows = pp.reshape(n, 3)
        if not np.all(np.isin(rows[:, 0], (TABLE_UNIFORM, TABLE_NORMAL, TABLE_LOGUNIFORM))):
            raise ValueError("prior table: kind outside 0..2")
        if np.any((rows[:, 0] != TABLE_LOGUNIFORM) & ~(rows[:, 2] > 0.0)):
            raise ValueError("prior table: the width of a uniform row / the sigma of a normal row is not positive")
    elif pp.size < (0 if prior_id == PRIOR_IDENTITY else 2):
        raise ValueError(f"prior id {prior_id}: {pp.size} parameters")


class Problem:
    """A (loglikelihood, prior_transform) pair known to host *and* device."""

    def __init__(self, ndim, like_id, like_par, prior_id, prior_par,
                 logz_truth=None, name=""):
        self.ndim = int(ndim)
        self.like_id = int(like_id)
        self.like_par = np.ascontiguousarray(like_par, dtype=np.float64)
        self.prior_id = int(prior_id)
        self.prior_par = np.ascontiguousarray(prior_par, dtype=np.float64)
        self.logz_truth = logz_truth
        self.name = name
        if like_id == LIKE_GAUSS_MIX or prior_id == PRIOR_TABLE:
            check_spec(ndim, like_id, self.like_par, prior_id, self.prior_par)
        if like_id == LIKE_GAUSS_PREC:
            self._prec = self.like_par[1:].reshape(ndim, ndim)
        if like_id == LIKE_GAUSS_MIX:
            blocks = self.like_par[1:].reshape(int(self.like_par[0]), 1 + ndim + ndim * ndim)
            self._mix_c = blocks[:, 0]
            self._mix_mu = blocks[:, 1:1 + ndim]
            self._mix_prec = blocks[:, 1 + ndim:].reshape(-1, ndim, ndim)
        if prior_id == PRIOR_TABLE:
            rows = self.prior_par.reshape(ndim, 3)
            self._tab = tuple((np.flatnonzero(rows[:, 0] == kind), rows[rows[:, 0] == kind, 1],
                               rows[rows[:, 0] == kind, 2])
                              for kind in (TABLE_UNIFORM, TABLE_NORMAL, TABLE_LOGUNIFORM))

    # -- host callables (the "user functions") ------------------------------
    def prior_transform(self, u):
        u = np.asarray(u, dtype=np.float64)
        if self.prior_id == PRIOR_IDENTITY:
            return u.copy()
        if self.prior_id == PRIOR_AFFINE:
            a, b = self.prior_par
            return a * (2.0 * u - 1.0) + b
        if self.prior_id == PRIOR_NORMAL:
            mu, sigma = self.prior_par
            return mu + sigma * ndtri(u)
        if self.prior_id == PRIOR_TABLE:
            v = np.empty_like(u)
            (iu, au, bu), (inn, an, bn), (il, al, bl) = self._tab
            v[..., iu] = u[..., iu] * bu + au
            v[..., inn] = an + bn * ndtri(u[..., inn])
            v[..., il] = np.exp(u[..., il] * bl + al)
            return v
        raise ValueError("unknown prior id")

    def loglikelihood(self, v):
        v = np.asarray(v, dtype=np.float64)
        if self.like_id == LIKE_GAUSS_IID:
            return float(-0.5 * np.dot(v, v) + self.like_par[0])
        if self.like_id == LIKE_GAUSS_PREC:
            return float(-0.5 * np.dot(v, self._prec @ v) + self.like_par[0])
        if self.like_id == LIKE_EGGBOX:
            tmax = self.like_par[0]
            t = 2.0 * tmax * v - tmax
            return float((2.0 + np.prod(np.cos(t / 2.0)))**5.0)
        if self.like_id == LIKE_GAUSS_MIX:
            a = []
            for c, mu, prec in zip(self._mix_c, self._mix_mu, self._mix_prec):
                d = v - mu
                a.append(c - 0.5 * np.dot(d, prec @ d))
            if len(a) == 1:
                return float(a[0])
            amax = max(a)
            s = 0.0
            for am in a:
                s += math.exp(am - amax)
            return float(amax + math.log(s))
        raise ValueError("unknown likelihood id")

    # vectorised versions, (k, ndim) -> (k, ndim) / (k,)
    def prior_transform_many(self, u):
        return self.prior_transform(u)

    def loglikelihood_many(self, v):
        v = np.asarray(v, dtype=np.float64)
        if self.like_id == LIKE_GAUSS_IID:
            return -0.5 * np.einsum('ij,ij->i', v, v) + self.like_par[0]
        if self.like_id == LIKE_GAUSS_PREC:
            return -0.5 * np.einsum('ij,jk,ik->i', v, self._prec,
                                    v) + self.like_par[0]
        if self.like_id == LIKE_EGGBOX:
            tmax = self.like_par[0]
            t = 2.0 * tmax * v - tmax
            return (2.0 + np.prod(np.cos(t / 2.0), axis=1))**5.0
        if self.like_id == LIKE_GAUSS_MIX:
            d = v[:, None, :] - self._mix_mu[None, :, :]
            a = self._mix_c[None, :] - 0.5 * np.einsum('kmi,mij,kmj->km', d, self._mix_prec, d)
            if a.shape[1] == 1:
                return a[:, 0].copy()
            amax = a.max(axis=1)
            s = np.zeros(len(a))
            for m in range(a.shape[1]):
                s += np.exp(a[:, m] - amax)
            return amax + np.log(s)
        raise ValueError("unknown likelihood id")

    def device_spec(self):
        return (self.like_id, self.like_par, self.prior_id, self.prior_par)

    def __repr__(self):
        return f"Problem({self.name!r}, ndim={self.ndim})"


def gauss_iid(ndim, prior_halfwidth=10.0, name=None):
    """C1 family: N(0, I) likelihood, uniform prior on [-w, w]^ndim."""
    c = -0.5 * ndim * math.log(2.0 * math.pi)
    truth = -ndim * math.log(2.0 * prior_halfwidth)
    return Problem(ndim, LIKE_GAUSS_IID, [c], PRIOR_AFFINE,
                   [prior_halfwidth, 0.0], logz_truth=truth,
                   name=name or f"gauss_iid{ndim}")


def gauss_corr(ndim=25, rho=0.4, prior_halfwidth=5.0, name=None):
    """C2: unit-variance Normal with uniform off-diagonal correlation ``rho``."""
    cov = np.full((ndim, ndim), rho)
    np.fill_diagonal(cov, 1.0)
    prec = np.linalg.inv(cov)
    prec = 0.5 * (prec + prec.T)
    _, logdet = np.linalg.slogdet(cov)
    c = -0.5 * (ndim * math.log(2.0 * math.pi) + logdet)
    # the prior box truncates a negligible part of the mass (|v|<5 sigma)
    truth = -ndim * math.log(2.0 * prior_halfwidth)
    par = np.concatenate([[c], prec.ravel()])
    return Problem(ndim, LIKE_GAUSS_PREC, par, PRIOR_AFFINE,
                   [prior_halfwidth, 0.0], logz_truth=truth,
                   name=name or f"gauss_corr{ndim}")


def eggbox(ndim=2, tmax=5.0 * math.pi, name=None):
    """C3: eggbox on the unit square (identity prior)."""
    return Problem(ndim, LIKE_EGGBOX, [tmax], PRIOR_IDENTITY, [],
                   logz_truth=235.856 if ndim == 2 else None,
                   name=name or f"eggbox{ndim}")


def gauss_normal_prior(ndim=200, name=None):
    """C4: iid N(0,1) likelihood with an N(0,1) prior via ndtri."""
    c = -0.5 * ndim * math.log(2.0 * math.pi)
    truth = -0.5 * ndim * math.log(2.0 * math.pi) - 0.5 * ndim * math.log(2.0)
    return Problem(ndim, LIKE_GAUSS_IID, [c], PRIOR_NORMAL, [0.0, 1.0],
                   logz_truth=truth, name=name or f"gauss_nprior{ndim}")


def prior_table(rows):
    """Per-coordinate priors: rows like ('uniform', lo, hi), ('normal', mu, sigma), ('loguniform', lo, hi).
    Returns the (ndim, 3) table [kind, p0, p1] that PRIOR_TABLE stores."""
    out = np.empty((len(rows), 3))
    for i, row in enumerate(rows):
        kind, a, b = row
        if kind not in _TABLE_KINDS:
            raise ValueError(f"prior row {i}: kind {kind!r} (one of {sorted(_TABLE_KINDS)})")
        a, b = float(a), float(b)
        if not (math.isfinite(a) and math.isfinite(b)):
            raise ValueError(f"prior row {i}: a parameter is not finite")
        if kind == "uniform":
            if not b > a:
                raise ValueError(f"prior row {i}: uniform needs lo < hi")
            out[i] = TABLE_UNIFORM, a, b - a
        elif kind == "normal":
            if not b > 0.0:
                raise ValueError(f"prior row {i}: normal needs sigma > 0")
            out[i] = TABLE_NORMAL, a, b
        else:
            if not (a > 0.0 and b > a):
                raise ValueError(f"prior row {i}: loguniform needs 0 < lo < hi")
            out[i] = TABLE_LOGUNIFORM, math.log(a), math.log(b / a)
    if len(rows) < 1 or not np.all(np.isfinite(out)):
        raise ValueError("prior table: no rows, or a stored parameter is not finite")
    return out


def _as_table(prior, ndim):
    tab = prior if isinstance(prior, np.ndarray) else prior_table(list(prior))
    if tab.shape != (ndim, 3):
        raise ValueError(f"the prior table has {tab.shape[0]} rows, the problem {ndim} coordinates")
    return tab


def mixture_logz(means, covs, weights, table, nsigma=6.0):
    """ln Z of a normalised Gaussian mixture under a table of uniform / normal rows, or None where it is not analytic.

    Uniform coordinates: the box is taken to hold every component (refused -- None -- unless mean +- nsigma standard
    deviations lies inside: at 6 the neglected mass is < 2e-9 per side), so they integrate to 1 / width and leave the
    marginal N(mu_N, C_NN) over the normal coordinates, whose integral against the prior N(mu0, diag(s^2)) is
    N(mu0; mu_N, C_NN + diag(s^2)).  A log-uniform row has no closed form: None."""
    kinds = table[:, 0]
    if np.any(kinds == TABLE_LOGUNIFORM):
        return None
    iu, inn = np.flatnonzero(kinds == TABLE_UNIFORM), np.flatnonzero(kinds == TABLE_NORMAL)
    terms = []
    for w, mu, cov in zip(weights, means, covs):
        sd = np.sqrt(np.diag(cov))
        lo, hi = table[iu, 1], table[iu, 1] + table[iu, 2]
        if np.any(mu[iu] - nsigma * sd[iu] < lo) or np.any(mu[iu] + nsigma * sd[iu] > hi):
            return None
        t = math.log(w) - float(np.sum(np.log(table[iu, 2])))
        if len(inn):
            c = cov[np.ix_(inn, inn)] + np.diag(table[inn, 2]**2)
            d = table[inn, 1] - mu[inn]
            _, logdet = np.linalg.slogdet(c)
            t += -0.5 * (len(inn) * math.log(2.0 * math.pi) + logdet + float(d @ np.linalg.solve(c, d)))
        terms.append(t)
    tmax = max(terms)
    return tmax + math.log(sum(math.exp(t - tmax) for t in terms))


def gauss_mixture(means, covs, weights=None, prior=None, name=None):
    """A normalised mixture of M <= 8 Gaussians, sum_m w_m N(v; mean_m, cov_m), under a per-coordinate prior table
    (rows as for prior_table, or its result; default: a uniform box of every mean +- 10 standard deviations)."""
    means = np.atleast_2d(np.asarray(means, dtype=np.float64))
    m, n = means.shape
    covs = np.asarray(covs, dtype=np.float64)
    if covs.ndim == 2:
        covs = np.broadcast_to(covs, (m, n, n))
    if not 1 <= m <= MIX_MAX:
        raise ValueError(f"a Gaussian mixture has 1..{MIX_MAX} components, got {m}")
    if covs.shape != (m, n, n):
        raise ValueError(f"covs has shape {covs.shape}, need {(m, n, n)}")
    w = np.full(m, 1.0 / m) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (m,) or not np.all(np.isfinite(w)) or not np.all(w > 0.0):
        raise ValueError("weights: one positive finite number per component")
    w = w / w.sum()
    if not (np.all(np.isfinite(means)) and np.all(np.isfinite(covs))):
        raise ValueError("a mean or a covariance is not finite")
    par = [np.array([float(m)])]
    for k in range(m):
        cov = 0.5 * (covs[k] + covs[k].T)
        try:
            np.linalg.cholesky(cov)
        except np.linalg.LinAlgError:
            raise ValueError(f"component {k}: the covariance is not positive definite") from None
        prec = np.linalg.inv(cov)
        prec = 0.5 * (prec + prec.T)
        _, logdet = np.linalg.slogdet(cov)
        c = math.log(w[k]) - 0.5 * logdet - 0.5 * n * math.log(2.0 * math.pi)
        par += [np.array([c]), means[k], prec.ravel()]
    if prior is None:
        sd = np.sqrt(np.array([np.diag(c) for c in covs]))
        prior = [("uniform", lo, hi) for lo, hi in zip((means - 10.0 * sd).min(axis=0), (means + 10.0 * sd).max(axis=0))]
    tab = _as_table(prior, n)
    return Problem(n, LIKE_GAUSS_MIX, np.concatenate(par), PRIOR_TABLE, tab.ravel(),
                   logz_truth=mixture_logz(means, covs, w, tab), name=name or f"gauss_mix{m}x{n}")


def gauss_general(mean, cov, prior=None, name=None):
    """A Gaussian likelihood N(v; mean, cov) with any mean: the one-component mixture (no exp, no log on the way)."""
    mean = np.asarray(mean, dtype=np.float64)
    return gauss_mixture(mean[None, :], np.asarray(cov, dtype=np.float64)[None, :, :], None, prior,
                         name or f"gauss_general{mean.size}")


BASELINE_PROBLEMS = {
    "C1": lambda: gauss_iid(3, 10.0, "C1"),
    "C2": lambda: gauss_corr(25, 0.4, 5.0, "C2"),
    "C3": lambda: eggbox(2, name="C3"),
    "C4": lambda: gauss_normal_prior(200, "C4"),
}
