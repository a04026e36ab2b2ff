"""Ellipsoid.scale_to_logvol restated on the stored principal axes (the function dynesty_amd/bounding.py's header says
the device computes), the reference scale_logvol_kernel is held to through dh_scale_to_logvol, dh_enlarge_batch_dev
and dh_enlarge_runs, and the bounds an fp64 evaluation of it has to keep.  Plain Python: no device code, nothing taken
from the kernel's operation order.

The function, for one ellipsoid (cov, am, axes, axlens, logvol) of dimension D and a target:
    logf = target - logvol      cap = ln(sqrt(D) / 2)      lax_k = ln axlens_k
  isotropic iff max lax < cap - logf / D:  f = exp(logf / D),
    cov' = cov f^2    am' = am / f^2    axes' = axes f    axlens' = axlens f
  otherwise the axes are visited by descending lax with left = logf, nleft = D:
    delta_k = max(min(cap - lax_k, left / nleft), 0),  left -= delta_k,  nleft -= 1,  fax_k = exp(delta_k)
    axlens'_k = axlens_k fax_k          axes'_ik = axes_ik fax_k
    cov'_ij = sum_k axes_ik axes_jk fax_k^2        am'_ij = sum_k axes_ik axes_jk / (axlens_k^4 fax_k^2)
  logvol' = target in both, exactly (also where capped axes leave volume unspent).

Precision.  The D logarithms, the chain and the D exponentials of an ellipsoid come from mpmath at 50 digits
(`scalars`); they enter the long-double part as sums of two doubles (2^-106).  Sums and products are np.longdouble.

Bounds (u = 2^-53; derived, none fitted to a device; every bound is multiplied by 1 + 2^-20 for the second-order terms,
which is ample while the first-order sum stays below 2^-20, and it stays below 2^-36).
One ulp is granted to each log and exp of the evaluation under test: 2u relative (2u |log x| absolute for a
logarithm).  `calibrate()` measures NumPy's float64 log / exp against long double on these arguments and
tests/test_scale_hp_cpu.py asserts <= 1 ulp there; the figure is never taken from a device.

  Isotropic branch, x = logf / D.  logf is one rounded difference (u |logf|), the division rounds once more:
  |err x| <= 2u |x|.  f = exp(x) then carries e_f = 2u |x| + 2u.  f^2 rounds once (2 e_f + u), 1 / f^2 once more, and
  each output is one more product:
      cov' 2 e_f + 2u    am' 2 e_f + 3u    axes', axlens' e_f + u          relative, per element.
  With logf == 0 every factor is exactly 1 (exp(0) = 1, products by 1 are exact): the bounds are 0.

  Greedy chain.  min and max are 1-Lipschitz in the sup norm, so the error of delta_k is the larger of the errors of
  its two arguments and no decision margin is needed inside the chain:
      err lax_k = 2u |lax_k|             (the granted ulp)
      err cap   = u + 2u |cap|           (sqrt rounds once: u relative, u in the logarithm; /2 is exact; the log)
      err t1    = err cap + err lax_k + u |t1|,   t1 = cap - lax_k
      err t2    = E / nleft + u |t2|,             t2 = left / nleft,   E = accumulated error of left (E_0 = u |logf|)
      d_k       = max(err t1, err t2);            E <- E + d_k + u |left - delta_k|
  Where min(t1, t2) < -d_k the evaluation's delta_k is 0 itself, not a rounded number: d_k = 0, fax_k = exp(0) = 1
  exactly, left is unchanged and so is E.  Otherwise fax_k carries r_k = d_k + 2u.  Exactly tied axes get equal
  delta in either order; a tied group takes the largest d_k of its members.
      axlens'_k, axes'_ik:  r_k + u relative (one product); 0 where r_k = 0 -- bit for bit.
      cov'_ij, am'_ij:  a sum of D three-factor terms in any order.  A term axes_ik axes_jk w_k has its two
        products, at most six more roundings inside the weight w_k (quotients by axlens_k, axlens_k^2, two products
        by fax_k, a reciprocal) and two to spare: 10u; the sum adds at most D - 1 roundings to a term, in any order;
        fax_k enters the weight squared: 2 r_k.  With S_ij = sum_k |axes_ik axes_jk| w_k:
            |err| <= sum_k |axes_ik axes_jk| w_k ((D + 10) u + 2 r_k).
        am' carries axlens^-4: an axis ratio kappa shows as kappa^2 in the weights, not in the coefficient.

  The reference's own roundings (2^-64 each): 4 per element on the isotropic branch, D + 8 per term on the greedy one.

Decisions.  margin = (cap - logf / D) - max lax; isotropic iff margin > 0.  The evaluation's margin is off by at most
    B = 2u max|lax| + (u + 2u |cap|) + 2u |x| + u |cap - x|
(the logs, cap, x, the subtraction).  DECIDED iff |margin| > B.  The two branches are continuous across margin = 0:
at |margin| <= B their delta differ by at most B (1 + 1 / (D - 1)), and cov f^2 differs from sum_k axes axes f^2 by
the input's own rounding of cov (u |cov_ij|, the cases round cov and am once from long double, whose sum adds
D 2^-64 S).  An undecided case is therefore held to the larger of the two branches' bounds plus
(u + D 2^-64 + 2 B (1 + 1 / (D - 1))) S_ij for cov' and am', and B (1 + 1 / (D - 1)) relative for axes' and axlens'.
(This is looser, by these few u, than holding it to the bound of the branch the reference lies inside: an evaluation may
rightly take the other branch there, and its bound and the gap between the branches have to be allowed for.  It touches
the two +-B/8 ellipsoids of each `edge` case only.)
The visit order is a decision only between distinct lax; the cases keep distinct lax 1e-9 apart (the error of a lax
is below 1e-13) and use exact ties otherwise.
"""
import mpmath as mp
import numpy as np

LD = np.longdouble
# the extended type must carry at least 60 bits, or the sums below would have to move to mpmath
assert np.finfo(LD).eps <= 2.0**-60, "np.longdouble is not an extended type here: do the arithmetic in mpmath"

U = 2.0 ** -53
U_LD = 2.0 ** -64
ULP = 2.0 * U  # the granted ulp of a log / exp, relative
SECOND = 1.0 + 2.0 ** -20
DPS = 50
FIELDS = ("cov", "am", "axes", "axlens", "logvol")


def ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def split(x):
    """An mpf as (hi, lo) doubles: hi + lo carries 106 bits."""
    hi = float(x)
    return hi, float(x - mp.mpf(hi))


def join(hi, lo):
    return ld(hi) + ld(lo)


def calibrate(n=200000, seed=5):
    """Largest error in ulps of NumPy's float64 log and exp against long double on the arguments scale_to_logvol puts
    them to: logs of axis lengths 1e-8 ... 20, exponentials of |delta| <= 3."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, f, x in (("log", np.log, np.exp(rng.uniform(np.log(1e-8), np.log(20.0), n))),
                       ("exp", np.exp, rng.uniform(-3.0, 3.0, n))):
        got, want = f(x), f(x.astype(LD))
        out[name] = float(np.max(np.abs(got.astype(LD) - want) / np.spacing(np.abs(got))))
    return out


def scalars(axlens, logvol, target):
    """The D numbers of one ellipsoid at 50 digits and the error chain of the module docstring (plain floats).
    Returns a dict: iso, margin, dec_bound, decided, x, lax, order (the visit, descending lax), and per branch the
    reference may be held to (its own; both when undecided) b_iso / b_greedy = dict(delta (hi, lo), fax (hi, lo),
    d (err of delta), r (relative err of fax; on the isotropic branch e_f for every axis))."""
    axl = [float(a) for a in np.asarray(axlens, dtype=np.float64)]
    D = len(axl)
    with mp.workdps(DPS):
        logf = mp.mpf(float(target)) - mp.mpf(float(logvol))
        cap = mp.log(mp.sqrt(D) / 2)
        lax = [mp.log(mp.mpf(a)) for a in axl]
        x = logf / D
        margin = (cap - x) - max(lax)
        iso = bool(margin > 0)
        a_err = [ULP * abs(float(l)) for l in lax]
        c_err = U + ULP * abs(float(cap))
        e_x = 2 * U * abs(float(x))
        dec_bound = SECOND * (max(a_err) + c_err + e_x + U * abs(float(cap - x)))
        order = sorted(range(D), key=lambda k: lax[k], reverse=True)
        out = dict(iso=iso, margin=float(margin), dec_bound=dec_bound, decided=bool(abs(margin) > dec_bound),
                   order=np.array(order), x=float(x), lax=np.array([float(l) for l in lax]))
        groups = {}
        for k, a in enumerate(axl):  # equal lax iff equal axlens
            groups.setdefault(a, []).append(k)
        for branch in ("iso", "greedy"):
            if out["decided"] and (branch == "iso") != iso:
                continue
            if branch == "iso":
                delta = [x] * D
                e_f = 0.0 if logf == 0 else e_x + ULP
                d = [e_x] * D
                r = [e_f] * D
            else:
                delta, d, r = [None] * D, [0.0] * D, [0.0] * D
                left, nleft, E = logf, D, U * abs(float(logf))
                for k in order:
                    t1, t2 = cap - lax[k], left / nleft
                    dk = max(c_err + a_err[k] + U * abs(float(t1)), E / nleft + U * abs(float(t2)))
                    m = min(t1, t2)
                    if m < -dk:  # delta_k is the constant 0 of the max, fax_k = exp(0) = 1: nothing is rounded
                        delta[k] = mp.mpf(0)
                    else:
                        delta[k] = max(m, mp.mpf(0))
                        d[k], r[k] = dk, dk + ULP
                        left -= delta[k]
                        E += dk + U * abs(float(left))
                    nleft -= 1
                for tied in groups.values():  # exactly tied axes: either may come first
                    if len(tied) > 1:
                        dm, rm = max(d[j] for j in tied), max(r[j] for j in tied)
                        for j in tied:
                            d[j], r[j] = dm, rm
            out["b_" + branch] = dict(delta=np.array([split(v) for v in delta]).T, fax=np.array([split(mp.exp(v)) for v in delta]).T,
                               d=np.array(d), r=np.array(r))
    return out


def own(sc):
    """The chain of the branch the reference takes."""
    return sc["b_iso" if sc["iso"] else "b_greedy"]


def _outputs(branch, sc, cov, am, axes, axlens, rows, want_s=False):
    """(values, bounds, S) of one branch in long double; cov / am / axes restricted to `rows`; S only where asked for."""
    D = len(axlens)
    b = sc["b_" + branch]
    fax, r = join(*b["fax"]), ld(b["r"])
    X, a = ld(axes), ld(axlens)
    Xr = X[rows]
    one = ld(b["r"] > 0)  # a factor that is exactly 1 rounds nothing
    val, bnd, S = {}, {}, {}
    val["axlens"] = a * fax
    bnd["axlens"] = np.abs(val["axlens"]) * (SECOND * (r + U * one) + 3 * U_LD * one)
    val["axes"] = Xr * fax
    bnd["axes"] = np.abs(val["axes"]) * (SECOND * (r + U * one) + 3 * U_LD * one)
    if branch == "iso":
        f, e_f = fax[0], r[0]
        f2 = f * f
        nz = LD(1 if e_f > 0 else 0)
        val["cov"], val["am"] = ld(cov)[rows] * f2, ld(am)[rows] / f2
        bnd["cov"] = np.abs(val["cov"]) * (SECOND * (2 * e_f + 2 * U * nz) + 4 * U_LD * nz)
        bnd["am"] = np.abs(val["am"]) * (SECOND * (2 * e_f + 3 * U * nz) + 4 * U_LD * nz)
        S["cov"], S["am"] = np.abs(val["cov"]), np.abs(val["am"])
    else:
        a2 = a * a
        for name, w in (("cov", fax * fax), ("am", 1 / (a2 * a2 * fax * fax))):
            coeff = SECOND * ((D + 10) * U + 2 * r) + (D + 8) * U_LD
            val[name] = (Xr * w) @ X.T
            bnd[name] = (np.abs(Xr) * (w * coeff)) @ np.abs(X).T
            if want_s:
                S[name] = (np.abs(Xr) * w) @ np.abs(X).T
    return val, bnd, S


def reference(cov, am, axes, axlens, logvol, target, sc=None, rows=None):
    """The five outputs of one ellipsoid and their bounds, as two dicts over FIELDS (long double; logvol a float with
    bound 0), and the scalars.  rows: the rows of cov / am / axes to evaluate (None: all)."""
    D = len(axlens)
    sc = scalars(axlens, logvol, target) if sc is None else sc
    rows = np.arange(D) if rows is None else np.asarray(rows)
    own, other = ("iso", "greedy") if sc["iso"] else ("greedy", "iso")
    val, bnd, S = _outputs(own, sc, cov, am, axes, axlens, rows, want_s=not sc["decided"])
    if not sc["decided"]:
        _, bnd2, _ = _outputs(other, sc, cov, am, axes, axlens, rows)
        gap = LD(sc["dec_bound"]) * (1 + LD(1) / max(D - 1, 1))
        for name in ("cov", "am"):
            bnd[name] = np.maximum(bnd[name], bnd2[name]) + (U + D * U_LD + 2 * gap) * S[name]
        for name in ("axes", "axlens"):
            bnd[name] = np.maximum(bnd[name], bnd2[name]) + gap * np.abs(val[name])
    val["logvol"], bnd["logvol"] = float(target), 0.0
    return val, bnd, sc


def ratios(out, val, bnd, rows=None):
    """error / bound per field for one ellipsoid's outputs `out` (dict over FIELDS, float64); an element whose bound
    is 0 must be met exactly (counted as 0, or inf when it is not)."""
    res = {}
    for name in FIELDS:
        got = np.asarray(out[name], dtype=np.float64)
        if rows is not None and name in ("cov", "am", "axes"):
            got = got[rows]
        if name == "logvol":
            res[name] = 0.0 if float(got) == val[name] else np.inf
            continue
        if not np.all(np.isfinite(got)):
            res[name] = np.inf
            continue
        err = np.abs(got.astype(LD) - val[name])
        b = np.asarray(bnd[name], dtype=LD)
        zero = b == 0
        worst = 0.0
        if zero.any() and np.any(err[zero] != 0):
            worst = np.inf
        if (~zero).any():
            worst = max(worst, float(np.max(err[~zero] / b[~zero])))
        res[name] = worst
    return res


def fresh_eigh_bounds(cov, axes, axlens, fax, r):
    """Bounds for an evaluator that decomposes the stored cov afresh on the greedy branch (oracle.bounding_ref:
    lam, vec = eigh(cov); cov' = vec diag(lam fax^2) vec^T, am' = vec diag(1 / (lam fax^2)) vec^T, the factors paired
    with the eigenvalues by ascending index).  That is another function of the input than the one on the stored axes,
    and the distance between the two is the conditioning of the decomposition.  Frobenius norms over the whole matrix.

    Write Q = axes / axlens, l_k = axlens_k^2, w_k = fax_k^2, g_k = w_k l_k (cov') or 1 / (w_k l_k) (am'), and
    R = Q diag(g) Q^T for the reference on the stored axes.
      (1) Q is orthogonal only to eta = |Q^T Q - I|_F (long double).  Its polar factor P has |Q - P|_F <= eta, and
          A0 = P diag(l) P^T has the eigen-system (l, P) exactly:  |R - P diag(g) P^T|_F <= (2 + eta) eta max|g|.
      (2) The stored cov:  |cov - A0|_F <= (2 + eta) eta max l + u |cov|_F + D^2 2^-64 max l   (Q, its one rounding, the
          long-double sum).
      (3) eigh is backward stable: its output is the eigen-system of cov + E2, |E2|_2 <= p(D) u |cov|_2, with vectors
          orthogonal to p(D) u.  LAPACK states p as "a modestly growing function"; p(D) = D is GRANTED here (recorded in
          EXPERIMENTS.md).  |E2|_F <= D^1.5 u |cov|_F.       E = (2) + (3).
      (4) For G(A) = sum_k g_k(l_k(A)) q_k q_k^T first-order perturbation theory (d l_k = E_kk, d q_k = sum_j E_jk /
          (l_k - l_j) q_j) gives, in the eigenbasis, dG_ij = Phi_ij E_ij with Phi_ij = (g_i - g_j) / (l_i - l_j) and
          Phi_ii = g_i': the eigenvalue gaps, weighted by the differences of the factors.  Axes that share a factor (the
          uncapped ones; exact ties) have Phi = w or -1 / (w l_i l_j) whatever their gap.  |dG|_F <= max|Phi| |E|_F.
          The case is POSED for such an evaluator when E <= gap / 8 for every pair with different factors, and, for
          am', E <= min l / 8; then sin(theta) <= E / (gap - E) and the moved eigenvalues change a divided difference
          by at most gap / (gap - 2 E): together below 2, the factor granted for the remainder.  Where it is not posed
          the decomposition mixes the axes whose factors differ and no bound exists: (False, inf, inf).
      (5) The evaluator's own roundings: fax from its float64 chain (2 max r |R|_F), the product vec diag vec^T
          ((D + 4) u per element, elements <= max|g|: D (D + 4) u max|g|) and the vectors' orthogonality
          (3 D^1.5 u max|g|).
    Returns (posed, bound for cov', bound for am')."""
    X, a, fax = ld(axes), ld(axlens), np.asarray(fax, dtype=LD)
    D = len(a)
    Q = X / a
    eta = LD(np.sqrt(np.sum((Q.T @ Q - np.eye(D, dtype=LD)) ** 2)))
    lam, w = a * a, fax * fax
    cov_f = LD(np.sqrt(np.sum(ld(cov) ** 2)))
    E = (2 + eta) * eta * lam.max() + U * cov_f + D * D * U_LD * lam.max() + D ** 1.5 * U * cov_f
    dl = lam[:, None] - lam[None, :]
    dw = np.abs(w[:, None] - w[None, :]) > 1e-12 * w.max()
    off = dl != 0
    gap = np.abs(dl[off & dw])
    posed = bool((gap.size == 0 or E <= gap.min() / 8) and E <= lam.min() / 8)
    if not posed:
        return False, np.inf, np.inf
    rmax = LD(np.max(r))
    out = []
    for g, dg in ((w * lam, w), (1 / (w * lam), 1 / (w * lam * lam))):
        phi = np.abs(dg).max()
        if off.any():
            phi = max(phi, np.abs((g[:, None] - g[None, :])[off] / dl[off]).max())
        gmax = np.abs(g).max()
        r_f = LD(np.sqrt(np.sum(((Q * g) @ Q.T) ** 2)))
        out.append(float((2 + eta) * eta * gmax + 2 * phi * E + 2 * rmax * r_f +
                         (D * (D + 4) + 3 * D ** 1.5) * U * gmax))
    return True, out[0], out[1]
