"""High-precision reference of the bounding-ellipsoid linear algebra (include/dynhip.h: dh_rebuild, dh_ell_from_cov,
dh_improve_covar_mat, dh_contains) and error bounds for an fp64 evaluation of it.  Plain Python: no device code,
nothing taken from the operation order of csrc/.

Two layers, so that no GPU test runs an mpmath eigen-solve:

  generator side (mpmath, DPS digits; tools/make_golden.py ell_hp and tests/test_ell_hp_cpu.py) -- the fp64 input is
  exact data:
    bounding_ellipsoid_hp(pts)   mean, covariance (ddof = 1), spectrum, improve_covar_mat verdict and result, largest
                                 Mahalanobis form fmax, the rescaling by fmax / (1 - 1e-3), ln V
    improve_covar_mat_hp(A)      the regularisation loop as include/dynhip.h states it for dh_improve_covar_mat
    ell_from_cov_hp(A)           spectrum and ln V of a positive definite matrix
    each with the decision margins (MARGIN_* below)

  test side (np.longdouble): residuals that need no eigen-solve, taken against the evaluator's OWN returned
  covariance, so that a covariance error does not compound into the eigen checks (hp_ref.loglike_bound takes the
  evaluator's own v for the same reason), and the bounds, each with its derivation beside it (EPS = 2^-53).

What cannot be proved is said where it stands: C_EIG and C_INV.
"""
import math

import mpmath as mp
import numpy as np

LD = np.longdouble
# the extended type must carry at least 60 bits, or the residuals below would have to move to mpmath
assert np.finfo(LD).eps <= 2.0**-60, "np.longdouble is not an extended type here: do the arithmetic in mpmath"

EPS = 2.0**-53
DPS = 50
ROUND_DELTA = 1e-3
LIM = 1.0 - ROUND_DELTA
NTRIES = 100

# margins, in fixture order
MARGIN_LOGK, MARGIN_TRTR, MARGIN_GAP, MARGIN_R = range(4)


# =========================================================================================================
# generator side: mpmath
# =========================================================================================================
def _obj(a):
    """fp64 array -> object array of mpf (exact)."""
    a = np.asarray(a, dtype=np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx, v in np.ndenumerate(a):
        out[idx] = mp.mpf(float(v))
    return out


def _eig_mp(a, vectors):
    """Ascending spectrum (list of mpf) and eigenvectors (object array, columns; None unless asked for) of a
    symmetric object matrix.  A diagonal matrix is its own decomposition (exactly)."""
    d = a.shape[0]
    if all(a[i, j] == 0 for i in range(d) for j in range(d) if i != j):
        order = sorted(range(d), key=lambda i: a[i, i])
        vec = np.array([[mp.mpf(1 if i == order[k] else 0) for k in range(d)] for i in range(d)], dtype=object)
        return [a[i, i] for i in order], (vec if vectors else None)
    m = mp.matrix(a.tolist())
    if not vectors:
        e = mp.eigsy(m, eigvals_only=True)
        return sorted(e[i] for i in range(d)), None
    e, q = mp.eigsy(m)
    order = sorted(range(d), key=lambda i: e[i])
    vec = np.array([[q[i, k] for k in order] for i in range(d)], dtype=object)
    return [e[k] for k in order], vec


def blend_coeff(trial):
    """The fp64 coefficient of blend `trial` (an exact datum for the reference, as every fp64 input is)."""
    return 1e-10 * (1.0 / 1e-10)**(trial * 1.0 / (NTRIES - 1))


def _hilo(x):
    hi = float(x)
    return hi, float(x - mp.mpf(hi))


def _margins(lam, r_min):
    """lam ascending (mpf).  log10(kappa) - 12 (nan unless positive); tr * tr^-1 (nan unless positive); relative gap
    of the two leading eigenvalues (nan for D = 1); the smallest |lam_min / lam_max - 1e-12| any trial met (or, in a
    trial whose top eigenvalue is not positive, its distance from zero relative to the largest modulus)."""
    top, bot = lam[-1], lam[0]
    pos = bot > 0
    logk = float(mp.log10(top / bot) - 12) if pos else math.nan
    trtr = float(sum(lam) * sum(1 / x for x in lam)) if pos else math.nan
    gap = float((lam[-1] - lam[-2]) / abs(lam[-1])) if len(lam) > 1 and lam[-1] != 0 else math.nan
    return np.array([logk, trtr, gap, r_min])


def _regularize_spectrum(lam):
    """The loop of dh_improve_covar_mat on an exact spectrum.  Every step keeps the eigenvectors (a floor replaces
    eigenvalues, a blend (1 - c) A + c I maps lam -> (1 - c) lam + c), so the loop runs on the spectrum alone.
    Returns (state, trials, spectrum, floored, alpha, beta, r_min): state 0 = accepted, 1 = identity after NTRIES
    failures; while nothing was floored the result is alpha * A + beta * I."""
    cur = list(lam)
    alpha, beta = mp.mpf(1), mp.mpf(0)
    floored = False
    r_min = math.inf
    for trial in range(NTRIES):
        top, bot = max(cur), min(cur)
        if top <= 0:
            failed = 2
            big = max(abs(x) for x in cur)
            if big > 0:  # (an all-zero matrix has an exact spectrum in any arithmetic)
                r_min = min(r_min, float(-top / big))
        else:
            r_min = min(r_min, abs(float(bot / top - mp.mpf(10)**-12)))
            failed = 1 if bot * mp.mpf(10)**12 < top else 0
        if failed == 0:
            return 0, trial, cur, floored, alpha, beta, r_min
        if failed == 1:
            floor = 10 * top / mp.mpf(10)**12
            cur = [max(x, floor) for x in cur]
            floored = True
        else:
            c = mp.mpf(blend_coeff(trial))
            cur = [(1 - c) * x + c for x in cur]
            alpha, beta = (1 - c) * alpha, (1 - c) * beta + c
    return 1, NTRIES - 1, [mp.mpf(1)] * len(cur), False, mp.mpf(0), mp.mpf(1), r_min


def improve_covar_mat_hp(a, _obj_in=False):
    """dict: good, trials, lam_in / lam_out (ascending mpf), cov_out (object matrix; None when the input is returned
    unchanged), vec (eigenvectors, only when something was floored), alpha / beta, margins of the INPUT."""
    with mp.workdps(DPS):
        a = a if _obj_in else _obj(a)
        d = a.shape[0]
        lam, _ = _eig_mp(a, False)
        state, trials, cur, floored, alpha, beta, r_min = _regularize_spectrum(lam)
        vec = None
        if state == 1:
            cov = np.array([[mp.mpf(1 if i == j else 0) for j in range(d)] for i in range(d)], dtype=object)
        elif trials == 0:
            cov = None
        elif floored:
            _, vec = _eig_mp(a, True)
            # the k-th column belongs to lam[k]; floor and blends are monotone, so cur[k] belongs to it too
            cov = (vec * np.array(cur, dtype=object)[None, :]).dot(vec.T)
        else:
            cov = alpha * a + beta * np.array([[mp.mpf(1 if i == j else 0) for j in range(d)] for i in range(d)],
                                              dtype=object)
        return dict(good=trials == 0, trials=trials, lam_in=lam, lam_out=sorted(cur), lam_out_by_vec=cur, cov_out=cov,
                    vec=vec, floored=floored, alpha=alpha, beta=beta, margins=_margins(lam, r_min))


def logvol_prefactor_mp(d):
    """ln volume of the unit d-ball."""
    return mp.mpf(d) / 2 * mp.log(mp.pi) - mp.loggamma(mp.mpf(d) / 2 + 1)


def ell_from_cov_hp(a):
    with mp.workdps(DPS):
        lam, _ = _eig_mp(_obj(a), False)
        if not lam[0] > 0:
            raise ValueError("ell_from_cov_hp: the matrix is not positive definite")
        lnv = logvol_prefactor_mp(len(lam)) + sum(mp.log(x) for x in lam) / 2
        return dict(lam=lam, lnv=lnv, margins=_margins(lam, abs(float(lam[0] / lam[-1]) - 1e-12)))


def ld_solve(a, b):
    """x with a x = b in np.longdouble: Gaussian elimination with partial pivoting."""
    a, b = np.array(a, dtype=LD), np.array(b, dtype=LD)
    d = a.shape[0]
    for k in range(d):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]], b[[k, p]] = a[[p, k]], b[[p, k]]
        f = a[k + 1:, k] / a[k, k]
        a[k + 1:] -= f[:, None] * a[k][None, :]
        b[k + 1:] -= f[:, None] * b[k][None, :]
    x = np.empty_like(b)
    for k in range(d - 1, -1, -1):
        x[k] = (b[k] - a[k, k + 1:] @ x[k + 1:]) / a[k, k]
    return x


def bounding_ellipsoid_hp(pts):
    """bounding_ellipsoid of an (n, D) fp64 cloud at DPS digits.  dict: mean (mpf list), cov (object matrix), icm (the
    improve_covar_mat_hp record of the first pass), fmax, mult, lam (final spectrum, ascending), lnv, margins."""
    pts = np.asarray(pts, dtype=np.float64)
    n, d = pts.shape
    with mp.workdps(DPS):
        x = _obj(pts)
        mean = x.sum(axis=0) / mp.mpf(n)
        dm = x - mean[None, :]
        cov = dm.T.dot(dm) / mp.mpf(n - 1)
        icm = improve_covar_mat_hp(cov, _obj_in=True)
        cov1 = cov if icm["cov_out"] is None else icm["cov_out"]
        # fmax: every point in long double first (relative accuracy cond * 2^-64 <= 1e-8 after a floor), then the
        # leaders again at full precision
        c64 = np.array([[float(v) for v in row] for row in cov1])
        d_ld = pts.astype(LD) - np.array([LD(mp.nstr(m, 25)) for m in mean])
        q_ld = np.sum(d_ld * ld_solve(c64, d_ld.T).T, axis=1).astype(np.float64)
        lead = np.flatnonzero(q_ld >= q_ld.max() * (1 - 1e-6))
        lead = np.union1d(lead, np.argsort(q_ld)[-3:])
        cm = mp.matrix(cov1.tolist())
        fmax = mp.mpf(0)
        for i in lead:
            rhs = mp.matrix([dm[i, j] for j in range(d)])
            sol = mp.lu_solve(cm, rhs) if d > 1 else mp.matrix([rhs[0] / cm[0, 0]])
            fmax = max(fmax, sum(rhs[j] * sol[j] for j in range(d)))
        assert abs(float(fmax) / q_ld.max() - 1) < 1e-6, "the long-double leaders missed the maximum"
        lim = mp.mpf(LIM)  # the fp64 constant 1 - 1e-3, as the evaluators hold it
        mult = fmax / lim if fmax > lim else mp.mpf(1)
        lam = [v * mult for v in icm["lam_out"]]
        if not icm["good"]:
            # the second pass sees the rescaled result of the first: it must be accepted as it stands, and the
            # points must be inside
            assert _regularize_spectrum(lam)[1] == 0 and fmax / mult < 1
        lnv = logvol_prefactor_mp(d) + sum(mp.log(v) for v in lam) / 2
        return dict(mean=list(mean), cov=cov, icm=icm, fmax=fmax, mult=mult, lam=lam, lnv=lnv,
                    margins=icm["margins"])


def fixture_record(rec, cov_scale=None):
    """What tests/golden/ell_hp.npz holds of one case: numeric arrays only.  `rec` is the dict of one of the three
    functions above; cov_scale multiplies the returned covariance (the cloud's rescaling)."""
    with mp.workdps(DPS):
        out = {}
        lam = rec["lam"] if "lam" in rec else rec["lam_out"]
        hl = [_hilo(v) for v in lam]
        out["lam_hi"] = np.array([h for h, _ in hl])
        # the low part relative to the high one (<= 2^-53 whatever the scale, so float32 holds it: 77 bits in all)
        out["lam_lo"] = np.array([l / h if h != 0 else 0.0 for h, l in hl], dtype=np.float32)
        if "lnv" in rec:
            out["lnv"] = np.array(_hilo(rec["lnv"]))
        if "fmax" in rec:
            out["fmax"] = np.float64(float(rec["fmax"]))
        out["margins"] = rec["margins"]
        icm = rec.get("icm", rec if "trials" in rec else None)
        if icm is not None:
            out["good"] = np.int32(icm["good"])
            out["trials"] = np.int32(icm["trials"])
            if icm["floored"]:
                sc = mp.mpf(1) if cov_scale is None else cov_scale
                out["cov_out"] = np.array([[float(v * sc) for v in row] for row in icm["cov_out"]])
            elif icm["trials"] > 0:
                out["ab"] = np.array(_hilo(icm["alpha"]) + _hilo(icm["beta"]))
        return out


# =========================================================================================================
# test side: np.longdouble residuals
# =========================================================================================================
def ld(a):
    return np.asarray(a).astype(LD)


def fro(a):
    a = ld(a)
    return float(np.sqrt(np.sum(a * a)))


def lam_ld(rec):
    """The fixture's spectrum as long double: hi * (1 + lo), lo the relative low part."""
    return rec["lam_hi"].astype(LD) * (LD(1) + rec["lam_lo"].astype(LD))


def cov_of_points_ld(pts):
    x = ld(pts)
    mu = x.sum(axis=0) / LD(len(x))
    d = x - mu
    return mu, d.T @ d / LD(len(x) - 1)


def quadforms_ld(pts, ctr, am):
    """(q, sabs): (x - c)^T A (x - c) and sum_ij |d_i| |A_ij| |d_j| of every point, in long double."""
    d = ld(pts) - ld(ctr)
    a = ld(am)
    return np.sum((d @ a) * d, axis=1), np.sum((np.abs(d) @ np.abs(a)) * np.abs(d), axis=1)


def logvol_prefactor(d):
    return 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)


# =========================================================================================================
# the bounds
# =========================================================================================================
# Factor of the eigen-system bounds.  A symmetric eigensolver built from orthogonal transformations (Jacobi rotations,
# Householder tridiagonalisation + QL) is backward stable:  the computed pairs are the exact ones of A + E with
# ||E|| <= p(D) eps ||A|| and the computed vectors orthonormal to p(D) eps, p "a modestly growing function of D"
# (Golub & Van Loan 8.5; Demmel & Veselic 1992 for Jacobi).  No textbook gives p as a number -- the provable worst
# cases (rotations times 6 eps, ~1e4 eps at D = 44) are far above what any solver shows -- so p(D) = C_EIG * D is NOT
# proved.  It is set from outside the code under test: LAPACK's dsyevd (the float64 oracle's solver in
# tests/test_ell_hp_cpu.py) and a textbook cyclic Jacobi in plain float64 stay below half of it on every case they are
# run on (tests/test_ell_hp_cpu.py prints and asserts that).
C_EIG = 8.0
# Factor of the orthogonality bound, c2(D) = C_ORTH D^1.5.  The eigenvectors of a Jacobi solver are a product of
# S (D - 1) plane rotations per column (S sweeps), and a computed rotation is orthogonal only to an ulp or two
# (c^2 + s^2 - 1, and the three roundings of c v0 - s v1), with a SIGN that does not average out: the column norms
# drift linearly, |u_k|^2 - 1 ~ beta S D eps, and ||U^T U - I||_F, which that diagonal dominates, grows like
# sqrt(D) S D eps -- D^1.5, not D.  Tridiagonalisation solvers apply D reflectors per column and show D or less, so a
# c D eps fitted to LAPACK alone (the first form of this bound) is a bound on LAPACK, not on "a backward-stable fp64
# solver": a textbook cyclic Jacobi in NumPy, run to off^2 <= 1e-31 dia^2, measures 0.17 S D^1.5 eps with S = 8..14 --
# 1.4 times 8 D eps at D = 43.  C_ORTH is set so that this Jacobi AND LAPACK stay below half of the bound; like C_EIG
# it is calibrated, not proved (the provable form, 10 sqrt(D) S (D - 1) eps, is a hundred times what either shows).
C_ORTH = 4.0
# Factor of the inverse's residual.  ||X A - I|| <= c D eps kappa(A) holds for an inverse formed from a backward
# stable factorisation (Higham, Accuracy and Stability, 14.1: c D eps || |X| |L| |U| || with growth omitted); the
# constant is unproved for the same reason as C_EIG and calibrated the same way (the oracle's V diag(1/lam) V^T
# measures at most 0.1 of it).
C_INV = 8.0


def c_eig(d):
    return C_EIG * d * EPS


def mean_bound(pts):
    """|mean_fp64 - mean| per coordinate: a sum of n terms in ANY order has relative error (n - 1) eps of
    sum |x|, the division one more, one spare:  (n + 1) eps mean|x_i|."""
    n = len(pts)
    return (n + 1) * EPS * np.mean(np.abs(pts), axis=0)


def mean_error(pts, ctr, mu):
    """|ctr - mean| per coordinate, measured: the long-double mean `mu` is itself only good to a few of ITS ulps of
    max|x| (n additions, but of same-sign terms in a type with 11 bits to spare: 4 ulp is ample), which next to an
    error of a fraction of an fp64 ulp is not nothing -- it is added."""
    return np.abs(ld(ctr) - mu) + 4 * np.finfo(LD).eps * LD(np.max(np.abs(pts)))


def cov_bound(pts, ctr):
    """Elementwise bound on |cov_fp64 - cov| for a two-pass covariance about the evaluator's own mean `ctr`
    (the rebuild's centre, or the k-means centroid a child keeps in its record).

    With ctr = mu + e:  sum (d_i - e_i)(d_j - e_j) = sum d_i d_j + n e_i e_j  exactly, because sum d = 0 about the
    true mean: a mean error enters at SECOND order only, n / (n - 1) |e_i| |e_j|.  e is measured (long double), not
    assumed; mean_bound() holds it separately.  For a cloud of width 1e-7 around 0.5 that term is (a few ulp of
    0.5)^2 ~ 1e-31 next to a covariance of 1e-15: visible, and inside the bound.
    The rounding of the sum itself: one subtraction per factor (2), one product, n - 1 additions in any order, one
    division, three spare:  (n + 6) eps S_ij  with  S_ij = sum |x_i - ctr_i| |x_j - ctr_j| / (n - 1).
    Returns (B, cov_ld, rho): rho = max_i B_ii / cov_ii, the relative error of a diagonal entry (and of the trace)."""
    n = len(pts)
    mu, cov = cov_of_points_ld(pts)
    e = mean_error(pts, ctr, mu).astype(np.float64)
    dabs = np.abs(ld(pts) - ld(ctr))
    s = (dabs.T @ dabs / LD(n - 1)).astype(np.float64)
    b = (n + 6) * EPS * s + n / (n - 1.0) * np.outer(e, e)
    diag = np.diag(cov).astype(np.float64)
    rho = float(np.max(np.diag(b) / diag)) if np.all(diag > 0) else math.inf
    return b, cov, rho


def eig_residual_bound(c):
    """||C - AX AX^T||_F <= c1(D) eps ||C||_F with c1(D) = C_EIG D (see C_EIG) plus 4 eps ||C||_F for forming
    AX = V sqrt(lam) (a square root and a product per entry: 2 eps on each of the two factors)."""
    return (c_eig(c.shape[0]) + 4 * EPS) * fro(c)


def orth_bound(d):
    """||U^T U - I||_F <= c2(D) eps, c2(D) = C_ORTH D^1.5 (see C_ORTH), plus 2 eps sqrt(D) for the division
    AX / axlens."""
    return C_ORTH * d**1.5 * EPS + 2 * EPS * math.sqrt(d)


def spectrum_bound(c, delta_in=0.0):
    """|axlens_k^2 - lam_k(C_true)| for every k.  From the two residuals, by the standard perturbation argument: with
    U^T U = I + F, AX AX^T = U diag(axlens^2) U^T is similar to diag(axlens^2) up to ||F|| ||C||, so the SET axlens^2
    is the exact spectrum of C + E, ||E|| <= eig_residual_bound + orth_bound ||C||; Weyl turns ||E|| and the input's
    own error delta_in (Frobenius, >= spectral) into the same absolute bound on every eigenvalue.  4 eps lam_k for
    squaring an axis length that was itself a rounded square root."""
    return delta_in + eig_residual_bound(c) + orth_bound(c.shape[0]) * fro(c)


def inverse_bound(d, kappa):
    """||AM C - I||_F <= C_INV D eps kappa(C) (see C_INV)."""
    return C_INV * d * EPS * kappa


def quadform_bound(d, sabs):
    """|q_fp64 - q| for q = sum_ij d_i A_ij d_j, d = x - c:  one subtraction per factor (2 eps), two products, D^2 - 1
    additions in any order (the VALU loop, the MFMA tiles and the wide form group them differently), one spare:
    (D^2 + 4) eps sum_ij |d_i| |A_ij| |d_j|."""
    return (d * d + 4) * EPS * np.asarray(sabs, dtype=np.float64)


def logvol_self_bound(d, axlens):
    """|ln V - (prefactor + sum ln axlens)|: D logarithms of relative error eps each and D additions in any order,
    (D + 4) eps (|prefactor| + sum |ln axlens_k|); an axis length within 3 eps of the square root of the eigenvalue
    the logarithm was taken of moves each term by 3 eps more."""
    mag = abs(logvol_prefactor(d)) + float(np.sum(np.abs(np.log(np.asarray(axlens, dtype=np.float64)))))
    return (d + 4) * EPS * mag + 3 * d * EPS


def log_spectrum_bound(spec_bound, lam):
    """|1/2 sum ln lam_hat_k - 1/2 sum ln lam_k| from |lam_hat_k - lam_k| <= spec_bound (Weyl):  with
    x_k = spec_bound / lam_k,  |ln(1 +- x)| <= x / (1 - x).  Where x_k >= 1/2 the eigenvalue is not determined and
    the bound is infinite (tests/test_ell_hp_cpu.py asserts that no case is there)."""
    x = spec_bound / np.asarray(lam, dtype=np.float64)
    if np.any(x >= 0.5):
        return math.inf
    return 0.5 * float(np.sum(x / (1 - x)))


def floored_cov_bound(d, b_fro, cnorm):
    """||cov_returned - V max(lam, floor) V^T||_F, floor = 1e-11 lam_max.  The map A -> V max(lam, f) V^T is the matrix
    function of g(x) = max(x, f), which is 1-Lipschitz, and a 1-Lipschitz function of a symmetric matrix is
    1-Lipschitz in the Frobenius norm (Bhatia, Matrix Analysis, VII.5.7 / X.2.2).  That is sharper than going through
    the Davis-Kahan rotation of the floored subspace and needs no gap: the input error b_fro and the solver's
    backward error pass through unamplified.  The floor moves with lam_max (1e-11 of its error, on at most D
    eigenvalues); recomposing V diag V^T in fp64 is another backward-error's worth; one ulp for the fixture's own
    rounding to float64."""
    ce = c_eig(d) * cnorm
    return b_fro + 2 * ce + d * 1e-11 * (b_fro + ce) + EPS * cnorm


# =========================================================================================================
# the checks, shared by the float64 oracle (tests/test_ell_hp_cpu.py) and the device (tests/test_gpu_ell_hp.py)
# =========================================================================================================
class Ratios(dict):
    """error / bound per bound name; add() keeps the worst."""

    def add(self, name, err, bound):
        err, bound = float(err), float(bound)
        if math.isnan(err):
            r = math.inf
        elif bound > 0:
            r = err / bound
        else:
            r = 0.0 if err == 0 else math.inf
        self[name] = max(self.get(name, 0.0), r)

    def merge(self, other):
        for k, v in other.items():
            self[k] = max(self.get(k, 0.0), v)

    def assert_ok(self, what):
        print(f"ell_hp {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in self.items()))
        bad = {k: v for k, v in self.items() if not v <= 1.0}
        assert not bad, f"{what}: error / bound above 1: {bad}"


def canon_sign_ok(axes):
    i = np.argmax(np.abs(axes), axis=0)
    return bool(np.all(axes[i, np.arange(axes.shape[1])] >= 0))


def check_eigen(r, cov, axes, axlens, canonical=True, delta_in=0.0):
    """Eigen-system of `cov` (the evaluator's own): residual, orthogonality, ascending order, ||column|| = axlen,
    canonical signs (canonical=False for LAPACK, which leaves the sign open and whose axes the oracle keeps in the
    order of the matrix they came from)."""
    d = cov.shape[0]
    c, ax, al = ld(cov), ld(axes), ld(axlens)
    r.add("eig_res", fro(c - ax @ ax.T), eig_residual_bound(cov))
    if canonical:
        assert np.all(np.diff(axlens) >= 0), "axis lengths are not ascending"
        assert canon_sign_ok(axes), "axes are not sign-canonical"
        # ||column|| = axlen: |u_k|^2 - 1 is a diagonal entry of U^T U - I, so half the orthogonality bound
        r.add("col_norm", np.max(np.abs(np.sqrt(np.sum(ax * ax, axis=0)) / al - 1)), 0.5 * orth_bound(d) + 2 * EPS)
        u = ax / al[None, :]
    else:
        u = ax / np.sqrt(np.sum(ax * ax, axis=0))[None, :]
    r.add("orth", fro(u.T @ u - np.eye(d, dtype=LD)), orth_bound(d))


def check_inverse(r, cov, am, kappa):
    d = cov.shape[0]
    r.add("inv_res", fro(ld(am) @ ld(cov) - np.eye(d, dtype=LD)), inverse_bound(d, kappa))


def check_bounding(pts, out, rec, what, canonical=True, logvol_from_spectrum=True):
    """One bounding ellipsoid of `pts` -- out: dict(ctr, cov, am, axes, axlens, logvol) -- against the fixture record
    `rec`.  Returns the Ratios (asserted by the caller through assert_ok)."""
    r = Ratios()
    n, d = pts.shape
    ctr, cov, am, axes, axlens = (np.asarray(out[k], dtype=np.float64) for k in ("ctr", "cov", "am", "axes", "axlens"))
    logvol = float(out["logvol"])
    mu, _ = cov_of_points_ld(pts)
    r.add("mean", np.max(np.abs(ld(ctr) - mu).astype(np.float64) / mean_bound(pts)), 1.0)
    b, cov_p, rho = cov_bound(pts, ctr)
    b_fro = fro(b)
    floored = "cov_out" in rec
    if floored:
        # fixture: V max(lam, floor) V^T times the reference's own rescaling; the evaluator's scale is taken from
        # the traces, and its error (sqrt(D) bound / trace) is carried
        target = ld(rec["cov_out"])
        cn = fro(target) / float(rec["fmax"] / LIM)
        delta = floored_cov_bound(d, b_fro, cn)
        mhat = float(np.trace(ld(cov)) / np.trace(target)) * float(rec["fmax"] / LIM)
        own_scale = LD(np.trace(ld(cov)) / np.trace(target))
        r.add("cov_floored", fro(ld(cov) / own_scale - target) / float(rec["fmax"] / LIM),
              delta * (1 + math.sqrt(d) * fro(target) / float(np.trace(target))))
        rho = math.sqrt(d) * delta / (float(np.trace(target)) / float(rec["fmax"] / LIM))
    else:
        # the evaluator's covariance is mult * cov; the scale is taken from the traces (relative error rho) and
        # held against the reference's fmax / (1 - 1e-3) on its own (below), so that fmax's conditioning does not
        # loosen the covariance check
        mhat = float(np.trace(ld(cov)) / np.trace(cov_p))
        err = np.abs(ld(cov) - LD(mhat) * cov_p).astype(np.float64)
        bnd = mhat * (b + rho * np.abs(cov_p).astype(np.float64)) + 2 * EPS * np.abs(cov)
        r.add("cov", np.max(err / bnd), 1.0)
        delta = b_fro + rho * fro(cov_p)
    assert bool(rec["good"]) == (not floored and int(rec["trials"]) == 0)
    # eigen-system and inverse, against the evaluator's own covariance
    check_eigen(r, cov, axes, axlens, canonical)
    lam_hat = np.sort(axlens.astype(np.float64)**2)
    kappa = float(lam_hat[-1] / lam_hat[0])
    check_inverse(r, cov, am, kappa)
    # spectrum against the fixture's (final spectrum = mult * lam; the evaluator's scale again from the traces)
    lam_ref = (lam_ld(rec) * LD(mhat) / LD(float(rec["fmax"] / LIM) if rec["fmax"] > LIM else 1.0))
    sb = spectrum_bound(cov, mhat * delta)  # delta is in the units of the unscaled covariance
    r.add("spectrum", np.max(np.abs(ld(lam_hat) - lam_ref).astype(np.float64) / (sb + 4 * EPS * lam_hat)), 1.0)
    # log-volume: against the evaluator's own axis lengths (only where ln V is computed from the eigenvalues: the
    # eigen-free root takes it from LDL^T pivots, and is held through the spectrum bound instead) ...
    pre = logvol_prefactor(d)
    own = float(LD(pre) + np.sum(np.log(ld(axlens))))
    lsb = log_spectrum_bound(spectrum_bound(cov), lam_hat)
    if logvol_from_spectrum:
        r.add("lnv_self", abs(logvol - own), logvol_self_bound(d, axlens))
    else:
        r.add("lnv_self", abs(logvol - own), logvol_self_bound(d, axlens) + 2 * lsb + 4 * d * EPS)
    # ... and against the fixture's ln V of the points, through Weyl; the scale enters as D / 2 ln(mhat / mult)
    lnv_ref = LD(rec["lnv"][0]) + LD(rec["lnv"][1]) + LD(0.5 * d) * np.log(LD(mhat) / LD(float(rec["fmax"] / LIM)))
    r.add("lnv_fix", abs(float(LD(logvol) - lnv_ref)),
          log_spectrum_bound(sb, lam_ref.astype(np.float64)) + logvol_self_bound(d, axlens) + 0.5 * d * (rho + 4 * EPS))
    # coverage: in long double with the evaluator's own precision matrix the outermost point sits at 1 - 1e-3.  The
    # evaluator divided by ITS largest form, so the distance is its quadratic-form rounding (quadform_bound over all
    # points: |max a - max b| <= max |a - b|; 4 eps for the division of am) -- a rigorous bound -- and, as the looser
    # closed form, C_INV D eps kappa.  After a floor the second pass inverts anew: the inverse's residual R enters as
    # sqrt(kappa) ||R|| (q_hat - q = w^T C^1/2 R C^-1/2 w with |w|^2 = q).
    q, sabs = quadforms_ld(pts, ctr, am)
    qmax = float(q.max())
    assert qmax < 1.0, f"{what}: a point is outside its bounding ellipsoid (q = {qmax!r})"
    if rec["fmax"] > LIM:
        qb = float(np.max(quadform_bound(d, sabs))) + 4 * EPS
        if floored:
            qb += math.sqrt(kappa) * inverse_bound(d, kappa)
        r.add("cover", abs(qmax - LIM), qb)
        r.add("cover_k", abs(qmax - LIM), qb if floored else inverse_bound(d, kappa))
    # the scale itself against the reference's fmax / (1 - 1e-3): the trace's error, the covariance error seen
    # through the smallest eigenvalue, the inverse's residual as above, the quadratic-form rounding, and the centre:
    # the evaluator's forms are taken about ITS mean mu + e, (d - e)^T A (d - e) - d^T A d = -2 e^T A d + e^T A e,
    # which for a cloud of width 1e-7 (|e| / |d| ~ 1e-9) is the largest term of all; e is measured, as in cov_bound
    if rec["fmax"] > LIM:
        e_abs = mean_error(pts, ctr, mu)
        d_own = ld(pts) - ld(ctr)
        shift = 2 * np.abs(d_own @ ld(am)) @ e_abs + e_abs @ np.abs(ld(am)) @ e_abs
        mb = rho + mhat * delta / float(lam_hat[0]) + math.sqrt(kappa) * inverse_bound(d, kappa) \
            + float(np.max(quadform_bound(d, sabs)) + np.max(shift)) / qmax
        r.add("scale", abs(mhat / float(rec["fmax"] / LIM) - 1), mb)
    return r


def check_ell_from_cov(a, axes, axlens, am, logvol, rec, canonical=True):
    r = Ratios()
    d = a.shape[0]
    check_eigen(r, a, axes, axlens, canonical)
    lam_hat = np.sort(np.asarray(axlens, dtype=np.float64)**2)
    check_inverse(r, a, am, float(lam_hat[-1] / lam_hat[0]))
    sb = spectrum_bound(a)
    lam_ref = lam_ld(rec)
    r.add("spectrum", np.max(np.abs(ld(lam_hat) - lam_ref).astype(np.float64) / (sb + 4 * EPS * lam_hat)), 1.0)
    own = float(LD(logvol_prefactor(d)) + np.sum(np.log(ld(axlens))))
    r.add("lnv_self", abs(float(logvol) - own), logvol_self_bound(d, axlens))
    r.add("lnv_fix", abs(float(LD(logvol) - LD(rec["lnv"][0]) - LD(rec["lnv"][1]))),
          log_spectrum_bound(sb, lam_ref.astype(np.float64)) + logvol_self_bound(d, axlens))
    return r


def icm_expected_cov(a, rec):
    """The covariance improve_covar_mat must return, from the fixture: the input itself, alpha A + beta I after
    blends, or the stored V max(lam, floor) V^T."""
    if "cov_out" in rec:
        return ld(rec["cov_out"])
    if "ab" in rec:
        al, be = LD(rec["ab"][0]) + LD(rec["ab"][1]), LD(rec["ab"][2]) + LD(rec["ab"][3])
        return al * ld(a) + be * np.eye(a.shape[0], dtype=LD)
    return ld(a)


def check_improve_covar_mat(a, good, cov, am, axes, rec, canonical=True):
    """`good` exact; the returned matrix against the fixture's (the input itself, bit for bit, when good; a blend's
    trial count shows in the matrix: one trial more or less changes the coefficient by a factor 1.26); eigen-system
    and inverse against the returned matrix."""
    r = Ratios()
    d = a.shape[0]
    assert bool(good) == bool(rec["good"]), f"good = {bool(good)}, the reference says {bool(rec['good'])}"
    want = icm_expected_cov(a, rec)
    if rec["good"]:
        assert np.array_equal(cov, a), "a good matrix must come back unchanged"
    elif "cov_out" in rec:
        r.add("cov_floored", fro(ld(cov) - want),
              floored_cov_bound(d, 0.0, fro(a)) + 4 * (int(rec["trials"]) + 1) * EPS * (fro(a) + math.sqrt(d)))
    else:
        # (1 - c) x + c y per entry and trial: three roundings of magnitudes <= |x| + c, and c itself from a pow()
        # that may differ by an ulp between libraries: 4 (trials + 1) eps (|A_ij| + beta delta_ij), elementwise
        bnd = 4 * (int(rec["trials"]) + 1) * EPS * (np.abs(a) + float(rec["ab"][2]) * np.eye(d))
        err = np.abs(ld(cov) - want).astype(np.float64)
        ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.where(err == 0, 0.0, np.inf))
        r.add("cov_blend", np.max(ratio), 1.0)
    ax = np.asarray(axes, dtype=np.float64)
    axlens = np.sqrt(np.sum(ld(ax) * ld(ax), axis=0)).astype(np.float64)
    c, x = ld(cov), ld(ax)
    r.add("eig_res", fro(c - x @ x.T), eig_residual_bound(cov))
    u = x / np.sqrt(np.sum(x * x, axis=0))[None, :]
    r.add("orth", fro(u.T @ u - np.eye(d, dtype=LD)), orth_bound(d))
    if canonical:
        # ascending, as far as the columns can say: the lengths here are column NORMS (improve_covar_mat returns no
        # axis lengths), each within col_norm's bound -- half the orthogonality bound -- of the square root of its
        # eigenvalue, so inside a cluster of equal eigenvalues two neighbours may stand that far the other way round
        assert np.all(np.diff(axlens) >= -(orth_bound(d) + 4 * EPS) * axlens[1:]), "axes are not in ascending order"
        assert canon_sign_ok(ax), "axes are not sign-canonical"
    lam_hat = np.sort(axlens**2)
    check_inverse(r, cov, am, float(lam_hat[-1] / lam_hat[0]))
    # the returned matrix may sit its own bound away from the fixture's, whose spectrum lam_out is
    delta = 0.0 if rec["good"] else 4 * (int(rec["trials"]) + 1) * EPS * (fro(a) + math.sqrt(d))
    if "cov_out" in rec:
        delta += floored_cov_bound(d, 0.0, fro(a))
    lam_ref = lam_ld(rec)
    r.add("spectrum", np.max(np.abs(ld(lam_hat) - lam_ref).astype(np.float64)
                             / (spectrum_bound(cov, delta) + 4 * EPS * lam_hat)), 1.0)
    return r


def decision_uncertainty(d, cnorm_over_top, b_fro_over_top=0.0):
    """How far an fp64 evaluator's lam_min / lam_max may sit from the true one: Weyl with the solver's backward error
    and the covariance error, relative to lam_max (the ratio's own denominator moves by the same amount, times a
    ratio <= 1e-11 near the threshold: inside the factor 2)."""
    return 2 * (c_eig(d) * cnorm_over_top * 2 + b_fro_over_top)


# =========================================================================================================
# the fixture, case by case (tools/make_golden.py ell_hp writes it; tests/test_ell_hp_cpu.py regenerates the small ones)
# =========================================================================================================
def case_record(key):
    """The fixture arrays of one case of tests/ell_cases.py, by its key: 'cl/D/kind[/nN]' and 'wd/D/kind' clouds,
    'mt/D/kind' matrices.  Clouds also record whether MultiEllipsoid.update keeps the root (the float64 oracle's
    verdict: which cases the multi-mode test uses, nothing numerical)."""
    import ell_cases as EC
    parts = key.split("/")
    d, kind = int(parts[1]), parts[2]
    if parts[0] == "mt":
        a = EC.matrix(kind, d)
        rec = improve_covar_mat_hp(a)
        out = fixture_record(rec)
        if EC.is_positive_kind(kind):
            with mp.workdps(DPS):
                out["lnv"] = np.array(_hilo(logvol_prefactor_mp(d) + sum(mp.log(x) for x in rec["lam_in"]) / 2))
        return out
    n = int(parts[3][1:]) if len(parts) > 3 else (6 * d if parts[0] == "wd" else None)
    pts = EC.cloud(kind, d, n)
    rec = bounding_ellipsoid_hp(pts)
    out = fixture_record(rec, cov_scale=rec["mult"])
    if parts[0] == "cl":
        from oracle import bounding_ref as B
        out["multi_ok"] = np.int32(B.multi_update(pts).nells == 1)
    return out


def all_case_keys():
    import ell_cases as EC
    keys = [c[0] for c in EC.cloud_cases()] + [c[0] for c in EC.wide_cases()]
    for d in EC.MAT_DIMS:
        keys += [k for k, _ in EC.matrix_cases(d)]
    return keys


_SCALARS = ("fmax", "good", "trials", "multi_ok")  # one number per case; NaN where a case has none
_ROWS = (("lnv", 2), ("margins", 4), ("ab", 4))  # one short row per case; NaN where a case has none


def pack_fixture(records):
    """{key: arrays} for every key of all_case_keys() -> the dozen numeric arrays tests/golden/ell_hp.npz holds, in the
    order of all_case_keys() (the keys themselves are regenerated, not stored): spectra and the upper triangles of the
    returned covariances end to end, with the dimension of every case to find them by."""
    keys = all_case_keys()
    assert sorted(keys) == sorted(records)
    g = {"dim": np.array([len(records[k]["lam_hi"]) for k in keys], dtype=np.int32)}
    g["lam_hi"] = np.concatenate([records[k]["lam_hi"] for k in keys])
    g["lam_lo"] = np.concatenate([records[k]["lam_lo"] for k in keys]).astype(np.float32)
    for name in _SCALARS:
        g[name] = np.array([float(records[k][name]) if name in records[k] else np.nan for k in keys])
    for name, width in _ROWS:
        g[name] = np.array([records[k][name] if name in records[k] else [np.nan] * width for k in keys],
                           dtype=np.float64)
    g["has_cov"] = np.array(["cov_out" in records[k] for k in keys], dtype=np.int8)
    tri = [records[k]["cov_out"][np.triu_indices(len(records[k]["lam_hi"]))] for k in keys if "cov_out" in records[k]]
    g["cov_tri"] = np.concatenate(tri) if tri else np.zeros(0)
    return g


def load_fixture(path=None):
    """{key: arrays of that case} from tests/golden/ell_hp.npz (see pack_fixture)."""
    import os
    g = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ell_hp.npz"))
    keys = all_case_keys()
    dim = g["dim"]
    assert len(dim) == len(keys), "tests/golden/ell_hp.npz does not belong to this list of cases: regenerate it"
    lam_at = np.concatenate([[0], np.cumsum(dim)])
    tri_at = np.concatenate([[0], np.cumsum(np.where(g["has_cov"] != 0, dim * (dim + 1) // 2, 0))])
    out = {}
    for i, key in enumerate(keys):
        d = int(dim[i])
        rec = {"lam_hi": g["lam_hi"][lam_at[i]:lam_at[i + 1]], "lam_lo": g["lam_lo"][lam_at[i]:lam_at[i + 1]]}
        for name in _SCALARS:
            if not np.isnan(g[name][i]):
                rec[name] = np.float64(g[name][i]) if name == "fmax" else np.int32(g[name][i])
        for name, _ in _ROWS:
            if not np.all(np.isnan(g[name][i])) or name == "margins":
                rec[name] = g[name][i]
        if g["has_cov"][i]:
            c = np.zeros((d, d))
            c[np.triu_indices(d)] = g["cov_tri"][tri_at[i]:tri_at[i + 1]]
            rec["cov_out"] = c + np.triu(c, 1).T
        out[key] = rec
    return out


def fixture_case(fix, key):
    return fix[key]


# =========================================================================================================
# membership next to the boundary (dh_contains)
# =========================================================================================================
CONTAINS_DIMS = (9, 10, 44, 45, 64)  # VALU below 10, MFMA from there, the wide form above 44
CONTAINS_KINDS = ("geo1e3", "geo1e9")
CONTAINS_RAYS = 12
_contains_cache = {}


def contains_case(d):
    """Points next to the boundary of two ellipsoids of dimension d: centre 1/2, precision matrix the long-double
    inverse (rounded to fp64, an exact datum from there on) of the kappa = 1e3 and kappa = 1e9 matrices of
    tests/ell_cases.py.  Along CONTAINS_RAYS random rays per ellipsoid, points at q = 1 +- 4 bound and 1 +- 1e-6 --
    as near to the former as the grid of fp64 points allows: moving one coordinate by an ulp moves q by
    2 |(A d)_j| ulp, which for a short axis is more than the bound, so each target is approached by a search over
    random offsets of a few ulp per coordinate and the nearest candidate that stays at least 2 bounds from the
    boundary is kept.  Returns dict(x, ctrs, ams, q (k, 2) long double, bound (k, 2), target (k,))."""
    if d in _contains_cache:
        return _contains_cache[d]
    import ell_cases as EC
    rng = np.random.default_rng(EC._seed("contains", d))
    ctrs = np.full((2, d), 0.5)
    ams = []
    for kind in CONTAINS_KINDS:
        am = ld_solve(EC.matrix(kind, d), np.eye(d)).astype(np.float64)
        ams.append(0.5 * (am + am.T))
    ams = np.array(ams)
    xs, targets = [], []
    ulp = 2.0**-53  # of a coordinate in [1/2, 1); below 1/2 the grid is finer, and a multiple of this is on it too
    for a in range(2):
        al = ld(ams[a])
        for _ in range(CONTAINS_RAYS):
            u = rng.standard_normal(d)
            u /= np.linalg.norm(u)
            t1 = float(1 / np.sqrt(ld(u) @ al @ ld(u)))  # q(t u) = 1
            for sign, off in ((1, None), (-1, None), (1, 1e-6), (-1, 1e-6)):
                base = 0.5 + t1 * u
                q0, s0 = quadforms_ld(base[None], ctrs[a], ams[a])
                b = float(quadform_bound(d, s0)[0])
                want = 1 + sign * (4 * b if off is None else off)
                base = 0.5 + t1 * math.sqrt(want / float(q0[0])) * u
                cand = base[None, :] + ulp * rng.integers(-4, 5, size=(256, d))
                cand[0] = base
                q, s = quadforms_ld(cand, ctrs[a], ams[a])
                q = (q - LD(1)).astype(np.float64)  # the distance from 1 in long double, then rounded
                ok = (np.sign(q) == sign) & (np.abs(q) >= 2 * quadform_bound(d, s))
                pick = np.flatnonzero(ok)[np.argmin(np.abs(q[ok] - (want - 1)))]
                xs.append(cand[pick])
                targets.append(want)
    x = np.array(xs)
    q = np.stack([quadforms_ld(x, ctrs[a], ams[a])[0] for a in range(2)], axis=1)
    bound = np.stack([quadform_bound(d, quadforms_ld(x, ctrs[a], ams[a])[1]) for a in range(2)], axis=1)
    out = dict(x=x, ctrs=ctrs, ams=ams, q=q, bound=bound, target=np.array(targets))
    _contains_cache[d] = out
    return out
