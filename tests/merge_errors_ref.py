"""One realization of a merged run's prior volumes (dynesty_amd/errors.py, csrc/merge_errors.hip's me_* kernels) restated in
np.longdouble (64-bit mantissa on x86), and the bounds its float64 evaluations are held to -- derived as
tests/merge_hp_ref.py derives the combiner's: c * 2^-53 * S with S the sum of absolute terms and c the longest chain of
roundings.  The words are tests/philox_ref.py's, not the package's.

Allowance per transcendental: 1 ulp = 2u (u = 2^-53), the figure tests/merge_hp_ref.py uses for the same functions.  No
accuracy statement for the device's math library is at hand, so the figure is calibrated on a float64 evaluator that
is not the device's -- `calibrate()`: NumPy's log, log1p, expm1 and exp against long double over the ranges a
realization puts them to (tests/test_merge_errors_cpu.py asserts <= 1 ulp there) -- never on device output.

Chains.  `device_chains(M)`: the three-launch scan of merge_hp_ref.scan_chain (ln X, the cumulative ln Z of the
per-point path) and the batch sums: a thread's 8 terms, 8 levels of the workgroup, the chunks one after another; the
mean sums a thread's 256 points, 8 segments, the chunks.  `host_chains(M)`: np.cumsum adds in sequence and BLAS may,
M roundings.
"""
import math

import numpy as np

import philox_ref
from merge_hp_ref import ETA, LD, LN2, SCAN_ITEMS, SCAN_THREADS, U, scan_chain


def device_chains(M):
    nblk = -(-M // (SCAN_ITEMS * SCAN_THREADS))
    return dict(scan=scan_chain(M), sums=SCAN_THREADS + 8 + 8 + nblk + 4)


def host_chains(M):
    return dict(scan=M + 16, sums=M + 16)


def calibrate(n=200000, seed=11):
    """Largest error in ulps of NumPy's float64 log / log1p / expm1 / exp against long double on the arguments of a
    realization: log of uniforms in (0, 1], log1p(1 / n), expm1 and log(-expm1) of steps, exp of differences <= 0."""
    rng = np.random.default_rng(seed)
    u = 1.0 - rng.random(n)
    s = np.log(u) / rng.integers(1, 5000, n)
    d = -rng.random(n) * 40.0
    out = {}
    for name, f, x in (("log", np.log, u), ("log1p", np.log1p, 1.0 / rng.integers(1, 5000, n)), ("expm1", np.expm1, s),
                       ("log_of_expm1", np.log, -np.expm1(s)), ("exp", np.exp, d)):
        got, want = f(x), f(x.astype(LD))
        out[name] = float(np.max(np.abs(got.astype(LD) - want) / np.spacing(np.abs(got))))
    return out


def uniforms(seed, real, M):
    """u_k of realization `real`: words 2k and 2k + 1 of subsequence `real` (tests/philox_ref.py)."""
    w = philox_ref.words(int(seed), [int(real)], 0, 2 * M)[0]
    return philox_ref.uniform_double(w[0::2], w[1::2])


def steps64(seed, real, samples_n, jitter=True):
    """The steps as float64 numbers (NumPy): what math.fsum adds exactly for the ln X checks."""
    n = np.asarray(samples_n, dtype=np.float64)
    return np.log(uniforms(seed, real, len(n))) / n if jitter else -np.log1p(1.0 / n)


def realization_hp(logl, samples_n, seed, real, jitter=True, logrwt=None, samples=None):
    """Everything of one realization in long double."""
    logl = np.asarray(logl, dtype=np.float64).astype(LD)
    M = len(logl)
    n = np.asarray(samples_n).astype(LD)
    s = np.log(uniforms(seed, real, M).astype(LD)) / n if jitter else -np.log1p(1 / n)
    logvol = np.cumsum(s)
    v0 = np.concatenate([[LD(0)], logvol[:-1]])
    with np.errstate(divide="ignore"):
        lterm = np.log(-np.expm1(s))
    logdvol = v0 + lterm - LN2
    l0 = np.concatenate([[LD(-1.e300)], logl[:-1]])
    hi, lo = np.maximum(logl, l0), np.minimum(logl, l0)
    lae = hi + np.log1p(np.exp(lo - hi))
    rw = np.zeros(M, dtype=LD) if logrwt is None else np.asarray(logrwt, dtype=np.float64).astype(LD)
    logwt = lae + logdvol + rw
    logz = np.logaddexp.accumulate(logwt)
    assert logz.dtype == LD
    lz = logz[-1]
    w0, w1 = np.exp(l0 - lz + logdvol), np.exp(logl - lz + logdvol)
    t0, t1 = np.where(w0 > 0, w0 * l0, LD(0)), np.where(w1 > 0, w1 * logl, LD(0))
    w = np.exp(logwt - lz)
    sw, sw2 = np.sum(w), np.sum(w * w)
    out = dict(M=M, step=s, logvol=logvol, v0=v0, lterm=lterm, logdvol=logdvol, lae=lae, rw=rw, logwt=logwt, logz=logz,
               logl=logl, l0=l0, information=np.sum(t0 + t1) - lz, abs_info=np.sum(np.abs(t0) + np.abs(t1)),
               w=w / sw, ess=sw * sw / sw2)
    if samples is not None:
        x = np.asarray(samples, dtype=np.float64).astype(LD)
        out["mean"] = (out["w"][:, None] * x).sum(axis=0)
        out["abs_mean"] = (out["w"][:, None] * np.abs(x)).sum(axis=0)
        out["abs_x"] = np.abs(np.asarray(samples, dtype=np.float64))
    return out


def bounds(hp, chains):
    """Absolute bounds on a float64 evaluation with the chains `chains` against `hp`.

      step    = log(u) / n (u exact): log 2u, division 1u; -log1p(1 / n): division, log1p of a 1u-relative argument
                                                                                                    -> 4u relative
      logvol  : terms of one sign, S = |logvol|                                                -> (c + 4) u |logvol|
      logdvol = logvol[k-1] + log(-expm1(s)) - ln 2: expm1 of a 4u-relative argument (|x e^x / (e^x - 1)| <= 1: 4u
                relative) + 2u, the log of that 8u absolute after its own 2u relative, two additions
                                                                  -> b_vol[k-1] + 8u + 4u (|terms|), merge_hp_ref's
      logwt   = logaddexp + logdvol (+ logrwt): merge_hp_ref's, and the further addition 2u (|logrwt| + |logwt|)
      logz_k  (cumulative, the per-point path's scan): merge_hp_ref's max b_wt + (4c + 4) u + 2u |logz|
      ln Z    (batch): m + log(sum exp(lw_k - m)) with the sums rescaled from the chunk's largest term to the largest
                chunk's: term k has the relative error r_k = b_wt[k] + u (|lw_k - top| + 8) (its exponent's bound, the
                subtractions' roundings -- |lw - m_c| + |m_c - top| = |lw - top| --, the two exp and a product), the sum
                (c_s + 4) u more; the log 2u and the last addition                -> sum w_k r_k + (c_s + 6) u + 2u |ln Z|
      H       : term k = w0 l0 + w1 l1, w = exp(l - ref + logdvol) scaled to ln Z: relative error of its exponent
                d_k = b_lnZ + b_ldv[k] + 2u (|l| + |l0| + |ln Z| + |logdvol|) + 2u |l + logdvol - ln Z| + 8u;
                S = sum |terms|, (c_s + 6) u for the sums and scalings, then - ln Z; terms that underflow carry ETA
                absolute instead (merge_hp_ref): (2 + |l0| + |l|) ETA per point
      ESS     = (sum w)^2 / sum w^2: both sums with the r_k (twice in w^2) and their chains
      mean_c  = sum w v_c / sum w: S = sum w |v_c|, r_k and the chain; the normalisation with sum w's own error
    """
    M = hp["M"]
    cs, cm = chains["scan"], chains["sums"]
    f = lambda k: np.asarray(hp[k], dtype=np.float64)  # noqa: E731
    logvol, v0, lterm, ldv, lae, rw, logwt, logz = (f(k) for k in ("logvol", "v0", "lterm", "logdvol", "lae", "rw", "logwt", "logz"))
    logl, l0, w = f("logl"), f("l0"), f("w")
    l0[0] = 0.0  # (the first point's l0 = -1e300 has weight 0)
    lz = float(hp["logz"][-1])
    fin = np.isfinite(ldv)  # (a step of exactly 0 has ln dX = -inf: held to equality, not to a bound)
    z = lambda a: np.where(fin, a, 0.0)  # noqa: E731
    b_vol = (cs + 4) * U * np.abs(logvol)
    b_v0 = np.concatenate([[0.], b_vol[:-1]])
    b_ldv = b_v0 + 8 * U + 4 * U * (np.abs(v0) + z(np.abs(lterm)) + np.log(2.) + z(np.abs(ldv)))
    b_wt = b_ldv + 4 * U * (1 + np.abs(lae)) + 2 * U * (np.abs(lae) + z(np.abs(ldv)) + z(np.abs(lae + ldv))) \
        + 2 * U * (np.abs(rw) + z(np.abs(logwt)))
    b_wt = np.where(np.isfinite(logwt), b_wt, 0.0)
    b_z = np.maximum.accumulate(b_wt) + (4 * cs + 4) * U + 2 * U * np.abs(logz)
    top = np.max(logwt)
    with np.errstate(invalid="ignore"):
        r = np.where(w > 0, b_wt + U * (np.abs(logwt - top) + 8), 0.0)
    b_lz = float(np.sum(w * r)) + (cm + 6) * U + 2 * U * abs(lz)
    with np.errstate(invalid="ignore"):
        d = b_lz + b_ldv + 2 * U * (np.abs(logl) + np.abs(l0) + abs(lz) + z(np.abs(ldv))) \
            + 2 * U * z(np.abs(logl + ldv - lz)) + 8 * U
    absi = float(hp["abs_info"])
    w0, w1 = np.exp(z(l0 - lz + ldv)) * fin, np.exp(z(logl - lz + ldv)) * fin
    terms = w0 * np.abs(l0) + w1 * np.abs(logl)
    b_h = float(np.sum(terms * d)) + (cm + 6) * U * absi + b_lz + 2 * U * (absi + abs(lz)) \
        + ETA * float(np.sum(2 + np.abs(l0) + np.abs(logl)))
    ess = float(hp["ess"])
    r_s = float(np.sum(w * r)) + (cm + 4) * U
    w2 = w * w
    r_s2 = float(np.sum(w2 / np.sum(w2) * 2 * r)) + (cm + 6) * U
    out = dict(logvol=b_vol, logwt=b_wt, logz=b_z, logz_last=b_lz, information=b_h, ess=ess * (2 * r_s + r_s2 + 4 * U))
    if "mean" in hp:
        mean, am = f("mean"), f("abs_mean")
        x_r = (w * r) @ hp["abs_x"]
        out["mean"] = x_r + am * (cm + 4) * U + np.abs(mean) * (r_s + 2 * U)
    return out


def fsum_logvol(s64, ks):
    """ln X at the points `ks`: the exact sum of the float64 steps, rounded once."""
    return np.array([math.fsum(s64[:k + 1]) for k in ks])


def check(got, want, bound, label):
    """|got - want| <= bound wherever `want` is finite, equality elsewhere; returns the worst error / bound."""
    got, want, bound = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (got, want, bound))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin]), label
    err = np.abs(got[fin] - want[fin])
    ok = err <= bound[fin]
    worst = float(np.max(err / np.maximum(bound[fin], 1e-300))) if err.size else 0.0
    print(f"[merge errors {label}] worst error / bound = {worst:.3g} (max error {err.max() if err.size else 0:.3g})")
    assert ok.all(), (label, int(np.argmin(ok)), float(err[np.argmin(ok)]), float(bound[fin][np.argmin(ok)]))
    return worst
