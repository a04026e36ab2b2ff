"""`ensemble.merge_static_runs` plus moments and resampling restated in np.longdouble (64-bit mantissa on x86): the
same formulas in a sequential order, np.logaddexp replaced by an exact-order form.  It is the reference the device
combiner's floating-point fields are held to, and it derives their bounds (`bounds`) in the way tests/hp_ref.py does:
c * 2^-53 * S with S the sum of absolute terms of the quantity and c the longest chain of roundings."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
ETA = 2.0 ** -1074  # float64's underflow quantum (the smallest subnormal)
LN2 = np.log(LD(2))

# the device scans (csrc/merge_dev.h): 8 consecutive points per thread, 256 threads per workgroup
SCAN_ITEMS, SCAN_THREADS = 8, 256


def scan_chain(M):
    """Longest chain of roundings that reaches one output of a three-launch scan over M points: the thread's own 8
    terms, 8 levels of the workgroup's scan, the carry (8 levels per 256 workgroups and one addition per further
    256), the carry's addition and the exclusive prefix's."""
    nblk = -(-M // (SCAN_ITEMS * SCAN_THREADS))
    return SCAN_ITEMS + 8 + 8 + -(-nblk // SCAN_THREADS) + 2


def moment_chain(M, cols):
    """Moment sums: one thread adds its chunk's points in order, then the chunks' sums in order."""
    n = min(-(-M // 2048), 1024, max(1, (8 << 20) // cols))
    n = max(n, 1)
    chunk = -(-M // n)
    return chunk + -(-M // chunk) + 1


def _lae(a, b):
    """ln(e^a + e^b), larger exponent first."""
    m, s = (a, b) if a >= b else (b, a)
    if s == -np.inf:
        return m
    return m + np.log1p(np.exp(s - m))


def merge_hp(dead_logl, niter, live_logl, samples=None):
    """The merged run in long double.  The ORDER is the host's (stable argsort of the float64 values: integer work);
    everything after it is long double.  samples: optional (M, D) parameters in merged order (for the moments)."""
    live_logl = np.asarray(live_logl, dtype=np.float64)
    R, N = live_logl.shape
    ls, dn = [], []
    for r in range(R):
        k = int(niter[r])
        lo = np.argsort(live_logl[r], kind="stable")
        ls.append(np.concatenate([np.asarray(dead_logl[r], dtype=np.float64)[:k], live_logl[r][lo]]))
        dn.append(np.concatenate([np.zeros(k, dtype=np.int64), -np.ones(N, dtype=np.int64)]))
    logl64 = np.concatenate(ls)
    order = np.argsort(logl64, kind="stable")
    logl64 = logl64[order]
    dn = np.concatenate(dn)[order]
    n = R * N + np.concatenate([[0], np.cumsum(dn)[:-1]])
    M = len(logl64)
    logl = logl64.astype(LD)
    nl = n.astype(LD)
    step = np.log1p(1 / nl)  # ln((n + 1) / n) without the quotient's rounding next to 1
    logvol = -np.cumsum(step)
    lpad = np.concatenate([[LD(-1.e300)], logl])
    vpad = np.concatenate([[LD(0)], logvol])
    logdvol = vpad[:-1] + np.log(-np.expm1(-step)) - LN2
    lae = np.array([_lae(lpad[i + 1], lpad[i]) for i in range(M)], dtype=LD)
    logwt = lae + logdvol
    logz = np.empty(M, dtype=LD)
    acc = LD(-np.inf)
    for i in range(M):
        acc = _lae(acc, logwt[i])
        logz[i] = acc
    lz = logz[-1]
    w0 = np.exp(lpad[:-1] - lz + logdvol)
    w1 = np.exp(lpad[1:] - lz + logdvol)
    t0 = np.where(w0 > 0, w0 * lpad[:-1], LD(0))
    t1 = np.where(w1 > 0, w1 * lpad[1:], LD(0))
    part = np.cumsum(t0 + t1)
    zfrac = np.exp(logz - lz)
    h = part - lz * zfrac
    dh = np.diff(h, prepend=LD(0))
    var = np.abs(np.cumsum(dh * step))
    w = np.exp(logwt - lz)
    w = w / np.sum(w)
    out = dict(M=M, R=R, N=N, order=order, samples_n=n, logl=logl, step=step, logvol=logvol, logdvol=logdvol, lae=lae,
               logwt=logwt, logz=logz, information=h, logzvar=var, logzerr=np.sqrt(var), weights=w, ess=1 / np.sum(w * w),
               abs_info=np.cumsum(np.abs(t0) + np.abs(t1)), zfrac=zfrac, dh=dh, lpad=lpad)
    if samples is not None:
        out.update(moments_hp(samples, w))
    return out


def moments_hp(samples, w):
    """utils.mean_and_cov in long double, with the sums of absolute terms."""
    x = np.asarray(samples).astype(LD)
    w = np.asarray(w).astype(LD)
    ws, w2 = np.sum(w), np.sum(w * w)
    mean = (w[:, None] * x).sum(axis=0) / ws
    dx = x - mean
    cov = ws / (ws * ws - w2) * np.einsum('i,ij,ik', w, dx, dx)
    return dict(mean=mean, cov=cov, abs_mean=(w[:, None] * np.abs(x)).sum(axis=0),
                abs_cov=np.einsum('i,ij,ik', w, np.abs(dx), np.abs(dx)), abs_dx=(w[:, None] * np.abs(dx)).sum(axis=0),
                norm=ws / (ws * ws - w2))


def resample_hp(samples, w, rstate):
    """utils.resample_equal with a long-double cumulative sum."""
    c = np.cumsum(np.asarray(w).astype(LD))
    c = c / c[-1]
    n = len(c)
    pos = (rstate.random() + np.arange(n)) / n
    idx = np.searchsorted(c, pos.astype(LD), side='right')
    return rstate.permutation(np.asarray(samples)[idx])


def bounds(hp):
    """Per-point absolute bounds on the device combiner's float64 fields against `hp` (float64 arrays).

    Every scan output carries at most c = scan_chain(M) roundings of partial sums, each relative to a partial sum that
    is at most S = the sum of absolute terms; the terms' own roundings come on top:
      step    = log1p(1 / n): a division, log1p (<= 1 ulp = 2u) of a 1u-relative argument          -> 4u relative
      logvol  : all terms of one sign, S = |logvol|                                            -> (c + 4) u |logvol|
      logdvol = logvol[k-1] + log(-expm1(-step)) - ln 2: the volume's bound, expm1 and log of an argument that is 4u
                relative (-> 8u absolute after the log), two additions                         -> 8u + 4u (|terms|)
      logwt   = logaddexp(l1, l0) + logdvol: logaddexp is exp, log1p, an addition              -> 4u (1 + |lae|) + ...
      logz    : the pairs' sums are sums of positive terms whose exponents carry the logwt bounds (a relative
                change of the term); per combination an exp (2u), a product and a sum          -> max logwt bound + (4c + 4) u
                and m + log s                                                                  -> + 2u |logz|
      H       : w = exp(l - lnZ + logdvol) has the relative error of its exponent's bound; S = sum |w l|; then
                - lnZ exp(logz_k - lnZ) with both ln Z's bounds
      var     : sum of dH step with dH the difference of two H's (both bounds), S = sum |dH step|
      logzerr = sqrt: |sqrt a - sqrt b| <= min(|a - b| / (2 sqrt(min)), sqrt |a - b|)
      weights : exp(logwt - lnZ) / sum: the exponent's bounds, relative

    Underflow.  The model above, fl(x) = x (1 + d) with |d| <= u, holds for results in the normal range only; a result in
    the subnormal range carries an absolute error of up to ETA = 2^-1074 instead (fl(x) = x (1 + d) + e, |e| <= ETA),
    and a bound of the form u S is itself below ETA there and rounds to 0.  The first points of a run that spans
    thousands of nats have such terms, so the fields whose terms are exp(...) of a far negative exponent get the
    absolute part as well (sums of subnormal numbers are exact and add nothing):
      H       : per point two exp (ETA each), their products with l0, l1 (the exp's ETA times |l|, and the product's
                own ETA): (2 + |l0| + |l1|) ETA, cumulative; - lnZ exp(logz_k - lnZ) likewise (|lnZ| + 1) ETA; the
                difference 1 ETA
      var     : dH carries H's bounds (already in b_h); the product dH step 1 ETA per point, and 1 for this
                bound's own product there, cumulative
      weights : the exp and the quotient by a sum next to 1: 2 ETA each at most
    """
    M = hp["M"]
    c = scan_chain(M)
    f = lambda k: np.asarray(hp[k], dtype=np.float64)  # noqa: E731
    logvol, logdvol, lae, logwt, logz, h = f("logvol"), f("logdvol"), f("lae"), f("logwt"), f("logz"), f("information")
    step, logl, zfrac, var = f("step"), f("logl"), f("zfrac"), f("logzvar")
    b_vol = (c + 4) * U * np.abs(logvol)
    v0 = np.concatenate([[0.], logvol[:-1]])
    b_v0 = np.concatenate([[0.], b_vol[:-1]])
    lterm = logdvol - v0 + np.log(2.)
    b_ldv = b_v0 + 8 * U + 4 * U * (np.abs(v0) + np.abs(lterm) + np.log(2.) + np.abs(logdvol))
    b_wt = b_ldv + 4 * U * (1 + np.abs(lae)) + 2 * U * (np.abs(lae) + np.abs(logdvol) + np.abs(logwt))
    b_z = np.maximum.accumulate(b_wt) + (4 * c + 4) * U + 2 * U * np.abs(logz)
    lz, b_lz = logz[-1], b_z[-1]
    l0 = np.concatenate([[0.], logl[:-1]])  # (the first point's l0 = -1e300 has weight 0)
    d_exp = b_lz + b_ldv + 2 * U * (np.abs(logl) + np.abs(l0) + abs(lz) + np.abs(logdvol)) + 2 * U
    abs_terms = np.diff(f("abs_info"), prepend=0.)
    b_part = np.cumsum(abs_terms * (d_exp + (c + 4) * U))
    b_h = b_part + (abs(lz) * (b_z + b_lz + 6 * U + 2 * U * (np.abs(logz) + abs(lz))) + b_lz) * zfrac \
        + 2 * U * (f("abs_info") + abs(lz) * zfrac) \
        + ETA * (np.cumsum(2 + np.abs(l0) + np.abs(logl)) + abs(lz) + 2)
    b_hm = np.concatenate([[0.], b_h[:-1]])
    dh = f("dh")
    b_var = np.cumsum((b_h + b_hm) * step + np.abs(dh * step) * (c + 8) * U + 2 * ETA)
    err = np.sqrt(var)
    with np.errstate(divide='ignore', invalid='ignore'):
        lin = b_var / (2 * np.sqrt(np.maximum(var - b_var, 0.)))
    b_err = np.minimum(np.where(np.isfinite(lin), lin, np.inf), np.sqrt(b_var)) + 2 * U * err
    w = f("weights")
    rel_w = 2 * (b_wt + b_lz + (c + 8) * U + 2 * U * (np.abs(logwt) + abs(lz)))
    return dict(logvol=b_vol, logwt=b_wt, logz=b_z, information=b_h, logzerr=b_err, weights=w * rel_w + 4 * ETA, rel_w=rel_w)


def moment_bounds(hp, rel_w):
    """Bounds on mean and covariance: every weight carries rel_w (relative), a sum of `moment_chain` roundings over
    S = sum w |x| (mean) or sum w |dx_i dx_j| (covariance), whose factors carry the mean's bound; the normalisations
    1 / sum w and sum w / ((sum w)^2 - sum w^2) a few roundings each."""
    M = hp["M"]
    D = len(hp["mean"])
    f = lambda k: np.asarray(hp[k], dtype=np.float64)  # noqa: E731
    rw = float(np.max(rel_w))
    c1, c2 = moment_chain(M, D + 2), moment_chain(M, D * D)
    b_mean = f("abs_mean") * (2 * rw + (c1 + 4) * U)
    adx = f("abs_dx")
    b_cov = f("norm") * (f("abs_cov") * (2 * rw + (c2 + 8) * U) + np.outer(adx, b_mean) + np.outer(b_mean, adx)
                         + np.outer(b_mean, b_mean)) + np.abs(f("cov")) * (4 * rw + (c1 + 8) * U)
    return b_mean, b_cov
