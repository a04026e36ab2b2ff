"""The static run loop's evidence integration (the reference's progress_integration recurrence and its final
compute_integrals) restated in np.longdouble (64-bit mantissa on x86) in sequential order with an exact-order
logaddexp, as tests/merge_hp_ref.py does for the merge -- the reference that ln Z, H and var ln Z of csrc/ns.hip
(ns_consume phase B, ns_finish) are held to -- and the bounds of a float64 evaluation against it.  `*_mp` are the same
formulas in mpmath at 50 digits: tools/make_golden.py ns_hp writes them to tests/golden/ns_hp.npz, and the tests hold
the long-double functions to that file; no mpmath runs in a test.

Which point dies in which slot, and which -d ln X it takes, is integer work and the oracle's (oracle/nested_ref.py);
the steps enter here as the float64 numbers the oracle recorded.

Bounds.  u = 2^-53.  The base form is c u S, S the sum of absolute terms of the quantity and c the longest chain of
roundings in the device's order (csrc/ns.hip): a lane adds its EPT = ceil(K / 256) deaths in order, a 64-lane scan
(6 levels), up to 3 wave totals, the incoming value and the lane's own prefix: c = EPT + 12 per fill (`chain`).
log, log1p, exp and expm1 are granted 1 ulp = 2u each, the allowance of tests/merge_hp_ref.py.  On top of it comes
what the base form does not cover, the rounding of every exponent's argument: a weight is exp(L - lnZ + ln dX), and
its argument carries lnZ's and ln dX's own bounds plus 2u (|L| + |lnZ| + |ln dX|) of absolute error from the two
additions, which is a RELATIVE error of the weight.  In H the weight multiplies L, and sum |w L| is about |L| itself:
so H's bound grows like L^2 u -- with every log-likelihood near 1e6 it is about 1e6 * 2e6 * 3 * 1.1e-16 = 7e-4 and not
the 1e-9 that c u S alone would give; ln Z's stays linear in |L| (a few u |L|: 1e-9 at 1e6).

Per death k (1-based over the whole chain of fills; lv = ln X, s = -d ln X, L_0 = the incoming last dead value):
  lv      per fill two roundings (lv_0 - (e + 1) s), or with plateau steps the scan: (c + 2) u |lv| per fill; a
          plateau step, which the device forms as -log1p(-1 / (N + 2 - j)) and the oracle as
          -log1p(-exp(plogdvol - lv)), may differ from the recorded one by tau = 2u (|lv| + |plogdvol|) + 8u relative
  ldv     = lv + log(expm1(s) / 2): b_lv + tau + 2u (expm1) + 2u |log| + u |ldv|
  lw      = logaddexp(L_k, L_k-1) + ldv: b_ldv + 5u + u |lae| + u |lw|
  lnZ     the weights are positive, so the sum's relative error is the weighted mean of the terms' exponent errors
          eps_j = b_lw_j + u |lw_j - M| + 2u (M: the fill's reference point, its largest weight or the incoming lnZ);
          a fill adds (c + 2) u for its sum, 2u |lnZ - M| for its log and u |lnZ| for the last addition
  H       g = H + lnZ = sum of the terms T_k = w_k-1 L_k-1 + w_k L_k relative to Z:
          b_g = sum |T_k| (b_z + b_ldv_k + 2u (|L_k| + |lnZ| + |ldv_k|) + 3u + (c + 1) u) + the carried part
          Z_0/Z (b_h0 + b_z0 + u |g_0|) + |Z_0/Z g_0| (b_z0 + b_z + u |lnZ_0 - lnZ| + 4u), + u |g|;
          b_h = b_g + b_z + u |H|; an H taken inside the fill (the plateau deaths') is rescaled from the fill's end:
          + |g| (b_z(end) + b_z + u |lnZ_end - lnZ| + 3u)
  var     = sum dH s: over the constant step it telescopes, (b_h(end) + b_h(start)) s + 4u |dH s| per fill; every
          plateau death adds (b_h(e) + b_h(e - 1)) |s_e - s| + |dH_e| (tau s_e + 4u |s_e - s|), their sum's chain
          c u sum |dH_e (s_e - s)|, and 2u |var| per fill
  plogdvol = lv - log1p(-j / (N + 1)) - ln(N + 1): b_lv + 3u (|log1p| + ln(N + 1)) + 2u |plogdvol|
  dz      = logaddexp(0, Lmax + lv - lnZ): b_lv + b_z + u (|Lmax + lv| + |Lmax + lv - lnZ|) + 5u
An argument's error x is a relative error e^x - 1 of the weight (`_rel`), which matters where |L| u is not small: with a
floor at -1e30 the plateau deaths' ln Z_e = -1e30 + ln dX cannot hold ln dX at all (u |lnZ| = 1e14), H_e and with it
var ln Z are beyond float64 in ANY order -- the oracle's included -- and the bound says so by being about 1e300.
Underflow: an exp below the normal range is off by ETA = 2^-1074 absolutely; the terms carry it times |L| + 1.

`order="serial"` gives the bounds of the recurrence run death by death (the oracle's order): the sums' chains are the
number of deaths so far, var takes every death's own dH, and ln dX is the reference's difference of exponentials.  The bounds are of first order in u."""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0**-60, "np.longdouble is not an extended type here: do the arithmetic in mpmath"
U = 2.0 ** -53
ETA = 2.0 ** -1074
ULP = 2 * U  # what log, log1p, exp and expm1 are granted (tests/merge_hp_ref.py: "log1p (<= 1 ulp = 2u)", "an exp (2u)")
kT = 256
UNDER = 600.0  # csrc/ns.hip kNsUnder: how far below a fill's M a plateau death's ln Z_e may lie for the scan form

QUANT = ("logvol", "logz", "h", "logzvar")


def chain(K):
    """Longest chain of roundings of one of phase B's sums over a fill of K entries."""
    return -(-K // kT) + 6 + 3 + 3


def _lae(a, b):
    """ln(e^a + e^b), larger exponent first."""
    m, s = (a, b) if a >= b else (b, a)
    if s == -np.inf:
        return m
    return m + np.log1p(np.exp(s - m))


def integrate_hp(dead, steps, state0):
    """The recurrence over a chain of deaths.  dead, steps: float64 arrays (death values, -d ln X of every death);
    state0 = (logvol, logz, h, logzvar, last dead value).  Returns long-double arrays of the state after every death
    (logvol, logz, h, logzvar) and the pieces the bounds need (ldv, lae, lw, dh)."""
    n = len(dead)
    lv, lz, h, var, lprev = (LD(x) for x in state0)
    out = {k: np.empty(n, dtype=LD) for k in ("logvol", "logz", "h", "logzvar", "ldv", "lae", "lw", "dh")}
    half = LD(0.5)
    for k in range(n):
        lnew, s = LD(dead[k]), LD(steps[k])
        lv = lv - s
        ldv = lv + np.log(half * np.expm1(s))
        a = _lae(lnew, lprev)
        lw = a + ldv
        lzn = _lae(lz, lw)
        t0, t1 = np.exp(lprev - lzn + ldv), np.exp(lnew - lzn + ldv)
        lzterm = (t0 * lprev if t0 > 0 else LD(0)) + (t1 * lnew if t1 > 0 else LD(0))
        w = np.exp(lz - lzn)
        hn = lzterm + (w * (h + lz) if w > 0 else LD(0)) - lzn
        var = var + (hn - h) * s
        out["dh"][k] = hn - h
        h, lz, lprev = hn, lzn, lnew
        for key, v in (("logvol", lv), ("logz", lz), ("h", h), ("logzvar", var), ("ldv", ldv), ("lae", a), ("lw", lw)):
            out[key][k] = v
    return out


def integrate_mp(dead, steps, state0, ends):
    """integrate_hp in mpmath (50 digits); returns the (logvol, logz, h, logzvar) rows at the 1-based death counts
    `ends` as strings-free float128-safe pairs: (hi, lo) float64 with hi + lo the value to 1e-32 relative."""
    import mpmath as mp
    mp.mp.dps = 50
    lv, lz, h, var, lprev = (mp.mpf(float(x)) for x in state0)

    def lae(a, b):
        m, s = (a, b) if a >= b else (b, a)
        return m + mp.log1p(mp.exp(s - m))

    rows = []
    ends = list(ends)
    for k in range(len(dead)):
        lnew, s = mp.mpf(float(dead[k])), mp.mpf(float(steps[k]))
        lv -= s
        ldv = lv + mp.log(mp.expm1(s) / 2)
        lw = lae(lnew, lprev) + ldv
        lzn = lae(lz, lw)
        hn = mp.exp(lprev - lzn + ldv) * lprev + mp.exp(lnew - lzn + ldv) * lnew + mp.exp(lz - lzn) * (h + lz) - lzn
        var += (hn - h) * s
        h, lz, lprev = hn, lzn, lnew
        if k + 1 in ends:
            rows.append([split(x) for x in (lv, lz, h, var)])
    return np.array(rows)  # (len(ends), 4, 2)


def split(x):
    """An mpmath number as (hi, lo) float64."""
    hi = float(x)
    return hi, float(x - hi)


def join(pair):
    return LD(pair[..., 0]) + LD(pair[..., 1])


def _wsum(logterm, lz):
    """sum_{j <= k} exp(logterm_j - lz_k) for every k (float64, log domain: no term overflows)."""
    if len(logterm) == 0:
        return np.zeros(0)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(np.logaddexp.accumulate(logterm) - lz)


def _rel(x):
    """The relative error of exp(a) whose argument is off by x: e^x - 1 (x itself while x is small; capped short of
    overflow -- a bound of that size says that float64 cannot know the quantity)."""
    return np.expm1(np.minimum(x, 700.0))


def _log(x):
    with np.errstate(divide="ignore"):
        return np.log(x)


def consume_bounds(hp, dead, steps, state0, fill_ends, K, nlive, order="device", plateau_pl=None):
    """Per-death absolute bounds (float64 arrays: logvol, logz, h, logzvar, and dz_extra = what dz adds to
    b_lv + b_z apart from the Lmax term) of a float64 evaluation of the chain against `hp` = integrate_hp(...).
    fill_ends: the 1-based death counts at which the fills end (increasing).  plateau_pl: per death the plateau's
    ln volume step (plogdvol) or nan for a death that took the constant step."""
    n = len(dead)
    f64 = lambda k: np.asarray(hp[k], dtype=np.float64)  # noqa: E731
    lv, lz, h, var, ldv, lae, lw, dh = (f64(k) for k in ("logvol", "logz", "h", "logzvar", "ldv", "lae", "lw", "dh"))
    dead = np.asarray(dead, dtype=np.float64)
    steps = np.asarray(steps, dtype=np.float64)
    lv0, lz0, h0, var0, lprev0 = (float(x) for x in state0)
    dlv = math.log((nlive + 1.0) / nlive)
    isp = np.zeros(n, bool) if plateau_pl is None else np.isfinite(plateau_pl)
    c1 = chain(K)
    idx = np.arange(1, n + 1)
    fill_of = np.searchsorted(np.asarray(fill_ends), idx, side="left")  # 0-based fill of every death
    nf = fill_of + 1.0
    cs = idx.astype(np.float64) if order == "serial" else np.full(n, float(c1))  # a sum's chain inside a fill
    # --- ln X
    lvprev = np.concatenate([[lv0], lv[:-1]])
    tau = np.where(isp, 2 * U * (np.abs(lvprev) + np.abs(np.where(isp, plateau_pl, 0.0))) + 4 * ULP, 0.0) \
        if plateau_pl is not None else np.zeros(n)
    b_lv = (idx * U if order == "serial" else nf * (c1 + 2) * U) * np.maximum(np.abs(lv), abs(lv0)) + np.cumsum(tau * steps)
    # --- ln dX, ln w
    lc = ldv - lv
    b_ldv = b_lv + tau + ULP + ULP * np.abs(lc) + U * np.abs(ldv)
    if order == "serial":
        # the reference forms ln dX as logsumexp([lv + s, lv], [0.5, -0.5]), a difference of two exponentials that
        # agree in all but s of their value: their roundings (2u each, u |lv + s| in the argument) come back divided
        # by 1 - e^-s, which is what limits the recurrence at nlive = 40 000 (s = 2.5e-5)
        b_ldv = b_ldv + (6 * U + 2 * U * (np.abs(lv) + steps)) / -np.expm1(-steps)
    b_lw = b_ldv + 5 * U + U * np.abs(lae) + U * np.abs(lw)
    # --- ln Z
    b_z = np.empty(n)
    carry = 0.0
    Mref = np.empty(n)
    start = 0
    fe = sorted(set(int(e) for e in fill_ends if e > 0))  # (a fill without a death leaves the state as it is)
    for e in fe:
        sl = slice(start, e)
        Mref[sl] = max(lw[sl].max(), lz0 if start == 0 else lz[start - 1])
        start = e
    eps = b_lw + U * np.abs(lw - Mref) + ULP
    werr = _wsum(lw + _log(eps), lz)
    start = 0
    for e in fe:
        sl = slice(start, e)
        own = (cs[sl] + 2) * U + ULP * np.abs(lz[sl] - Mref[sl]) + U * np.abs(lz[sl])
        b_z[sl] = werr[sl] + carry + own + n * ETA
        carry += own[-1] if order != "serial" else 0.0
        start = e
    if order == "serial":  # every death is a logaddexp of its own
        b_z = werr + (7 * U + U * np.abs(lz)) * idx + n * ETA
    # --- H: terms relative to Z_k, in the log domain
    Lp = np.concatenate([[lprev0], dead[:-1]])
    with np.errstate(divide="ignore"):
        lt0, lt1 = Lp + ldv + np.log(np.abs(Lp)), dead + ldv + np.log(np.abs(dead))
    lt0 = np.where(Lp < -1e299, -np.inf, lt0)  # the first death's L_0 = -1e300 has weight 0
    alpha0 = _rel(b_ldv + 2 * U * (np.abs(Lp) + np.abs(ldv)) + 3 * U + (cs + 1) * U)
    alpha1 = _rel(b_ldv + 2 * U * (np.abs(dead) + np.abs(ldv)) + 3 * U + (cs + 1) * U)
    b_h = np.empty(n)
    b_hin = np.empty(n)  # an H taken inside a fill
    g = h + lz
    B0, bz0, g0, lzs = 0.0, 0.0, h0 + lz0, lz0  # the state a fill starts from
    start = 0
    for e in fe:
        sl = slice(start, e)
        with np.errstate(under="ignore", over="ignore"):
            w = np.exp(lzs - lz[sl]) if lzs > -1e299 else np.zeros(e - start)
        old = np.seterr(over="ignore", invalid="ignore")  # (bounds beyond the range are inf: see _rel)
        absT = _wsum(np.logaddexp(lt0[sl], lt1[sl]), lz[sl])
        aT = _wsum(np.logaddexp(lt0[sl] + _log(alpha0[sl]), lt1[sl] + _log(alpha1[sl])), lz[sl])
        under = ETA * np.cumsum(2 + np.abs(Lp[sl]) + np.abs(dead[sl]))
        bg = aT + absT * _rel(b_z[sl] + 2 * U * np.abs(lz[sl])) + under + U * np.abs(g[sl])
        if lzs > -1e299:
            bg = bg + w * (B0 + bz0 + U * abs(g0)) + np.abs(w * g0) * _rel(bz0 + b_z[sl] + U * np.abs(lzs - lz[sl]) + 4 * U)
        b_h[sl] = bg + b_z[sl] + U * np.abs(h[sl])
        zE, bzE = lz[e - 1], b_z[e - 1]
        b_hin[sl] = b_h[sl] + np.abs(g[sl]) * _rel(bzE + b_z[sl] + U * np.abs(zE - lz[sl]) + 3 * U)
        b_hin[e - 1] = b_h[e - 1]
        np.seterr(**old)
        b_h[sl] = np.where(np.isnan(b_h[sl]), np.inf, b_h[sl])
        b_hin[sl] = np.where(np.isnan(b_hin[sl]), np.inf, b_hin[sl])
        B0, bz0, g0, lzs = b_h[e - 1], b_z[e - 1], g[e - 1], lz[e - 1]
        start = e
    # --- var ln Z
    b_var = np.empty(n)
    if order == "serial":
        bhp = np.concatenate([[0.0], b_h[:-1]])
        b_var = np.cumsum((b_h + bhp) * steps + 4 * U * np.abs(dh * steps)) + idx * U * np.maximum.accumulate(np.abs(var))
    else:
        acc, start, hs, bhs = 0.0, 0, h0, 0.0
        for e in fe:
            sl = slice(start, e)
            delta = np.where(isp[sl], steps[sl] - dlv, 0.0)
            bprev = np.concatenate([[bhs], b_hin[start:e - 1]])
            with np.errstate(over="ignore", invalid="ignore"):
                pl = (b_hin[sl] + bprev) * np.abs(delta) + np.abs(dh[sl]) * (tau[sl] * steps[sl] + 4 * U * np.abs(delta)) \
                    + c1 * U * np.abs(dh[sl] * delta)
            pl = np.where(np.isnan(pl), np.inf, pl)  # (a bound beyond the range times a step of 0: no bound)
            # inside the fill: the telescoped part up to the death in question
            tel = (b_h[sl] + bhs) * dlv + 4 * U * np.abs((h[sl] - hs) * dlv)
            b_var[sl] = acc + tel + np.cumsum(pl) + 2 * U * np.abs(var[sl]) + 2 * U * abs(var0)
            acc, hs, bhs = b_var[e - 1], h[e - 1], b_h[e - 1]
            start = e
    return dict(logvol=b_lv, logz=b_z, h=b_h, logzvar=b_var)


def dz_bound(b, k, lmax, lv, lz):
    """Bound on the stopping rule's dz after death k (0-based) given the bounds `b` of consume_bounds."""
    x = lmax + lv
    return b["logvol"][k] + b["logz"][k] + U * (abs(x) + abs(x - lz)) + 5 * U


def plogdvol_hp(lv_start, nlive):
    """ln of a plateau's volume step: ln X at its start - ln(N + 1)."""
    return LD(lv_start) - np.log(LD(nlive) + 1)


def plogdvol_bound(b_lv, j, nlive, pl):
    return b_lv + 3 * U * (abs(math.log1p(-j / (nlive + 1.0))) + math.log(nlive + 1.0)) + 2 * U * abs(pl)


# ---------------------------------------------------------------------------------------------------------------------
# what ns_finish reports: compute_integrals over dead + sorted live values with given volumes
# ---------------------------------------------------------------------------------------------------------------------
def integrals_hp(logl, logvol):
    """ref: utils.py:1411-1467 (reweight=None) in long double, sequential.  logl, logvol: float64 arrays (dead points in
    death order then the final live points ascending; ln X of each).  Returns the final (logz, logzvar, h) and the
    sums of absolute terms the bound needs."""
    logl = np.asarray(logl, dtype=np.float64).astype(LD)
    lv = np.asarray(logvol, dtype=np.float64).astype(LD)
    n = len(logl)
    lpad = np.concatenate([[LD(-1.e300)], logl])
    vpad = np.concatenate([[LD(0)], lv])
    step = vpad[:-1] - vpad[1:]
    ldv = vpad[:-1] + np.log(-np.expm1(-step)) - np.log(LD(2))
    lw = np.array([_lae(lpad[i + 1], lpad[i]) for i in range(n)], dtype=LD) + ldv
    lz = np.empty(n, dtype=LD)
    acc = LD(-np.inf)
    for i in range(n):
        acc = _lae(acc, lw[i])
        lz[i] = acc
    lzf = lz[-1]
    w0, w1 = np.exp(lpad[:-1] - lzf + ldv), np.exp(lpad[1:] - lzf + ldv)
    t0 = np.where(w0 > 0, w0 * lpad[:-1], LD(0))
    t1 = np.where(w1 > 0, w1 * lpad[1:], LD(0))
    part = np.cumsum(t0 + t1)
    zfrac = np.exp(lz - lzf)
    hh = part - lzf * zfrac
    dh = np.diff(hh, prepend=LD(0))
    var = np.abs(np.cumsum(dh * step))
    return dict(logz=lzf, logzvar=var[-1], h=hh[-1], lz=lz, hh=hh, dh=dh, step=step, ldv=ldv, lw=lw,
                absT=np.cumsum(np.abs(t0) + np.abs(t1)), zfrac=zfrac, lpad=lpad, n=n)


def integrals_mp(logl, logvol):
    """integrals_hp in mpmath (50 digits): (logz, logzvar, h) as (hi, lo) pairs."""
    import mpmath as mp
    mp.mp.dps = 50
    L = [mp.mpf(-1.e300)] + [mp.mpf(float(x)) for x in logl]
    V = [mp.mpf(0)] + [mp.mpf(float(x)) for x in logvol]
    n = len(logl)
    ldv, lz = [], []
    acc = None
    for i in range(n):
        step = V[i] - V[i + 1]
        d = V[i] + mp.log(-mp.expm1(-step)) - mp.log(2)
        ldv.append(d)
        a, b = (L[i + 1], L[i]) if L[i + 1] >= L[i] else (L[i], L[i + 1])
        lw = a + mp.log1p(mp.exp(b - a)) + d
        if acc is None:
            acc = lw
        else:
            m, s = (acc, lw) if acc >= lw else (lw, acc)
            acc = m + mp.log1p(mp.exp(s - m))
        lz.append(acc)
    lzf = lz[-1]
    part, hprev, var = mp.mpf(0), mp.mpf(0), mp.mpf(0)
    for i in range(n):
        part += mp.exp(L[i] - lzf + ldv[i]) * L[i] + mp.exp(L[i + 1] - lzf + ldv[i]) * L[i + 1]
        hi = part - lzf * mp.exp(lz[i] - lzf)
        var += (hi - hprev) * (V[i] - V[i + 1])
        hprev = hi
    return np.array([split(lzf), split(abs(var)), split(hprev)])


def _top(x, m):
    """Sum of the m largest entries of x."""
    x = np.sort(np.asarray(x, dtype=np.float64))
    return float(x[max(len(x) - int(m), 0):].sum())


def finish_bounds(fin, ndead, nlive, K, nfills, open_plateau=False):
    """Bounds (logz, h, logzvar, logzerr) on the record of a whole device run against `fin` = integrals_hp(logl, lv):
    `ndead` dead points consumed in at most `nfills` fills of K entries, then ns_finish over the N sorted live points.
    The volumes lv are INPUTS here (float64, replayed from the run's record by the oracle, death by death); the device
    has its own, so everything that differs between the two replays is part of the bound:

      lv      dead point k: the device's (nfills (c + 2)) u |lv| (consume_bounds) and the replay's k subtractions,
              (k + 1) u |lv|; plateau steps tau = 2u (2 |lv| + ln(N + 1)) + 8u relative (granted to every step).
              Live point i: both sides form lv_n + log(1 - i / (N + 1)) from the same expression: 2 ulp |rel| + 2u |lv|;
              with a plateau still open the steps are log1p(-i e^(plogdvol - lv_n)), whose argument carries both
              volume bounds: (2 b_lv + 8u) (e^|rel| - 1)
      step    the reference differences the volumes; the device takes the constant step (dead) or differences its own
              (live): 2u |lv| + tau step (dead), 4u |lv| + 2 (b_rel_i + b_rel_i-1) (live).  ln dX = lv + ln(expm1(step)
              / 2) feels it divided by 1 - e^-step -- at nlive = 9000 that is 1e4 * 4u |lv|
      lnZ     weighted mean of the terms' exponent errors as in consume_bounds, (c + 2) u + 2u ln(K + 1) + u |lnZ_k| for
              every fill, weighted by Z_k / Z (the `nfills` largest), and ns_finish's logaddexp chain: a thread's
              ceil(N / 256) points, 6 scan levels, 4 wave totals, the incoming ln Z: c_f (7u + u |lnZ|)
      H       sum |T_j| rel(alpha_j), alpha_j = b_z + b_ldv_j + 2u (|L_j| + |lnZ| + |ln dX_j|) + 3u + the sums' chain
              (nfills (c + 2) + c_f + 2) u, and for a dead point the fills' rescaling e^(lnZ_0 - lnZ_E) (the same
              float leaves one factor and enters the next: u |lnZ_j - lnZ| + 3u per fill); between fills the device
              keeps H = g - lnZ and re-forms g: 2u (|g| + |H|) per fill weighted by Z_k / Z (the `nfills` largest);
              - lnZ Z_i / Z with both ln Z bounds
      var     dead points: telescoped, b_h(n) s + sum |dH_k| |s - step_k|; a plateau death (step off the constant
              one) (b_h(k) + b_h(k - 1)) |step_k - s| + |dH_k| b_step; live points (b_h(i) + b_h(i - 1)) step_i +
              |dH_i| b_step_i; the chain (c_f + nfills + 8) u sum |dH step|
      logzerr = sqrt: |sqrt a - sqrt b| <= min(|a - b| / (2 sqrt(min)), sqrt |a - b|)"""
    n = fin["n"]
    f64 = lambda k: np.asarray(fin[k], dtype=np.float64)  # noqa: E731
    lz, hh, dh, step, ldv, lw, absT, zfrac = (f64(k) for k in ("lz", "hh", "dh", "step", "ldv", "lw", "absT", "zfrac"))
    lpad = f64("lpad")
    lv = -np.cumsum(step)
    lzf = float(fin["logz"])
    dlv = math.log((nlive + 1.0) / nlive)
    c1, cf = chain(K), -(-nlive // kT) + 12
    k1 = np.arange(1, n + 1, dtype=np.float64)
    dead = np.arange(n) < ndead
    lvn = lv[ndead - 1] if ndead else 0.0
    # --- volumes
    tau = 2 * U * (2 * np.abs(lv) + math.log(nlive + 1.0)) + 4 * ULP
    b_lv_dead = (nfills * (c1 + 2) + k1) * U * np.abs(lv) + np.cumsum(np.where(dead, tau * step, 0.0))
    b_lvn = b_lv_dead[ndead - 1] if ndead else 0.0
    rel = lv - lvn
    b_rel = 2 * ULP * np.abs(rel) + 2 * U * np.abs(lv) + ((2 * b_lvn + 8 * U) * np.expm1(np.abs(rel)) if open_plateau else 0.0)
    b_lv = np.where(dead, b_lv_dead, b_lvn + b_rel)
    b_relp = np.concatenate([[0.0], b_rel[:-1]])
    b_step = np.where(dead, 2 * U * np.abs(lv) + tau * step, 4 * U * np.abs(lv) + 2 * (b_rel + b_relp))
    lc = ldv - lv
    b_ldv = b_lv + b_step / -np.expm1(-step) + ULP * (1 + np.abs(lc)) + U * np.abs(ldv)
    lae = lw - ldv
    b_lw = b_ldv + 5 * U + U * np.abs(lae) + U * np.abs(lw)
    # --- ln Z
    eps = b_lw + U * (np.abs(lw - lz) + math.log(K + 1.0)) + ULP
    fillc = (c1 + 2) * U + ULP * math.log(K + 1.0) + U * np.abs(lz)
    with np.errstate(divide="ignore"):
        lfc = np.where(dead, lz + np.log(fillc), -np.inf)
    fc_k = np.minimum(nfills, k1) * np.exp(np.maximum.accumulate(lfc) - lz) if ndead else np.zeros(n)
    lchain = cf * (7 * U + U * np.max(np.abs(lz[ndead:]))) if n > ndead else 0.0
    b_zk = _wsum(lw + _log(eps), lz) + fc_k + np.where(dead, 0.0, lchain) + n * ETA
    b_zf = float(b_zk[-1])
    # --- H
    l0, l1 = lpad[:-1].copy(), lpad[1:]
    l0[l0 < -1e299] = 0.0
    nch = nfills * (c1 + 2) + cf + 2
    alpha = b_zf + b_ldv + 2 * U * (np.maximum(np.abs(l0), np.abs(l1)) + abs(lzf) + np.abs(ldv)) + 3 * U + (nch + 1) * U \
        + np.where(dead, U * np.abs(lz - lzf) + 3 * U * nfills, 0.0)
    dT = np.diff(absT, prepend=0.0)
    b_part = np.cumsum(dT * _rel(alpha)) + ETA * np.cumsum(2 + np.abs(l0) + np.abs(l1))
    part = hh + lzf * zfrac
    hcost = 2 * U * (2 * np.abs(part) + np.abs(lz) * zfrac)
    HC = _top(hcost[:ndead], nfills) if ndead else 0.0
    b_hk = b_part + abs(lzf) * zfrac * _rel(b_zk + b_zf + U * np.abs(lz - lzf) + ULP) + (b_zf + U * abs(lzf)) * zfrac \
        + HC + U * np.abs(hh)
    b_hm = np.concatenate([[0.0], b_hk[:-1]])
    # --- var
    off = np.abs(step - dlv)
    plat = dead & (off > 8 * U * (np.abs(lv) + 1.0))
    pts = np.where(dead, np.abs(dh) * off, 0.0) + np.where(plat, (b_hk + b_hm) * off + np.abs(dh) * b_step, 0.0) \
        + np.where(dead, 0.0, (b_hk + b_hm) * step + np.abs(dh) * b_step)
    b_var = float(np.sum(pts)) + (b_hk[ndead - 1] * dlv if ndead else 0.0) \
        + (cf + nfills + 8) * U * float(np.sum(np.abs(dh * step))) + 2 * n * ETA
    var = float(fin["logzvar"])
    err = math.sqrt(var)
    lin = b_var / (2 * math.sqrt(var - b_var)) if var > b_var else np.inf
    b_err = min(lin, math.sqrt(b_var)) + 2 * U * err
    return dict(logz=b_zf, h=float(b_hk[-1]), logzvar=b_var, logzerr=b_err)


def fill_rows(hp, b, ends, state0):
    """The reference's (logvol, logz, h, logzvar) after every fill (long double) and their bounds: rows of
    integrate_hp / consume_bounds at the fills' ends; a fill without a death leaves the state as it came."""
    ref, bd = np.empty((len(ends), 4), dtype=LD), np.zeros((len(ends), 4))
    for f, e in enumerate(ends):
        for q, name in enumerate(QUANT):
            ref[f, q] = hp[name][e - 1] if e > 0 else LD(state0[q])
            bd[f, q] = b[name][e - 1] if e > 0 else 0.0
    return ref, bd


def ratio(err, bound):
    """error / bound; a non-finite error is an infinite ratio, 0 / 0 is 0."""
    err = np.asarray(err, dtype=np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, np.abs(err) / bound)
    return np.where(np.isfinite(err), q, np.inf)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements: the recurrence as the reference runs it, and the scan form of csrc/ns.hip phase B
# ---------------------------------------------------------------------------------------------------------------------
def recurrence_f64(dead, steps, state0, ldv_err=0.0):
    """progress_integration death by death in float64 (ldv_err: added to every ln dX -- a degraded form).  Returns
    the (n, 4) states (logvol, logz, h, logzvar) after every death."""
    lv, lz, h, var, lprev = (float(x) for x in state0)
    out = np.empty((len(dead), 4))
    with np.errstate(all="ignore"):
        for k in range(len(dead)):
            lnew, s = float(dead[k]), float(steps[k])
            lv -= s
            ldv = lv + math.log(0.5 * math.expm1(s)) + ldv_err
            lw = np.logaddexp(lnew, lprev) + ldv
            lzn = np.logaddexp(lz, lw)
            lzterm = np.exp(lprev - lzn + ldv) * lprev + np.exp(lnew - lzn + ldv) * lnew
            hn = lzterm + np.exp(lz - lzn) * (h + lz) - lzn
            var += (hn - h) * s
            h, lz, lprev = hn, lzn, lnew
            out[k] = lv, lz, h, var
    return out


def scan_form_f64(dead, steps, pl, ends, state0, nlive, guard=True):
    """Phase B of ns_consume restated in float64 numpy, fill by fill: the weights summed in the linear domain relative
    to the fill's M, H from the additive G, the variance telescoped over the constant step and the plateau deaths
    patched back in with per-death H_e differences.  guard=False: the plateau correction as it stood before the deaths
    whose ln Z_e underflows relative to M were given to the recurrence.  Returns the (nfills, 4) states after every fill."""
    lv0, lz0, h0, var, lprev0 = (float(x) for x in state0)
    dlv = math.log((nlive + 1.0) / nlive)
    out = []
    start = 0
    with np.errstate(all="ignore"):
        for e1 in ends:
            d, s, p = dead[start:e1], steps[start:e1], pl[start:e1]
            n = len(d)
            if n == 0:
                out.append((lv0, lz0, h0, var))
                continue
            tie = bool(np.isfinite(p).any())
            prev = np.concatenate([[lprev0], d[:-1]])
            lvv = lv0 - np.cumsum(s) if tie else lv0 - np.arange(1, n + 1) * dlv
            ldv = lvv + np.log(0.5 * np.expm1(s))
            lw = np.logaddexp(d, prev) + ldv
            M = max(lz0, lw.max())
            z0 = math.exp(lz0 - M)
            lze = M + np.log(z0 + np.cumsum(np.exp(lw - M)))
            lzE = lze[-1]
            t0, t1 = np.exp(prev - lzE + ldv), np.exp(d - lzE + ldv)
            tt = np.where(t0 > 0, t0 * prev, 0.0) + np.where(t1 > 0, t1 * d, 0.0)
            w = math.exp(lz0 - lzE)
            g0 = w * (h0 + lz0) if w > 0 else 0.0
            hE = tt.sum() + g0 - lzE
            var0 = var
            var += (hE - h0) * dlv
            if tie:
                P = np.cumsum(tt)
                lzb = np.concatenate([[M + np.log(z0) if z0 > 0 else -np.inf], lze[:-1]])
                pd = np.flatnonzero(np.isfinite(p) & (s != dlv))
                if guard and len(pd) and min(lze[pd].min(), lzb[pd].min()) < M - UNDER:
                    # a plateau death whose ln Z_e is out of the linear sums' reach: the fill's variance from the
                    # recurrence, death by death
                    var = recurrence_f64(d, s, (lv0, lz0, h0, var0, lprev0))[-1, 3]
                    pd = []
                for e in pd:
                    delta = s[e] - dlv
                    pb = P[e - 1] if e else 0.0
                    hprev = h0 if e == 0 else np.exp(lzE - lzb[e]) * (g0 + pb) - lzb[e]
                    he = np.exp(lzE - lze[e]) * (g0 + pb + tt[e]) - lze[e]
                    var += (he - hprev) * delta
            lv0, lz0, h0, lprev0 = lvv[-1], lzE, hE, d[-1]
            out.append((lv0, lz0, h0, var))
            start = e1
    return np.array(out)


def open_plateau(hp, pl, e, state0, plogdvol):
    """Of a plateau still open after e deaths whose recorded ln volume step is `plogdvol`: how many deaths it has
    taken (the trailing deaths that carry this very step) and its ln volume step in long double."""
    j = 0
    while j < e and pl[e - 1 - j] == plogdvol:
        j += 1
    start = e - j  # deaths before the plateau
    return j, (hp["logvol"][start - 1] if start > 0 else LD(state0[0]))


def golden_record(key):
    """What tests/golden/ns_hp.npz holds of a case: per run the mpmath state after every fill that took a death, as
    (hi, lo) pairs, and the number of deaths after which a `stop` case's rule fires."""
    import ns_cases as C
    case = C.build(key)
    rec = {}
    for r in range(case.runs):
        ch = C.chain_inputs(case, r)
        ends = sorted(set(int(e) for e in ch["ends"] if e > 0))
        rec[f"{key}/r{r}/state"] = integrate_mp(ch["dead"], ch["steps"], ch["state0"], ends)
        rec[f"{key}/r{r}/ends"] = np.array(ends, dtype=np.int64)
        if case.family == "stop":
            rec[f"{key}/r{r}/ndead"] = np.array(ch["ends"][-1], dtype=np.int64)
            rec[f"{key}/r{r}/stopped"] = np.array(bool([x for x in case.ref[r] if x is not None][-1]["stopped"]))
    return rec
