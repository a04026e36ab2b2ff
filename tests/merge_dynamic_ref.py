"""The divergence and the weight function of a merged run (dynesty_amd/errors.py; csrc/merge_errors.hip's me_integrate<., true>,
me_kld_finish, FRealKld, mw_*) restated in np.longdouble, and the bounds their float64
evaluations are held to.  Built on tests/merge_errors_ref.py (one realization and its bounds b_wt, b_lnZ),
tests/merge_bootstrap_ref.py (the expansion) and tests/merge_hp_ref.py (u, the scans' chains).  Nothing here is the
package's code, and no bound is fitted to an output.

The divergence.  A realization has ln w_p (bound b_wt[p], merge_errors_ref.bounds), Z = ln sum exp ln w; the merged run's
own LOGWT and LOGZ_{M-1} are data (float64 numbers taken as exact).  e_p = ln w_p - LOGWT_src(p), dz = Z - LOGZ_{M-1},
p_p = exp(ln w_p - Z):

  batch       K = (sum w'_p e_p) / (sum w'_p) - dz, w' the weights rescaled to the largest term
      e_p        : b_wt[p] + u |e_p| (the subtraction)                                                          =: be_p
      w'_p       : relative r_p = b_wt[p] + u (|ln w_p - top| + 8), merge_errors_ref's figure for the same number
      numerator  : sum p_p (|e_p| (r_p + 2u) + be_p) + (c_s + 4) u sum p_p |e_p|  (products, the batch-sum chain c_s)
      denominator: relative r_s = sum p_p r_p + (c_s + 4) u, times |sum p e| <= sum p |e|
      dz         : b_lnZ + u |dz|;   the division and the last subtraction: 2u (|ratio| + |dz| + |K|)
    Which term dominates: sum p_p be_p and b_lnZ, i.e. b_wt -- the (c + 4) u |ln X_p| of the volume scan carried into
    ln w_p -- at the points that hold the posterior mass; the products' and sums' own roundings are u sum p |e|, with
    |e| of order 1 where it would be u |ln Z| had ln w - lq been formed first.
  cumulative  term_p = p_p (e_p - dz) with Z from the per-point scan (bound b_Z = b_logz[-1]):
      d_p = e_p - dz : be_p + b_Z + u |dz| + u |d_p|                                                              =: bd_p
      p_p            : relative b_wt[p] + b_Z + u |ln w_p - Z| + 4u                                               =: rp_p
      prefix k       : sum_{p <= k} p_p (|d_p| (rp_p + 2u) + bd_p) + (c + 4) u sum_{p <= k} p_p |d_p|, c the scan's chain,
                       and ETA (1 + |d_p|) per point for terms that underflow

The weight function.  Ztot = logaddexp(LOGZ_{M-1}, LOGL_{M-1} + LOGVOL_{M-1}), D_k = LOGZ_k - Ztot <= 0,
lzw_k = Ztot + g(D_k) - log n_k with g = log(-expm1(.)), L = ln sum exp lzw, zweight = exp(lzw - L).

      Ztot   : u |LOGL + LOGVOL| + 4u (1 + |Ztot|) (merge_errors_ref's figure for a logaddexp)                    =: b_T
      D_k    : b_T + u |D_k|                                                                                      =: bD_k
      g(D_k) : |g'| = e^D / (1 - e^D) =: c_k, which grows without limit towards the end of the run; expm1 and log one
               ulp each: c_k bD_k + 2u + 2u |g|
      lzw_k  : b_T + that + 2u |log n| (the log) + 2u (|Ztot| + |g| + |log n| + |lzw|) (two additions), without c_k bD_k =: bl_k
      L      : sum zw_k (bl_k + c_k bD_k + u (|lzw_k - top| + 8)) + (c + 6) u + 2u |L|                            =: b_L
      zw_k   : ABSOLUTE: zw_k c_k bD_k + zw_k (bl_k + b_L + u |lzw_k - L| + 4u).  The product zw_k c_k =
               exp(Ztot + D_k - log n_k - L) is bounded (zweight vanishes like 1 - e^D where c_k diverges) and is
               formed as that exponential, never as a product of an overflowing and a vanishing number.
      pweight: exp(LOGWT_k - LOGZ_{M-1}) / sum: zw-like: pw_k (u |LOGWT_k - LOGZ| + (c + 10) u)
      weight : (1 - pfrac) b_zw + pfrac b_pw + 4u weight
      index k is decided when |weight_k - maxfrac max| > b_w[k] + maxfrac max(b_w) + 2u maxfrac max
    The reference's own zweight (a signed scipy logsumexp: 1 - e^D by subtraction) is allowed 4u (zw_k + zw_k c_k) more.
"""
import numpy as np

import merge_bootstrap_ref as br
import merge_errors_ref as er
from merge_errors_ref import check, device_chains, host_chains  # noqa: F401
from merge_hp_ref import ETA, LD, U


def sequence(m, mode, seed, index, mult=None):
    """(idx, n') of realization / bootstrap `index`: the merged run itself for 'jitter', else the expansion of the drawn
    (or given) multiplicities strand by strand (merge_bootstrap_ref)."""
    import bootstrap_cases as bc
    if mode == "jitter":
        return np.arange(len(m["logl"])), np.asarray(m["samples_n"])
    key, S = bc.strands(m)
    mult = np.bincount(br.draws(seed, index, S), minlength=S) if mult is None else mult
    return br.expand(m["logl"], key, mult)


def kld_hp(m, idx, n, seed, index, jitter):
    """The realization in long double with its divergence: adds e, dz, p, kld_cum, kld to merge_errors_ref's record."""
    h = er.realization_hp(np.asarray(m["logl"])[idx], n, seed, index, jitter)
    lqw = np.asarray(m["logwt"], dtype=np.float64)[idx].astype(LD)
    lz0 = LD(np.float64(m["logz"][-1]))
    lz = h["logz"][-1]
    with np.errstate(invalid="ignore"):
        e = h["logwt"] - lqw
        p = np.exp(h["logwt"] - lz)
        term = np.where(p > 0, p * (e - (lz - lz0)), LD(0))
    h.update(e=e, dz=lz - lz0, p=p, kld_cum=np.cumsum(term), kld=np.sum(term))
    return h


def kld_bounds(h, chains):
    """dict(batch=scalar, cum=[M']) for a float64 evaluation with the chains `chains` (see the module's text)."""
    b = er.bounds(h, chains)
    cs, cm = chains["scan"], chains["sums"]
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    p, e, lw = f(h["p"]), f(h["e"]), f(h["logwt"])
    dz, lz, K = float(h["dz"]), float(h["logz"][-1]), float(h["kld"])
    on = (p > 0) & np.isfinite(e)
    z = lambda a: np.where(on, a, 0.0)  # noqa: E731
    with np.errstate(invalid="ignore"):
        ae, top = z(np.abs(e)), np.max(lw)
        be = z(b["logwt"]) + U * ae
        r = z(b["logwt"] + U * (np.abs(lw - top) + 8))
        spe = float(np.sum(p * ae))
        r_s = float(np.sum(p * r)) + (cm + 4) * U
        batch = float(np.sum(p * (ae * (r + 2 * U) + be))) + (cm + 4) * U * spe + spe * r_s + b["logz_last"] + U * abs(dz) \
            + 2 * U * (spe + abs(dz) + abs(K))
        bz = float(b["logz"][-1])
        d = z(np.abs(e - dz))
        bd = be + bz + U * abs(dz) + U * d
        rp = z(b["logwt"] + bz + U * np.abs(lw - lz) + 4 * U)
        cum = np.cumsum(p * (d * (rp + 2 * U) + bd)) + (cs + 4) * U * np.cumsum(p * d) + ETA * np.cumsum(1 + d)
    return dict(batch=batch, cum=cum)


def weights_hp(m, pfrac):
    """pweight, zweight, weight of the merged run `m` (its arrays as data) in long double, and what the bounds need."""
    logz, logl, logvol, logwt = (np.asarray(m[k], dtype=np.float64).astype(LD) for k in ("logz", "logl", "logvol", "logwt"))
    n = np.asarray(m["samples_n"]).astype(LD)
    M = len(logz)
    pw = np.exp(logwt - logz[-1])
    pw = pw / pw.sum()
    out = dict(M=M, pw=pw, dlw=np.abs(logwt - logz[-1]))
    if logz[0] == logz[-1]:
        zw = np.full(M, LD(1) / M)
        out.update(zw=zw, degenerate=True)
    else:
        hi, lo = max(logz[-1], logl[-1] + logvol[-1]), min(logz[-1], logl[-1] + logvol[-1])
        ztot = hi + np.log1p(np.exp(lo - hi))
        D = logz - ztot
        with np.errstate(divide="ignore"):
            g = np.log(-np.expm1(D))
        lzw = ztot + g - np.log(n)
        top = lzw.max()
        L = top + np.log(np.exp(lzw - top).sum())
        zw = np.exp(lzw - L)
        out.update(zw=zw, degenerate=False, ztot=ztot, rem=logl[-1] + logvol[-1], D=D, g=g, logn=np.log(n), lzw=lzw, L=L,
                   zc=np.exp(ztot + D - np.log(n) - L))
    pf = LD(np.float64(pfrac))
    out["w"] = (1 - pf) * zw + pf * pw
    return out


def weight_bounds(h, pfrac, chain):
    """Absolute bounds dict(pw, zw, w) and the reference's extra allowance `ref_zw` (see the module's text)."""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    pw, zw, w = f(h["pw"]), f(h["zw"]), f(h["w"])
    b_pw = pw * (U * f(h["dlw"]) + (chain + 10) * U)
    if h["degenerate"]:
        b_zw, ref = 2 * U * zw, np.zeros_like(zw)
    else:
        ztot, D, g, logn, lzw, L, zc = (f(h[k]) for k in ("ztot", "D", "g", "logn", "lzw", "L", "zc"))
        fin = np.isfinite(g)
        z = lambda a: np.where(fin, a, 0.0)  # noqa: E731
        b_T = U * abs(float(h["rem"])) + 4 * U * (1 + abs(float(ztot)))
        bD = b_T + U * np.abs(D)
        bl = b_T + 2 * U + 2 * U * z(np.abs(g)) + 2 * U * logn + 2 * U * (abs(float(ztot)) + z(np.abs(g)) + logn + z(np.abs(lzw)))
        top = np.max(lzw)
        b_L = float(np.sum(zw * (bl + z(np.abs(lzw - top)) * U + 8 * U) + zc * bD)) + (chain + 6) * U + 2 * U * abs(float(L))
        b_zw = zc * bD + zw * (bl + b_L + U * z(np.abs(lzw - L)) + 4 * U)
        ref = 4 * U * (zw + zc)
    b_w = (1 - pfrac) * b_zw + pfrac * b_pw + 4 * U * w
    return dict(pw=b_pw, zw=b_zw, w=b_w, ref_zw=ref)


def decide(h, b_w, maxfrac):
    """(first, last) index with weight > maxfrac max(weight), and the smallest margin |weight_k - maxfrac max| over its
    allowance (> 1: every index is decided, whatever a float64 evaluation within the bounds does)."""
    w = np.asarray(h["w"], dtype=np.float64)
    thr = maxfrac * w.max()
    allow = b_w + maxfrac * np.max(b_w) + 2 * U * thr
    on = np.flatnonzero(h["w"] > LD(np.float64(maxfrac)) * h["w"].max())
    return (int(on[0]), int(on[-1])), float(np.min(np.abs(w - thr) / allow))
