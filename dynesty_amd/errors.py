"""Statistical errors of a merged run, one surface for both merge routes: realizations of the prior-volume sequence
(the reference's utils.jitter_run, utils.py:1317-1408) and reweighting (utils.reweight_run, utils.py:1663-1708).

`ensemble.MergedRun` (merge='host') computes them in NumPy with the functions below, `_lib.DeviceMergedRun`
(merge='device') where the run lives (csrc/merge_errors.hip).  Both are the same function of
(seed, realization index):

  words      realization r uses subsequence r of the Philox4x32-10 stream keyed by `seed` (rocrand's stream model: the
             counter of block b is (b mod 2^32, b >> 32, r mod 2^32, r >> 32)); point k takes words 2k and 2k + 1
  uniform    u_k = 2^-53 + (w0 | (w1 >> 11) << 32) 2^-53 in (0, 1] (rocrand's uniform_distribution_double), exact
  step       s_k = log(u_k) / n_k, i.e. t_k = u_k^(1 / n_k) ~ Beta(n_k, 1); jitter=False: the expected -log1p(1 / n_k)
  integrals  utils.compute_integrals (utils.py:1411-1467): ln X_k = s_0 + .. + s_k,
             ln dX_k = ln X_{k-1} + log(-expm1(s_k)), ln w_k = logaddexp(l_k, l_{k-1}) + ln dX_k + ln 1/2 (+ logrwt_k),
             ln Z = ln sum exp ln w, H = sum(w0 l0 + w1 l1) - ln Z with w0, w1 the two trapezoid halves WITHOUT logrwt
             (as the reference), ESS = (sum w)^2 / sum w^2, mean = sum w v / sum w

The ratios of consecutive uniform order statistics are independent Beta(j, 1) (Renyi / Malmquist), and a merged run's
live count never drops by more than 1 per point, so the reference's exact form and its approx=True are this same
distribution; the stream is not NumPy's Generator.beta.  u_k = 1 is a step of 0 and a weight of 0.

The strand bootstrap (utils.resample_run, utils.py:1495-1660) is on the same surface: a
strand is a (run, live slot) pair, bootstrap b draws as many strands as there are from subsequence 2^63 + b
(`strand_multiplicities`), the resampled run is every merged point repeated as often as its strand was drawn, in merged
order, with the reference's live counts (`expand_host`), and its integrals are realization b of that sequence
(jitter=False: utils.resample_run; jitter=True: a jitter_run after it, the documentation's simulate_run).

Run-level analysis of a dynamic sampler, again one surface: the Kullback-Leibler divergence
from the merged run to a realization or a bootstrap (utils.kld_error, utils.py:1932-1997), with e_p = ln w_p -
LOGWT_src(p) and Z the realization's own ln Z

  kld = sum_p w_p e_p / sum_p w_p - (Z - LOGZ_{M-1}),   cumulative: cumsum exp(ln w_p - Z) (e_p - (Z - LOGZ_{M-1}))

(the difference form: ln w - lq sits near ln Z while the divergence is small); the weight function
(dynamicsampler.weight_function, dynamicsampler.py:48-170: `weights_host`, `weight_bounds`) and the stopping function
(dynamicsampler.py:173-297), which is composition only."""
import warnings

import numpy as np

MAX_REAL = 65536  # realizations per call (dh_merged_realize's cap)
MAX_BOOT = 65536  # bootstraps per call (dh_merged_bootstrap's cap)
BOOT_SEQ = 1 << 63  # bootstrap b draws its strands from subsequence BOOT_SEQ + b: realization indices stay below it
# (the subsequences of one seed: realizations [0, 2^63), bootstraps 2^63 + b with b < 2^62, and from 2^63 + 2^62 on the
# strands of a dynamic batch's weighted choice of seeds -- seeds.SEED_SEQ + s, csrc/merge_seed.hip)
FIELDS = ("logvol", "logwt", "logz")
BOOT_FIELDS = ("idx", "samples_n", "logvol", "logwt", "logz")
KLD_MODES = ("jitter", "resample", "simulate")  # dh_merged_kld's DH_KLD_JITTER, _RESAMPLE, _SIMULATE
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
_LN_HALF = -0.6931471805599453


def philox_blocks(seed, seq, block):
    """Philox4x32-10 under key `seed` of the counters (block, seq), broadcast: uint32 [..., 4] in stream order."""
    seed, seq, block = np.broadcast_arrays(np.asarray(seed, dtype=np.uint64), np.asarray(seq, dtype=np.uint64),
                                           np.asarray(block, dtype=np.uint64))
    k0, k1 = seed & _MASK, seed >> _S32
    c0, c1, c2, c3 = block & _MASK, block >> _S32, seq & _MASK, seq >> _S32
    for r in range(10):
        if r:
            k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
        p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64 bits
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform_double(w0, w1):
    """rocrand's uniform_distribution_double(w0, w1): (0, 1], exact in float64."""
    m = np.asarray(w0, dtype=np.uint64) | ((np.asarray(w1, dtype=np.uint64) >> np.uint64(11)) << _S32)
    return 2.0 ** -53 + m.astype(np.float64) * 2.0 ** -53


def uniforms(seed, reals, M):
    """u[r, k] for the realizations `reals` (Python ints / uint64) and the points k < M."""
    reals = np.array([int(r) for r in np.atleast_1d(reals)], dtype=np.uint64)
    nb = (int(M) + 1) // 2
    w = philox_blocks(np.uint64(int(seed)), reals[:, None], np.arange(nb, dtype=np.uint64)[None, :])
    return uniform_double(w[..., 0::2], w[..., 1::2]).reshape(len(reals), 2 * nb)[:, :M]


def steps(seed, reals, samples_n, jitter=True):
    """s[r, k] = ln t_k of the realizations `reals`."""
    n = np.asarray(samples_n, dtype=np.float64)
    if not jitter:
        return np.broadcast_to(-np.log1p(1.0 / n), (len(np.atleast_1d(reals)), len(n))).copy()
    return np.log(uniforms(seed, reals, len(n))) / n


def _check_common(M, seed, logrwt):
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed: an unsigned 64-bit integer")
    if logrwt is None:
        return None
    logrwt = np.ascontiguousarray(logrwt, dtype=np.float64)
    if logrwt.shape != (M,):
        raise ValueError(f"logrwt of shape {logrwt.shape} for {M} points")
    if not (logrwt < np.inf).all():
        raise ValueError("logrwt: NaN and +inf are not weights (-inf is a weight of 0)")
    return logrwt


def _logwt(logl, s, logrwt):
    """(ln X, ln dX / 2, ln w) for steps s [T, M]."""
    logvol = np.cumsum(s, axis=1)
    v0 = np.concatenate([np.zeros((len(s), 1)), logvol[:, :-1]], axis=1)
    with np.errstate(divide="ignore"):
        ldv = v0 + np.log(-np.expm1(s)) + _LN_HALF
    lae = np.logaddexp(logl, np.concatenate([[-1.e300], logl[:-1]]))
    lw = lae + ldv
    if logrwt is not None:
        lw = lw + logrwt
    return logvol, ldv, lw


def realize_host(logl, samples_n, samples, seed, first, nreal, jitter=True, logrwt=None, means=False):
    """dh_merged_realize in NumPy: (logz, information, ess, mean or None) of the realizations first .. first + nreal - 1,
    a tile of realizations at a time."""
    logl = np.asarray(logl, dtype=np.float64)
    M = len(logl)
    logrwt = _check_common(M, seed, logrwt)
    first, nreal = int(first), int(nreal)
    if not 1 <= nreal <= MAX_REAL:
        raise ValueError(f"nreal {nreal} outside [1, {MAX_REAL}]")
    if not jitter and nreal != 1:
        raise ValueError("the expected volumes are one realization: nreal = 1 with jitter=False")
    if first < 0 or first + nreal > 1 << 63:
        raise ValueError("first: a non-negative realization index")
    if means and samples is None:
        raise ValueError("means: this merged run has no samples")
    l0 = np.concatenate([[-1.e300], logl[:-1]])
    logz, h, ess = np.empty(nreal), np.empty(nreal), np.empty(nreal)
    mean = np.empty((nreal, np.shape(samples)[1])) if means else None
    tile = max(1, min(nreal, (1 << 21) // max(M, 1)))
    for r0 in range(0, nreal, tile):
        r1 = min(nreal, r0 + tile)
        s = steps(seed, [first + r for r in range(r0, r1)], samples_n, jitter)
        _, ldv, lw = _logwt(logl, s, logrwt)
        with np.errstate(invalid="ignore", over="ignore"):
            top = lw.max(axis=1, keepdims=True)
            w = np.exp(lw - np.where(np.isfinite(top), top, 0.0))
            sw = w.sum(axis=1)
            lz = top[:, 0] + np.log(sw)
            w0, w1 = np.exp(l0 - lz[:, None] + ldv), np.exp(logl - lz[:, None] + ldv)
            h[r0:r1] = (np.where(w0 > 0, w0 * l0, 0.0) + np.where(w1 > 0, w1 * logl, 0.0)).sum(axis=1) - lz
            logz[r0:r1], ess[r0:r1] = lz, sw * sw / (w * w).sum(axis=1)
            if means:  # (one realization at a time: a matrix product's order of additions depends on its shape)
                v = np.asarray(samples, dtype=np.float64)
                for i in range(r1 - r0):
                    mean[r0 + i] = (w[i][:, None] * v).sum(axis=0) / sw[i]
    return logz, h, ess, mean


def realization_host(logl, samples_n, seed, real, jitter=True, logrwt=None, field="logz", first=0, count=None):
    """dh_merged_realization in NumPy: `count` points from `first` on of one per-point field of one realization."""
    logl = np.asarray(logl, dtype=np.float64)
    M = len(logl)
    logrwt = _check_common(M, seed, logrwt)
    if field not in FIELDS:
        raise ValueError(f"field {field!r}: one of {FIELDS}")
    first = int(first)
    count = M - first if count is None else int(count)
    if int(real) < 0 or int(real) >= 1 << 63:
        raise ValueError("real: a non-negative realization index")
    if first < 0 or count < 0 or first + count > M:
        raise ValueError(f"[{first}, {first + count}) of {M} points")
    logvol, _, lw = _logwt(logl, steps(seed, [int(real)], samples_n, jitter), logrwt)
    out = logvol[0] if field == "logvol" else lw[0] if field == "logwt" else np.logaddexp.accumulate(lw[0])
    return np.ascontiguousarray(out[first:first + count])


def strand_multiplicities(seed, boot, S):
    """m_u of bootstrap `boot`: the histogram of S strand draws.  Draw j takes words 2j and 2j + 1 of subsequence
    2^63 + boot of the stream keyed by `seed`; with x = w0 | w1 << 32 the strand is the high 64 bits of x S (no
    rejection: a bias below S 2^-64)."""
    S, boot = int(S), int(boot)
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed: an unsigned 64-bit integer")
    if not 0 <= boot < BOOT_SEQ:
        raise ValueError("boot: a non-negative bootstrap index")
    if not 1 <= S < 1 << 31:
        raise ValueError(f"{S} strands")
    w = philox_blocks(np.uint64(int(seed)), np.uint64(BOOT_SEQ + boot), np.arange((S + 1) // 2, dtype=np.uint64))
    w = w.reshape(-1, 2)[:S].astype(np.uint64)  # draw j: (w0, w1)
    lo, hi, s = w[:, 0], w[:, 1], np.uint64(S)
    u = (hi * s + ((lo * s) >> _S32)) >> _S32  # the high 64 bits of (lo | hi << 32) S, S < 2^31
    return np.bincount(u.astype(np.int64), minlength=S).astype(np.int64)


def expand_host(logl, strand, final, mult):
    """The resampled run of the multiplicities `mult` (per strand): merged point k repeated m_k = mult[strand[k]]
    times in merged order (one valid result of the reference's unstable argsort; the stable one) and the live count
    of every expanded position (utils.resample_run, utils.py:1601-1622).  With T = sum of m over the strands, E the
    exclusive prefix over merged order of (final ? m_k : 0): a point alone at its ln L has n' = T - E for all its
    copies, a final one T - E - c for copy c.  A group of equal ln L = L holding g expanded positions i = 0 .. g - 1:

        n'(i) = T - (sum of m over final points with ln L <= L)
                + sum over the group's final points with m > 0 of int((g - 1 - i) / (g / m)) + 1

    the division in float64 as written.  Returns (idx, n'), int64."""
    logl = np.asarray(logl, dtype=np.float64)
    M = len(logl)
    final = np.asarray(final).astype(bool)
    mk = np.asarray(mult, dtype=np.int64)[np.asarray(strand, dtype=np.int64)]
    off = np.concatenate([[0], np.cumsum(mk)])
    mf = np.where(final, mk, 0)
    E = np.concatenate([[0], np.cumsum(mf)])
    T, Mx = int(E[-1]), int(off[-1])
    if not 0 < Mx < 1 << 31:
        raise ValueError(f"the resampled run has {Mx} points (1 to 2^31 - 1)")
    idx = np.repeat(np.arange(M, dtype=np.int64), mk)
    n = T - E[idx] - np.where(final[idx], np.arange(Mx, dtype=np.int64) - off[idx], 0)
    head = np.flatnonzero(np.concatenate([[True], logl[1:] != logl[:-1], [True]]))
    tied = np.flatnonzero(np.diff(head) >= 2)  # the groups of two or more merged points
    for a, b in zip(head[tied], head[tied + 1]):
        p0, g = int(off[a]), int(off[b] - off[a])
        if g == 0:
            continue
        i = np.arange(g, dtype=np.int64)
        acc = np.full(g, T - int(E[b]), dtype=np.int64)
        for e in range(a, b):
            if final[e] and mk[e] > 0:
                acc += ((g - 1 - i) / (g / int(mk[e]))).astype(np.int64) + 1
        n[p0:p0 + g] = acc
    return idx, n


def _check_boot(seed, first, nboot, mult, S):
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed: an unsigned 64-bit integer")
    if not 1 <= int(nboot) <= MAX_BOOT:
        raise ValueError(f"nboot {nboot} outside [1, {MAX_BOOT}]")
    if int(first) < 0 or int(first) + int(nboot) > BOOT_SEQ:
        raise ValueError("first: a non-negative bootstrap index")
    if mult is None:
        return None
    mult = np.ascontiguousarray(mult)
    if mult.shape != (S,) or mult.dtype.kind not in "iu":
        raise ValueError(f"mult: {S} integers, one per strand (run * nlive + slot)")
    if int(nboot) != 1:
        raise ValueError("mult: given multiplicities are one bootstrap (nboot = 1)")
    if (mult < 0).any() or (mult >= 1 << 31).any():
        raise ValueError("mult: multiplicities are non-negative 32-bit integers")
    return mult.astype(np.int64)


def bootstrap_host(logl, strand, final, S, samples, seed, first, nboot, jitter=False, mult=None, means=False):
    """dh_merged_bootstrap in NumPy: (logz, information, ess, mean or None, npoints) of the bootstraps
    first .. first + nboot - 1: the strands' multiplicities (`mult` in their place), the expansion, then realization
    `b` of the expanded sequence (realize_host: jitter=False is the expected volumes of the resampled run, the
    reference's utils.resample_run; jitter=True its jitter after the resampling)."""
    mult = _check_boot(seed, first, nboot, mult, int(S))
    if means and samples is None:
        raise ValueError("means: this merged run has no samples")
    nboot, first = int(nboot), int(first)
    logl = np.asarray(logl, dtype=np.float64)
    logz, h, ess, npts = np.empty(nboot), np.empty(nboot), np.empty(nboot), np.empty(nboot, dtype=np.int64)
    mean = np.empty((nboot, np.shape(samples)[1])) if means else None
    for b in range(nboot):
        m = strand_multiplicities(seed, first + b, S) if mult is None else mult
        idx, n = expand_host(logl, strand, final, m)
        r = realize_host(logl[idx], n, np.asarray(samples)[idx] if means else None, seed, first + b, 1, bool(jitter),
                         None, means)
        logz[b], h[b], ess[b], npts[b] = r[0][0], r[1][0], r[2][0], len(idx)
        if means:
            mean[b] = r[3][0]
    return logz, h, ess, mean, npts


def bootstrap_run_host(logl, strand, final, S, seed, boot, jitter=False, mult=None):
    """dh_merged_bootstrap_run in NumPy: idx, samples_n, logvol, logwt and the cumulative logz of one bootstrap."""
    mult = _check_boot(seed, boot, 1, mult, int(S))
    logl = np.asarray(logl, dtype=np.float64)
    idx, n = expand_host(logl, strand, final, strand_multiplicities(seed, boot, S) if mult is None else mult)
    logvol, _, lw = _logwt(logl[idx], steps(seed, [int(boot)], n, bool(jitter)), None)
    return dict(idx=idx, samples_n=n, logvol=logvol[0], logwt=lw[0], logz=np.logaddexp.accumulate(lw[0]))


def _kld_of(lw, lqw, lz0):
    """(kld, ln Z) of the realizations lw [T, M'] against LOGWT_src `lqw` [M'] and the merged run's last ln Z."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        top = lw.max(axis=1, keepdims=True)
        w = np.exp(lw - np.where(np.isfinite(top), top, 0.0))
        we = np.where(w > 0, w * (lw - lqw), 0.0)  # (a weight of 0 adds nothing, also where e is inf - inf)
        sw = w.sum(axis=1)
        lz = top[:, 0] + np.log(sw)
        return we.sum(axis=1) / sw - (lz - lz0), lz


def _kld_cum(lw, lqw, lz0):
    """The cumulative divergence of one realization lw [M']."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lz = np.logaddexp.accumulate(lw)[-1]
        p = np.exp(lw - lz)
        return np.cumsum(np.where(p > 0, p * ((lw - lqw) - (lz - lz0)), 0.0))


def _check_kld(seed, first, n, cap):
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed: an unsigned 64-bit integer")
    if not 1 <= int(n) <= cap:
        raise ValueError(f"n {n} outside [1, {cap}]")
    if int(first) < 0 or int(first) + int(n) > 1 << 63:
        raise ValueError("first: a non-negative index")


def kld_host(logl, samples_n, logwt, logz_last, seed, first, n, jitter=True):
    """dh_merged_kld(DH_KLD_JITTER) in NumPy: (kld, logz) of the realizations first .. first + n - 1 against the merged
    run's own logwt and last logz.  jitter=False (n = 1): the expected volumes, whose divergence is 0 to rounding."""
    logl = np.asarray(logl, dtype=np.float64)
    M, first, n = len(logl), int(first), int(n)
    _check_kld(seed, first, n, MAX_REAL)
    if not jitter and n != 1:
        raise ValueError("the expected volumes are one realization: n = 1 with jitter=False")
    lqw = np.asarray(logwt, dtype=np.float64)
    kld, logz = np.empty(n), np.empty(n)
    tile = max(1, min(n, (1 << 21) // max(M, 1)))
    for r0 in range(0, n, tile):
        r1 = min(n, r0 + tile)
        s = steps(seed, [first + r for r in range(r0, r1)], samples_n, jitter)
        kld[r0:r1], logz[r0:r1] = _kld_of(_logwt(logl, s, None)[2], lqw, float(logz_last))
    return kld, logz


def kld_bootstrap_host(logl, strand, final, S, logwt, logz_last, seed, first, n, jitter=False, mult=None):
    """dh_merged_kld(DH_KLD_RESAMPLE / _SIMULATE) in NumPy: (kld, logz, npoints) of the bootstraps first .. first + n - 1."""
    mult = _check_boot(seed, first, n, mult, int(S))
    logl, lqw = np.asarray(logl, dtype=np.float64), np.asarray(logwt, dtype=np.float64)
    n, first = int(n), int(first)
    kld, logz, npts = np.empty(n), np.empty(n), np.empty(n, dtype=np.int64)
    for b in range(n):
        idx, nx = expand_host(logl, strand, final, strand_multiplicities(seed, first + b, S) if mult is None else mult)
        lw = _logwt(logl[idx], steps(seed, [first + b], nx, bool(jitter)), None)[2]
        k, z = _kld_of(lw, lqw[idx], float(logz_last))
        kld[b], logz[b], npts[b] = k[0], z[0], len(idx)
    return kld, logz, npts


def kld_run_host(logl, samples_n, logwt, logz_last, seed, real, jitter=True):
    """The field DH_MERGED_KLD of dh_merged_realization in NumPy: the cumulative divergence of realization `real`."""
    logl = np.asarray(logl, dtype=np.float64)
    _check_kld(seed, real, 1, MAX_REAL)
    lw = _logwt(logl, steps(seed, [int(real)], samples_n, jitter), None)[2][0]
    return _kld_cum(lw, np.asarray(logwt, dtype=np.float64), float(logz_last))


def kld_bootstrap_run_host(logl, strand, final, S, logwt, logz_last, seed, boot, jitter=False, mult=None):
    """The same of dh_merged_bootstrap_run: the cumulative divergence of bootstrap `boot`."""
    mult = _check_boot(seed, boot, 1, mult, int(S))
    logl = np.asarray(logl, dtype=np.float64)
    idx, nx = expand_host(logl, strand, final, strand_multiplicities(seed, boot, S) if mult is None else mult)
    lw = _logwt(logl[idx], steps(seed, [int(boot)], nx, bool(jitter)), None)[2][0]
    return _kld_cum(lw, np.asarray(logwt, dtype=np.float64)[idx], float(logz_last))


def weights_host(logl, logvol, logz, samples_n, pweight, pfrac):
    """(pweight, zweight, weight) of dynamicsampler.compute_weights / weight_function as dh_merged_weights forms them:
    the remaining evidence through expm1 (the reference's signed logsumexp cancels at the end of the run)."""
    logz, M = np.asarray(logz, dtype=np.float64), len(logl)
    if logz[0] == logz[-1]:  # the reference's np.ptp(logz) == 0 (logz never decreases)
        zw = np.full(M, 1.0 / M)
    else:
        with np.errstate(divide="ignore"):
            ztot = np.logaddexp(logz[-1], logl[-1] + logvol[-1])
            lzw = ztot + np.log(-np.expm1(logz - ztot)) - np.log(np.asarray(samples_n, dtype=np.float64))
            top = lzw.max()
            zw = np.exp(lzw - (top + np.log(np.exp(lzw - top).sum())))
    pw = np.asarray(pweight, dtype=np.float64)
    return pw, zw, (1.0 - pfrac) * zw + pfrac * pw


def weight_indices(weight, maxfrac):
    """The first and last point with weight > maxfrac max(weight)."""
    on = np.flatnonzero(weight > maxfrac * np.max(weight))
    if not len(on):
        raise ValueError(f"weight_function: no weight above {maxfrac} x the largest")
    return int(on[0]), int(on[-1])


def weight_bounds(i0, i1, pad, M, logl_at):
    """(logl_min, logl_max) from the two indices: the padding and overflow rules of dynamicsampler.py:147-166 as
    written.  logl_at(k): ln L of point k (at most two are asked for)."""
    b0, b1 = int(i0) - int(pad), int(i1) + int(pad)
    if b1 > M - 1:  # overflow on the right: the left side moves
        b0, b1 = b0 - (b1 - (M - 1)), M - 1
    if b0 <= 0:  # overflow on the left: -inf, and the right side expands
        logl_min, logl_max = -np.inf, None if b1 == M - 1 else float(logl_at(min(b1 - b0, M - 1)))
    else:
        logl_min, logl_max = float(logl_at(b0)), None if b1 == M - 1 else float(logl_at(b1))
    return logl_min, np.inf if logl_max is None else logl_max


class Errors:
    """The methods both merged runs offer.  A class supplies `niter` (points), `_err_logl()`,
    `_err_realize(seed, first, nreal, jitter, logrwt, means)` -> (logz, information, ess, mean or None) and
    `_err_field(seed, real, jitter, logrwt, field, first, count)`, which validate their own arguments; for the strand
    bootstrap `_err_bootstrap(seed, first, nboot, jitter, mult, means)` -> (logz, information, ess, mean or None,
    npoints) and `_err_bootstrap_run(seed, boot, jitter, mult)` -> a dict of BOOT_FIELDS."""

    def logz_realizations(self, nreal, seed=0, first=0, logrwt=None, means=False, jitter=True):
        """Realizations first .. first + nreal - 1 of the prior volumes under `seed`: a dict of logz, information and
        ess (nreal each) and with means=True mean (nreal, ndim).  logrwt: per-point ln(new / old target) added to
        ln w.  jitter=False (nreal = 1): the expected volumes."""
        lz, h, ess, mean = self._err_realize(seed, first, nreal, bool(jitter), logrwt, bool(means))
        out = dict(logz=lz, information=h, ess=ess)
        if means:
            out["mean"] = mean
        return out

    def logz_error(self, nreal=256, seed=0):
        """(mean, standard deviation with ddof = 1) of ln Z over `nreal` realizations: the error bar the reference's
        documentation takes from utils.jitter_run."""
        if int(nreal) < 2:
            raise ValueError("logz_error: at least 2 realizations")
        lz = self.logz_realizations(nreal, seed)["logz"]
        return float(lz.mean()), float(lz.std(ddof=1))

    def realization(self, field, seed=0, real=0, first=0, count=None, jitter=True, logrwt=None):
        """`count` points (None: to the end) from point `first` on of logvol, logwt or the cumulative logz of one
        realization."""
        return self._err_field(seed, real, bool(jitter), logrwt, field, first, count)

    def jitter_run(self, seed=0, real=0):
        """utils.jitter_run's per-point results for realization `real`: a dict of logvol, logwt and logz."""
        return {f: self.realization(f, seed, real) for f in FIELDS}

    def reweight(self, logp_new, logp_old=None):
        """utils.reweight_run at the expected volumes: logz, information, ess (floats) and mean (ndim) under the
        target logp_new in place of logp_old (None: the merged logl)."""
        old = self._err_logl() if logp_old is None else np.asarray(logp_old, dtype=np.float64)
        new = np.asarray(logp_new, dtype=np.float64)
        if new.shape != (self.niter,) or old.shape != (self.niter,):
            raise ValueError(f"reweight: {self.niter} values of logp_new (and logp_old)")
        with np.errstate(invalid="ignore"):
            logrwt = new - old
        lz, h, ess, mean = self._err_realize(0, 0, 1, False, logrwt, True)
        return dict(logz=float(lz[0]), information=float(h[0]), ess=float(ess[0]), mean=mean[0])

    def bootstrap_realizations(self, nboot, seed=0, first=0, jitter=False, means=False):
        """Strand bootstraps first .. first + nboot - 1 under `seed` (the reference's utils.resample_run; with
        jitter=True followed by its utils.jitter_run, the documentation's simulate_run): a dict of logz, information,
        ess and npoints (the resampled run's length), nboot each, and with means=True mean (nboot, ndim)."""
        lz, h, ess, mean, npts = self._err_bootstrap(seed, first, nboot, bool(jitter), None, bool(means))
        out = dict(logz=lz, information=h, ess=ess, npoints=npts)
        if means:
            out["mean"] = mean
        return out

    def resample_run(self, seed=0, boot=0, mult=None):
        """utils.resample_run(res, return_idx=True)'s per-point results for bootstrap `boot`: a dict of idx (the
        merged-run index of every point of the resampled run, the reference's samp_idx in the stable order),
        samples_n, logvol, logwt and logz.  mult: multiplicities per strand (run * nlive + slot) in place of the
        drawn ones."""
        return self._err_bootstrap_run(seed, boot, False, mult)

    def simulate_run(self, seed=0, boot=0):
        """resample_run followed by jitter_run: position p of bootstrap `boot` takes the uniform of point p of
        realization `boot`."""
        return self._err_bootstrap_run(seed, boot, True, None)

    def _boot_error(self, nboot, seed, jitter, what):
        if int(nboot) < 2:
            raise ValueError(f"{what}: at least 2 bootstraps")
        lz = self.bootstrap_realizations(nboot, seed, jitter=jitter)["logz"]
        return float(lz.mean()), float(lz.std(ddof=1))

    def logz_error_sampling(self, nboot=256, seed=0):
        """(mean, standard deviation with ddof = 1) of ln Z over `nboot` strand bootstraps: the sampling part of the
        error (utils.resample_run)."""
        return self._boot_error(nboot, seed, False, "logz_error_sampling")

    def logz_error_total(self, nboot=256, seed=0):
        """The same over bootstraps that are jittered too: the total error (simulate_run)."""
        return self._boot_error(nboot, seed, True, "logz_error_total")

    # Run-level analysis.  A class supplies `_err_kld(seed, first, n, mode, mult)` ->
    # (kld, logz, npoints), `_err_kld_run(seed, index, mode, mult, first, count)`, `_err_weights(pfrac)` -> (pweight,
    # zweight, weight), `_err_weight_function(pfrac, maxfrac, pad)` -> ((logl_min, logl_max), (first, last)) and
    # `_err_summary()` -> (logzerr, ess); mode is an index into KLD_MODES.

    @staticmethod
    def _kld_mode(error):
        if error not in KLD_MODES:
            raise ValueError(f"error {error!r}: one of {KLD_MODES}")
        return KLD_MODES.index(error)

    def kld_realizations(self, n, seed=0, first=0, error="jitter"):
        """utils.kld_error's last value for the realizations (error='jitter': logz_realizations' stream) or strand
        bootstraps ('resample': bootstrap_realizations; 'simulate': the same with jitter) first .. first + n - 1: a
        dict of kld and logz, and npoints for the bootstrap modes.  The bootstrap modes may be negative, as the
        reference's are."""
        mode = self._kld_mode(error)
        kld, lz, npts = self._err_kld(seed, first, n, mode, None)
        out = dict(kld=kld, logz=lz)
        if mode:
            out["npoints"] = npts
        return out

    def kld_error(self, seed=0, index=0, error="jitter", mult=None, first=0, count=None):
        """utils.kld_error: `count` points (None: to the end) from point `first` on of the cumulative divergence from
        this run to realization or bootstrap `index`.  mult (bootstrap modes): multiplicities per strand in place of the
        drawn ones."""
        mode = self._kld_mode(error)
        if mode == 0 and mult is not None:
            raise ValueError("mult: multiplicities belong to the bootstrap modes")
        return self._err_kld_run(seed, index, mode, mult, first, count)

    @staticmethod
    def _check_weight_args(pfrac, maxfrac, pad):
        if not 0. <= pfrac <= 1.:
            raise ValueError(f"The provided `pfrac` {pfrac} is not between 0. and 1.")
        if not 0. <= maxfrac <= 1.:
            raise ValueError(f"The provided `maxfrac` {maxfrac} is not between 0. and 1.")
        if pad != int(pad) or pad < 0:
            raise ValueError(f"`lpad` {pad} is less than zero (or no integer).")

    def weight_function(self, pfrac=0.8, maxfrac=0.8, pad=1, return_weights=False):
        """dynamicsampler.weight_function: (logl_min, logl_max), the ln L range of the points whose weight
        (1 - pfrac) zweight + pfrac pweight lies above maxfrac x the largest, padded by `pad` points; with
        return_weights=True also (pweight, zweight, weight)."""
        self._check_weight_args(pfrac, maxfrac, pad)
        bounds, _ = self._err_weight_function(float(pfrac), float(maxfrac), int(pad))
        if return_weights:
            return bounds, self._err_weights(float(pfrac))
        return bounds

    def stopping_function(self, pfrac=1.0, evid_thresh=0.1, target_n_effective=10000, n_mc=0, error="jitter", seed=0,
                          return_vals=False):
        """dynamicsampler.stopping_function: stop <= 1 with stop = pfrac stop_post + (1 - pfrac) stop_evid,
        stop_post = target_n_effective / ESS, stop_evid = std(ln Z) / evid_thresh; the standard deviation (ddof 0) over
        n_mc > 1 realizations ('jitter') or bootstraps ('resample', 'simulate') under `seed`, else the run's own
        logzerr.  The divergences the reference computes there and drops are not computed.  return_vals: also
        (stop_post, stop_evid, stop)."""
        if not 0. <= pfrac <= 1.:
            raise ValueError(f"The provided `pfrac` {pfrac} is not between 0. and 1.")
        if pfrac < 1. and evid_thresh < 0.:
            raise ValueError(f"The provided `evid_thresh` {evid_thresh} is not non-negative even though `pfrac` is {pfrac}.")
        if pfrac > 0. and target_n_effective < 0.:
            raise ValueError(f"The provided `target_n_effective` {target_n_effective} is not non-negative even though "
                             f"`pfrac` is {pfrac}")
        if n_mc < 0:
            raise ValueError(f"The number of realizations {n_mc} must be greater or equal to zero.")
        if 0 < n_mc < 20:
            warnings.warn("Using a small number of realizations might result in excessively noisy stopping value estimates.")
        mode = self._kld_mode(error)
        logzerr, ess = self._err_summary()
        if n_mc > 1:
            lz = (self.logz_realizations(n_mc, seed) if mode == 0 else
                  self.bootstrap_realizations(n_mc, seed, jitter=mode == 2))["logz"]
            lnz_std = float(np.std(lz))
        else:
            lnz_std = float(logzerr)
        stop_evid = lnz_std / evid_thresh
        stop_post = target_n_effective / float(ess)
        stop = pfrac * stop_post + (1. - pfrac) * stop_evid
        return (stop <= 1., (stop_post, stop_evid, stop)) if return_vals else stop <= 1.
