"""Statistical errors of a merged run, one surface for both merge routes: realizations of the prior-volume sequence
(the reference's utils.jitter_run, utils.py:1317-1408) and reweighting (utils.reweight_run, utils.py:1663-1708).

`ensemble.MergedRun` (merge='host') computes them in NumPy with the functions below, `_lib.DeviceMergedRun`
(merge='device') where the run lives (csrc/merge.hip).  Both are the same function of
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
distribution; the stream is not NumPy's Generator.beta.  u_k = 1 is a step of 0 and a weight of 0."""
import numpy as np

MAX_REAL = 65536  # realizations per call (dh_merged_realize's cap)
FIELDS = ("logvol", "logwt", "logz")
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


class Errors:
    """The methods both merged runs offer.  A class supplies `niter` (points), `_err_logl()`,
    `_err_realize(seed, first, nreal, jitter, logrwt, means)` -> (logz, information, ess, mean or None) and
    `_err_field(seed, real, jitter, logrwt, field, first, count)`, which validate their own arguments."""

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
