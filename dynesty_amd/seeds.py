"""The seeds of a dynamic batch as a pure function: the NumPy mirror of the device's choice (csrc/merge_seed.hip,
dh_merged_batch_seed).

The reference draws nlive_new indices without replacement, each draw proportional to the remaining weights
exp(logvol_i) (_configure_batch_sampler, dynamicsampler.py:457-533: successive sampling; dynamic.batch_seed makes the
Generator's call).  The same law, order of the draws included, is "the nlive_new largest of logvol_i + G_i, G_i i.i.d.
standard Gumbel, in descending order" (Plackett-Luce).  It needs no normalisation and no sequential pass, and it is a
function of (seed, strand, point) like the volume realizations and the strand bootstrap of errors.py:

  words   strand s (a global index) uses subsequence SEED_SEQ + s = 2^63 + 2^62 + s of the Philox4x32-10 stream keyed
          by `seed`; point i -- its index in the merged run, not its position in the subset -- takes words 2 i and
          2 i + 1; u = 2^-53 + m 2^-53 in (0, 1] (errors.uniforms)
  key     logvol_i - log(-log u); u = 1 gives +inf, a legal key that is always chosen
  order   descending key, equal keys by smaller i; the strand's seeds are the first nlive_new points, in that order

The subset and the bookkeeping follow dynamic.batch_seed line for line, with one departure: a point can be chosen iff
logvol_i - max(logvol over the subset) >= LOG_MIN = -708 (the host's exp(..) / sum > 0 replaced by a threshold on exp's
argument, so that two libraries' exp cannot disagree at the denormal edge)."""
import numpy as np

from . import errors

__all__ = ["SEED_SEQ", "LOG_MIN", "seed_keys_host", "batch_seeds_host"]

SEED_SEQ = (1 << 63) + (1 << 62)  # strand s draws from subsequence SEED_SEQ + s (errors.BOOT_SEQ documents the ranges)
LOG_MIN = -708.0
MAX_STRANDS = 65536
MAX_NLIVE = 65535


def seed_keys_host(logvol, seed, strands, first=0):
    """key[s, i] = logvol_i - log(-log u[s, i]) for the strands first .. first + strands - 1 and every point i."""
    logvol = np.asarray(logvol, dtype=np.float64)
    u = errors.uniforms(seed, [SEED_SEQ + int(first) + s for s in range(int(strands))], len(logvol))
    with np.errstate(divide="ignore"):
        return logvol[None, :] - np.log(-np.log(u))


def _check(seed, first, strands, nlive_new, logl_min):
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed: an unsigned 64-bit integer")
    if not 1 <= int(strands) <= MAX_STRANDS:
        raise ValueError(f"batch_seeds: strands = {strands} (1 ... {MAX_STRANDS})")
    if not 1 <= int(nlive_new) <= MAX_NLIVE:
        raise ValueError(f"batch_seeds: nlive_new = {nlive_new} (1 ... {MAX_NLIVE})")
    if np.isnan(logl_min):
        raise ValueError("batch_seeds: logl_min is NaN")
    if not 0 <= int(first) <= (1 << 62) - int(strands):
        raise ValueError("batch_seeds: first must be 0 ... 2^62 - strands")


def batch_seeds_host(logl, logvol, logz, information, logzerr, logl_min, nlive_new, seed, strands, first=0):
    """The start points of `strands` strands of one batch from the saved run's columns: dict(prior, idx (strands,
    nlive_new) in draw order or None, keys (same shape) or None, logl_min (effective), vol_idx, start = (logvol, logz,
    information, logzerr^2, logl) at vol_idx - 1 or None, lo, count, n_pos).  Raises RuntimeError where no point lies
    above logl_min, ValueError where fewer than nlive_new points of positive weight do (dynamic.batch_seed's)."""
    logl = np.asarray(logl, dtype=np.float64)
    logvol = np.asarray(logvol, dtype=np.float64)
    k, S, M = int(nlive_new), int(strands), len(logl)
    logl_min = float(logl_min)
    _check(seed, first, S, k, logl_min)
    lo = int(np.searchsorted(logl, logl_min, side="right"))  # #{logl <= logl_min}
    count = M - lo

    def vol_idx_of(x):
        return 0 if x == -np.inf else int(np.argmin(np.abs(logl - x))) + 1
    if lo == 0:  # from the prior: no choice is made
        return dict(prior=True, idx=None, keys=None, logl_min=logl_min, vol_idx=vol_idx_of(logl_min), start=None, lo=0,
                    count=M, n_pos=0)
    if count == 0:
        raise RuntimeError(f"Could not find live points in the required logl interval: logl_min {logl_min}, "
                           f"saved ln L max {logl.max()}")
    if count < k:  # the boundary moves down to collect nlive_new points
        lo = 0 if M < k else M - k
        count = M - lo
        logl_min = float(logl[lo - 1]) if lo > 0 else -np.inf
    sub = logvol[lo:]
    can = sub - sub.max() >= LOG_MIN
    n_pos = int(can.sum())
    prior = logl_min == -np.inf
    vol_idx = vol_idx_of(logl_min)
    if n_pos < k:
        raise ValueError(f"batch_seeds: {n_pos} saved points of positive weight above ln L = {logl_min}, "
                         f"nlive_new = {k} are needed (a batch on fewer live points is not supported)")
    idx = np.empty((S, k), dtype=np.int64)
    keys = np.empty((S, k))
    cand = lo + np.nonzero(can)[0]
    step = max(1, (1 << 22) // max(M, 1))  # strands per block of keys: about 32 MB of them at a time
    for s0 in range(0, S, step):
        n = min(step, S - s0)
        key = seed_keys_host(logvol, seed, n, int(first) + s0)[:, cand]
        # descending key, equal keys by smaller index: a stable sort of the negated keys over ascending indices
        order = np.argsort(-key, axis=1, kind="stable")[:, :k]
        idx[s0:s0 + n] = cand[order]
        keys[s0:s0 + n] = np.take_along_axis(key, order, axis=1)
    if prior:
        start = None
    else:
        i = vol_idx - 1
        start = (float(logvol[i]), float(np.asarray(logz)[i]), float(np.asarray(information)[i]),
                 float(np.asarray(logzerr)[i]) ** 2, float(logl[i]))
    return dict(prior=prior, idx=idx, keys=keys, logl_min=logl_min, vol_idx=vol_idx, start=start, lo=lo, count=count,
                n_pos=n_pos)
