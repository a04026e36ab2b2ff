"""The integrals of a run that holds dynamic batches, restated in np.longdouble from the run's order alone -- its
sorted log-likelihoods and live counts: combine_runs' plateau rule in closed form (a group of p >= 2 equal ln L entered at
volume X with live count n has ln X_j = ln X + log1p(-(j + 1) / (n + 1))), then ln w, ln Z, H and var ln Z exactly as
tests/merge_hp_ref.py restates them for a merge of static runs.  The result has merge_hp's keys, so merge_hp_ref.bounds
and moment_bounds derive the device's bounds from it the way they do for the static merge; `bounds` here adds what the
closed form's log1p costs inside a group."""
import numpy as np

import merge_hp_ref as hp

LD = hp.LD


def groups(logl64):
    """(start index of the point's group, the group's length) per point of a sorted sequence."""
    logl64 = np.asarray(logl64, dtype=np.float64)
    M = len(logl64)
    change = np.concatenate([[True], logl64[1:] != logl64[:-1]])
    gid = np.cumsum(change) - 1
    gstart = np.flatnonzero(change)
    glen = np.diff(np.append(gstart, M))
    return gstart[gid], glen[gid]


def fold_hp(logl64, n, samples=None):
    logl64 = np.asarray(logl64, dtype=np.float64)
    n = np.asarray(n, dtype=np.int64)
    M = len(logl64)
    g0, p = groups(logl64)
    j = np.arange(M) - g0
    ni = n[g0]
    if (p >= ni + 1).any():
        raise ValueError("a plateau longer than the live count where it starts")
    single = p == 1
    # the point's own step ln X_{k-1} - ln X_k: log1p(1 / n), inside a group log1p(1 / (n_i - j))
    step = np.log1p(1 / np.where(single, n, ni - j).astype(LD))
    # the volume: per group one term, -log1p(-p / (n_i + 1)), which for p = 1 is the single point's step
    last = j == p - 1
    gterm = np.where(single, step, -np.log1p(-(p.astype(LD)) / (ni.astype(LD) + 1)))
    total = np.cumsum(np.where(last, gterm, LD(0)))          # the groups up to and including this point's, at its last
    before = np.concatenate([[LD(0)], total[:-1]])[g0]        # the groups before this point's
    logvol = np.where(single, -(before + gterm), -before + np.log1p(-((j + 1).astype(LD)) / (ni.astype(LD) + 1)))
    logl = logl64.astype(LD)
    lpad = np.concatenate([[LD(-1.e300)], logl])
    vpad = np.concatenate([[LD(0)], logvol])
    logdvol = vpad[:-1] + np.log(-np.expm1(-step)) - hp.LN2
    lae = np.array([hp._lae(lpad[i + 1], lpad[i]) for i in range(M)], dtype=LD)
    logwt = lae + logdvol
    logz = np.empty(M, dtype=LD)
    acc = LD(-np.inf)
    for i in range(M):
        acc = hp._lae(acc, logwt[i])
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
    out = dict(M=M, samples_n=n, logl=logl, step=step, logvol=logvol, logdvol=logdvol, lae=lae, logwt=logwt, logz=logz,
               information=h, logzvar=var, logzerr=np.sqrt(var), weights=w, ess=1 / np.sum(w * w),
               abs_info=np.cumsum(np.abs(t0) + np.abs(t1)), zfrac=zfrac, dh=dh, lpad=lpad, group_j=j, group_n=ni, group_p=p)
    if samples is not None:
        out.update(hp.moments_hp(samples, w))
    return out


def bounds(ref):
    """merge_hp_ref.bounds, plus inside a group: x = (j + 1) / (n_i + 1) carries two roundings, and log1p(-x) turns a
    relative error of x into x / (1 - x) absolute (its own 2u relative on top); the neighbour's enters ln dX of the
    next point, so every field downstream of ln X takes the larger of a point's and its predecessor's addition."""
    b = hp.bounds(ref)
    j, ni, p = ref["group_j"].astype(np.float64), ref["group_n"].astype(np.float64), ref["group_p"]
    x = (j + 1) / (ni + 1)
    add = np.where(p > 1, 4 * hp.U * x / (1 - x), 0.0)
    near = np.maximum(add, np.concatenate([[0.], add[:-1]]))
    b["logvol"] = b["logvol"] + add
    for k in ("logwt", "logz"):
        b[k] = b[k] + np.maximum.accumulate(near) if k == "logz" else b[k] + near
    return b
