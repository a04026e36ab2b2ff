"""High-precision reference of the RadFriends / SupFriends bounds (include/dynhip.h: dh_friends_update,
dh_friends_update_batch, dh_friends_within, dh_friends_draw) and error bounds for an fp64 evaluation of them, in the
manner of tests/ell_hp_ref.py, whose helpers and constants it uses.  Plain Python: no device code, nothing taken from
the operation order of csrc/.

  generator side (mpmath, 50 digits; tools/make_golden.py friends_hp and tests/test_friends_hp_cpu.py) -- the fp64
  input is exact data:
    partition_hp     pairwise Mahalanobis distances in the previous metric, single linkage cut at 1, the smallest
                     |dist - 1| of any pair (so that a case can declare its partition decided)
    shape_hp         covariance (ddof = 1) of the points re-centred per cluster, its spectrum and symmetric square root
    near_pairs_hp    the (probe, centre) distances of a membership case that lie within NEAR of 1

  test side (np.longdouble): the covariance, residuals taken on the covariance THE EVALUATOR RETURNED (so that a
  covariance error does not compound into the shape checks), the radius on the points whitened with the evaluator's
  own axes_inv, membership distances (difference first, then the metric), and the bounds, each beside its derivation.
  eps = 2^-53 throughout.

Not proved: the factors C_EIG, C_ORTH and C_INV of ell_hp_ref (calibrated there) are reused wherever the same
operation is bounded, and C_PINV_ROOT below.  tests/test_friends_hp_cpu.py holds two independent float64
implementations -- oracle/friends_ref.py (LAPACK through SciPy's pinvh / sqrtm) and a textbook Jacobi -- to half of
every bound; nothing is calibrated on device output.
"""
import math
import os

import mpmath as mp
import numpy as np
from scipy.spatial.distance import cdist

import ell_hp_ref as H
from ell_hp_ref import (DPS, EPS, LD, Ratios, _eig_mp, _hilo, _obj, cov_of_points_ld, fro, inverse_bound, ld,
                        log_spectrum_bound, logvol_prefactor_mp, mean_bound)

NEAR = 1e-5  # pairs closer to the threshold than this are evaluated at 50 digits

# Factor on inverse_bound(d, sqrt(kappa)) for axes_inv = pinvh(sqrtm(cov)).  The residual of an inverse built from
# the eigen-system of ANOTHER matrix (the covariance's, square-rooted) carries that system's orthogonality defect F
# as Lam^-1/2 F Lam^1/2, i.e. sqrt(kappa) ||F||, and ||F|| grows like D^1.5 for a Jacobi solver (ell_hp_ref.C_ORTH)
# where C_INV D eps grows like D.  Calibrated as C_INV is, on the CPU and on all 83 cases
# (tests/test_friends_hp_cpu.py asserts half of the bound or less and prints the worst): the float64 oracle reaches
# 0.28 of the bound (corr1e12/31), the textbook Jacobi in the parallel ordering 0.42 (iso/64/1025) and the row-cyclic
# one 0.43 (tail/60/1025) -- so the factor holds the half-bound criterion with a margin of 1.16, no more: 3 would not.
C_PINV_ROOT = 4.0


# =========================================================================================================
# generator side
# =========================================================================================================
def _pair_dist64(pts, am, rows):
    diff = pts[rows, None, :] - pts[None, :, :]
    return np.sqrt(np.maximum(np.einsum("rna,ab,rnb->rn", diff, am, diff, optimize=True), 0.0))


def _mahalanobis_mp(u, v, am_obj):
    dlt = _obj(u) - _obj(v)
    return mp.sqrt(dlt.dot(am_obj).dot(dlt))


def partition_hp(pts, am_prev):
    """Single-linkage partition of the points at Mahalanobis distance 1 in the metric am_prev.  Every pair in float64
    (difference first: relative error a few d eps), every pair within 1e-4 of the threshold again at 50 digits.
    Returns (labels: smallest index of the point's cluster, nclusters, margin = min |dist - 1| over all pairs)."""
    pts = np.asarray(pts, dtype=np.float64)
    n = len(pts)
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    margin = math.inf
    with mp.workdps(DPS):
        am_obj = _obj(am_prev)
        for r0 in range(0, n, 64):
            rows = np.arange(r0, min(n, r0 + 64))
            dist = _pair_dist64(pts, am_prev, rows)
            for a, i in enumerate(rows):
                dist[a, :i + 1] = np.inf  # pairs i < j once
            gap = np.abs(dist - 1.0)
            adj = dist <= 1.0
            for a, j in zip(*np.nonzero(gap < 1e-4)):
                dm = _mahalanobis_mp(pts[rows[a]], pts[j], am_obj)
                gap[a, j] = abs(float(dm - 1))
                adj[a, j] = dm <= 1
            margin = min(margin, float(gap[np.isfinite(dist)].min()) if np.isfinite(dist).any() else math.inf)
            for a, j in zip(*np.nonzero(adj)):
                ra, rb = find(int(rows[a])), find(int(j))
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    labels = np.array([find(i) for i in range(n)], dtype=np.int64)
    return labels, len(np.unique(labels)), margin


def shape_hp(pts, labels):
    """Covariance (ddof = 1) of the points after re-centring every cluster on its own mean -- one cluster: np.cov of
    the points --, its spectrum (ascending) and its symmetric square root V diag(sqrt lam) V^T, at 50 digits."""
    pts = np.asarray(pts, dtype=np.float64)
    n, d = pts.shape
    with mp.workdps(DPS):
        x = _obj(pts)
        if len(np.unique(labels)) > 1:
            for c in np.unique(labels):
                sel = labels == c
                x[sel] = x[sel] - (x[sel].sum(axis=0) / mp.mpf(int(sel.sum())))[None, :]
        dm = x - (x.sum(axis=0) / mp.mpf(n))[None, :]
        cov = dm.T.dot(dm) / mp.mpf(n - 1)
        lam, vec = _eig_mp(cov, True)
        root = (vec * np.array([mp.sqrt(v) if v > 0 else mp.mpf(0) for v in lam], dtype=object)[None, :]).dot(vec.T)
        return dict(cov=cov, lam=lam, root=root)


def near_pairs_hp(ctrs, axes_inv, x, kind):
    """(probe index, centre index, dist - 1 at 50 digits rounded to fp64) of every pair within NEAR of the threshold."""
    t64 = (ctrs[None, :, :] - x[:, None, :]) @ axes_inv
    d64 = np.sqrt((t64 * t64).sum(-1)) if kind == "balls" else np.abs(t64).max(-1)
    pi, ci = np.nonzero(np.abs(d64 - 1.0) < NEAR)
    out = []
    with mp.workdps(DPS):
        m_obj = _obj(axes_inv)
        for p, c in zip(pi, ci):
            t = (_obj(ctrs[c]) - _obj(x[p])).dot(m_obj)
            dist = mp.sqrt(sum(v * v for v in t)) if kind == "balls" else max(abs(v) for v in t)
            out.append(float(dist - 1))
    return pi.astype(np.int16), ci.astype(np.int16), np.array(out, dtype=np.float64)


# =========================================================================================================
# test side: long-double references and the bounds
# =========================================================================================================
def recentred_ld(pts, labels):
    x = ld(pts)
    if labels is not None and len(np.unique(labels)) > 1:
        x = x.copy()
        for c in np.unique(labels):
            sel = labels == c
            x[sel] -= x[sel].sum(axis=0) / LD(int(sel.sum()))
    return x


_COV_BOUND = {}


def friends_cov_bound(pts, labels):
    """_friends_cov_bound, kept for the last cloud (both kinds and every evaluator of a case ask for the same one)."""
    key = (np.asarray(pts).tobytes(), None if labels is None else np.asarray(labels).tobytes())
    if key not in _COV_BOUND:
        _COV_BOUND.clear()
        _COV_BOUND[key] = _friends_cov_bound(pts, labels)
    return _COV_BOUND[key]


def _friends_cov_bound(pts, labels):
    """(B, cov_ld): elementwise bound on |cov_fp64 - cov| and the long-double covariance.

    One cluster: ell_hp_ref.cov_bound's argument with the mean error BOUNDED (mean_bound) where that one measures it
    (no centre comes back from a friends update): (n + 6) eps S_ij for the two-pass sum, S_ij = sum |d_i| |d_j| /
    (n - 1), and n / (n - 1) e_i e_j for a mean off by e (second order: sum d = 0 about the true mean).
    Several clusters: every point first loses its cluster's mean.  That mean's error is constant over the cluster and
    again enters at second order (the deviations of one cluster sum to zero), e_i <- max over clusters of mean_bound
    plus the bound of the overall mean of the moved points; the rounding of x - mean, eps |d| per factor, adds
    2 eps S_ij."""
    n = len(pts)
    x = recentred_ld(pts, labels)
    _, cov = cov_of_points_ld(x)
    e = mean_bound(np.asarray(pts, dtype=np.float64))
    extra = 0
    if labels is not None and len(np.unique(labels)) > 1:
        e = np.max([mean_bound(pts[labels == c]) for c in np.unique(labels)], axis=0) + mean_bound(x.astype(np.float64))
        extra = 2
    dabs = np.abs(x - x.sum(axis=0) / LD(n))
    s = (dabs.T @ dabs / LD(n - 1)).astype(np.float64)
    return (n + 6 + extra) * EPS * s + n / (n - 1.0) * np.outer(e, e), cov


def sqrt_residual_bound(cov0, axes0):
    """||X X - C||_F for X = V diag(sqrt lam) V^T from an eigen-system of C:  X X = V Lam V^T + V Lam^1/2 F Lam^1/2 V^T
    with F = V^T V - I, so  eig_residual_bound(C)  (||C - V Lam V^T||, C_EIG)  +  orth_bound(d) lam_max  (C_ORTH;
    lam_max <= ||C||_F); forming X entry by entry, sum_k V_ik V_jk sqrt(lam_k) in any order, is off by
    (d + 2) eps sum_k |V_ik| |V_jk| sqrt(lam_k), whose Frobenius norm is at most sum_k sqrt(lam_k) = tr X (each
    |v_k| |v_k|^T has norm 1), and that enters X X as 2 ||X|| times it."""
    d = cov0.shape[0]
    return H.eig_residual_bound(cov0) + H.orth_bound(d) * fro(cov0) \
        + 2 * (d + 2) * EPS * fro(axes0) * float(np.trace(ld(axes0)))


def sqrt_error_bound(delta_c, lam_min):
    """||X - sqrtm(C)||_F from ||X X - C||_F <= delta_c:  E = X - sqrtm(C) solves the Sylvester equation
    sqrtm(C) E + E sqrtm(C) = X X - C - E E, whose operator has smallest singular value 2 sqrt(lam_min):
    ||E|| <= delta_c / (2 sqrt(lam_min)) to first order -- sqrt(kappa) / 2 in relative Frobenius terms --, and
    1 / (1 - ||E|| / sqrt(lam_min)) carries the quadratic term."""
    e1 = delta_c / (2 * math.sqrt(lam_min))
    th = e1 / math.sqrt(lam_min)
    return e1 / (1 - th) if th < 0.5 else math.inf


def pinv_root_bound(d, kappa):
    """||axes_inv axes - I||_F <= C_PINV_ROOT C_INV d eps sqrt(kappa)  (see C_PINV_ROOT)."""
    return C_PINV_ROOT * inverse_bound(d, math.sqrt(kappa))


def whiten_error(x, m, d, extra=0):
    """|fl(x M) - x M| per coordinate: d products and d - 1 additions in any order, fused or not,
    (d + 2) eps sum_k |x_k| |M_kj|  (`extra` more eps where M itself carries that many roundings)."""
    return (d + 2 + extra) * EPS * (np.abs(x) @ np.abs(m))


def _norm_rows(v, kind):
    return np.sqrt(np.sum(v * v, axis=-1)) if kind == "balls" else np.max(np.abs(v), axis=-1)


def radius_ld(y, kind, masks):
    """max_i min_j of the nearest-neighbour distances of the whitened points y (n, d) long double: leave-one-out, or
    per bootstrap replica from every left-out point to the resampled ones (a replica that leaves nothing out
    contributes nothing).  Candidates are ranked in float64 (difference first) and the four nearest re-measured in
    long double: a nearer one the ranking missed would have to tie four others to a few eps."""
    n = len(y)
    y64 = y.astype(np.float64)
    reps = [None] if masks is None else list(np.asarray(masks, dtype=bool))
    best = -math.inf
    for mk in reps:
        qi = np.arange(n) if mk is None else np.flatnonzero(~mk)
        cj = np.arange(n) if mk is None else np.flatnonzero(mk)
        for q0 in range(0, len(qi), 64):
            q = qi[q0:q0 + 64]
            d64 = cdist(y64[q], y64[cj], "euclidean" if kind == "balls" else "chebyshev")
            if mk is None:
                d64[np.arange(len(q)), q] = np.inf
            k = min(4, len(cj) - (1 if mk is None else 0))
            cand = np.argpartition(d64, k - 1, axis=1)[:, :k]
            dl = _norm_rows(y[q][:, None, :] - y[cj[cand]], kind)
            best = max(best, float(np.max(np.min(dl, axis=1))))
    return best


def radius_bound(pts, m, d, kind, r):
    """|r_fp64 - r|: max_i min_j is 1-Lipschitz in the distances, a distance moves by at most the sum of the two
    points' whitening errors in the norm of the kind (2 max_i ||e(x_i)||; M = axes_inv_out * rmax carries 2 eps more),
    and the norm itself -- d squares, additions in any order and a square root, or d subtractions and maxima -- by
    (d + 2) eps r."""
    e = whiten_error(np.asarray(pts, dtype=np.float64), np.asarray(m, dtype=np.float64), d, extra=2)
    return 2 * float(np.max(_norm_rows(e, kind))) + (d + 2) * EPS * r


def lam_of(rec):
    return H.lam_ld(rec)


def check_update(pts, kind, masks, out, rec, labels=None):
    """One successful update of `pts` -- out: dict(cov, am, axes, axes_inv, logvol, rmax, nclusters), scaled by the
    radius as dh_friends_update returns them -- against the fixture record `rec` of its cloud (lam_hi / lam_lo, root,
    ncl) and the long-double references.  Returns the Ratios."""
    r = Ratios()
    pts = np.asarray(pts, dtype=np.float64)
    n, d = pts.shape
    rm = float(out["rmax"])
    assert rm > 0 and math.isfinite(rm)
    assert int(out["nclusters"]) == int(rec["ncl"]), f"nclusters {out['nclusters']}, the reference has {rec['ncl']}"
    # un-scale in long double: two roundings (r * r, then the product or quotient) per entry of each matrix
    r2 = LD(rm) * LD(rm)
    cov0, am0 = ld(out["cov"]) / r2, ld(out["am"]) * r2
    ax0, ai0 = ld(out["axes"]) / LD(rm), ld(out["axes_inv"]) * LD(rm)
    eye = np.eye(d, dtype=LD)
    lam = lam_of(rec).astype(np.float64)
    kappa = float(lam[-1] / lam[0])
    # covariance, elementwise
    b, cov_ld = friends_cov_bound(pts, labels)
    bnd = b + 3 * EPS * np.abs(cov_ld).astype(np.float64)
    r.add("cov", np.max(np.abs(cov0 - cov_ld).astype(np.float64) / np.where(bnd > 0, bnd, 1.0)), 1.0)
    b_fro = fro(b)
    c64 = cov0.astype(np.float64)
    cn = fro(cov0)
    # spectrum of the returned covariance against the exact one's (Weyl), for kappa and ln V
    sb = H.spectrum_bound(c64, b_fro)
    x_min = sb / float(lam[0])
    kap = kappa / (1 - x_min) if x_min < 0.5 else math.inf
    # the three derived matrices on the evaluator's own covariance; 3 eps per un-scaled factor
    r.add("am", fro(am0 @ cov0 - eye), inverse_bound(d, kap) + 6 * EPS * math.sqrt(d))
    srb = sqrt_residual_bound(c64, ax0.astype(np.float64)) + 6 * EPS * cn
    r.add("axes_res", fro(ax0 @ ax0 - cov0), srb)
    # axes_inv = pinvh(axes): an evaluator that reads ONE triangle of its own square root (scipy's pinvh does) inverts
    # X + A with ||A||_F <= ||X - X^T||_F, and  axes_inv X - I = [axes_inv (X + A) - I] - axes_inv A
    asym = fro(ax0 - ax0.T)
    r.add("axes_inv", fro(ai0 @ ax0 - eye), pinv_root_bound(d, kap) + fro(ai0) * asym + 6 * EPS * math.sqrt(d))
    # ... the square root against the exact one of the exact covariance
    lam_min = float(lam[0]) * (1 - x_min)
    if "root" in rec:
        seb = sqrt_error_bound(b_fro + srb, float(lam[0])) + 2 * EPS * fro(rec["root"])
        r.add("axes", fro(ax0 - ld(rec["root"])), seb)
    # symmetry: M and M^T approximate one symmetric matrix, each within its own bound (for the square root: of ITS
    # covariance, sqrt_error_bound of the residual alone)
    r.add("sym_am", fro(am0 - am0.T) / fro(am0), 2 * inverse_bound(d, kap))
    r.add("sym_axes", asym, 2 * sqrt_error_bound(srb, lam_min))
    r.add("sym_axes_inv", fro(ai0 - ai0.T) / fro(ai0), 2 * pinv_root_bound(d, kap) + 2 * fro(ai0) * asym)
    # radius, on the points whitened with the evaluator's own axes_inv
    rr = radius_ld(ld(pts) @ ai0, kind, masks)
    r.add("rmax", abs(rm - rr), radius_bound(pts, ai0.astype(np.float64), d, kind, rr))
    # ln V of one shape: prefactor + 1/2 sum ln lam + d ln r, r the evaluator's own (held above)
    with mp.workdps(DPS):
        pre = logvol_prefactor_mp(d) if kind == "balls" else d * mp.log(2)
        pre_f, lg = float(pre), abs(float(mp.loggamma(mp.mpf(d) / 2 + 1))) + d * abs(float(mp.loggamma(mp.mpf(3) / 2)))
        lnr = float(mp.log(mp.mpf(rm)))
    half_sum = np.sum(np.log(lam_of(rec))) / 2
    want = float(LD(pre_f) + half_sum + LD(d) * LD(lnr))
    r.add("logvol", abs(float(out["logvol"]) - want), logvol_bound(d, sb, lam, pre_f, lg, lnr))
    return r


def logvol_bound(d, spec_bound, lam, pre, lgam, lnr):
    """|ln V_fp64 - ln V|: the spectrum's log bound (Weyl: every eigenvalue within spec_bound; x / (1 - x) per term);
    d logarithms and d + 3 additions and products of relative error eps each on the magnitudes they act on,
    (d + 6) eps (|prefactor| + 1/2 sum |ln lam_k| + d |ln r|); lgamma to 4 eps of its own value(s) (an fp64 libm
    rounds lgamma to a few ulp, not to one); d ln r: the logarithm of the radius to eps |ln r| + eps (its argument is
    the evaluator's own fp64 radius, so no d eps / r term of a radius error enters: the radius is held separately)."""
    mag = abs(pre) + 0.5 * float(np.sum(np.abs(np.log(np.asarray(lam, dtype=np.float64))))) + d * abs(lnr)
    return log_spectrum_bound(spec_bound, lam) + (d + 6) * EPS * mag + 4 * EPS * lgam + d * EPS


# ---- membership -------------------------------------------------------------------------------------------------------
def within_reference(ctrs, axes_inv, x, kind, near=None):
    """(gap, bound), both (m, n) float64: gap = dist - 1 of probe p to centre j -- float64 with the difference first
    everywhere, long double within 1e-3 of the threshold, the fixture's 50-digit value within NEAR -- and the DECISION
    bound of an evaluator that whitens centres and probes separately and subtracts afterwards: each whitened
    coordinate is off by whiten_error, the difference by eps more, and the norm by (d + 2) eps of itself."""
    ctrs, x, m = (np.asarray(a, dtype=np.float64) for a in (ctrs, x, axes_inv))
    d = ctrs.shape[1]
    t = (ctrs[None, :, :] - x[:, None, :]) @ m
    dist = _norm_rows(t, kind)
    gap = dist - 1.0
    pi, ci = np.nonzero(np.abs(gap) < 1e-3)
    if len(pi):
        tl = (ld(ctrs[ci]) - ld(x[pi])) @ ld(m)
        gap[pi, ci] = (_norm_rows(tl, kind) - LD(1)).astype(np.float64)
    if near is not None:
        gap[near[0], near[1]] = near[2]
    e = whiten_error(ctrs, m, d)[None, :, :] + whiten_error(x, m, d)[:, None, :] + EPS * np.abs(t)
    return gap, _norm_rows(e, kind) + (d + 2) * EPS * dist


def rows_from_bits(bits, n):
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def check_within(counts, bits, gap, bound, ring, what, free_ring=0.0):
    """Counts and bit rows of every decided probe equal the reference's; returns (share of undecided probes outside
    the rings at or below free_ring, number of undecided probes on those rings)."""
    m, n = gap.shape
    decided = np.all(np.abs(gap) > bound, axis=1)
    got = rows_from_bits(bits, n)
    want = gap <= 0
    for p in np.flatnonzero(decided):
        assert np.array_equal(got[p], want[p]), f"{what}: probe {p} bit row differs at {np.flatnonzero(got[p] != want[p])}"
        assert counts[p] == want[p].sum(), f"{what}: probe {p} count {counts[p]}, the reference has {want[p].sum()}"
    assert np.array_equal(got.sum(axis=1), counts), f"{what}: counts and bit rows disagree"
    free = np.abs(ring) <= free_ring
    free &= ring != 0
    return float(np.mean(~decided & ~free)), int(np.sum(~decided & free))


# =========================================================================================================
# the fixture (tools/make_golden.py friends_hp writes it)
# =========================================================================================================
def update_record(key):
    import friends_cases as FC
    case = {c[0]: c for c in FC.update_cases()}[key]
    _, name, d, n, clustering, _, fails = case
    pts = FC.cloud(name, d, n)
    out = {"ncl": np.int32(1), "margin": np.float64(np.inf), "labels": np.zeros(n, dtype=np.int16)}
    if clustering:
        labels, ncl, margin = partition_hp(pts, FC.prev_metric(name, d, n))
        out.update(ncl=np.int32(ncl), margin=np.float64(margin), labels=labels.astype(np.int16))
    if not fails:
        rec = shape_hp(pts, out["labels"])
        with mp.workdps(DPS):
            hl = [_hilo(v) for v in rec["lam"]]
            out["lam_hi"] = np.array([h for h, _ in hl])
            out["lam_lo"] = np.array([lo / h for h, lo in hl], dtype=np.float32)
            out["root"] = np.array([[float(v) for v in row] for row in rec["root"]])
    return out


def within_record(key, kind):
    import friends_cases as FC
    case = {c[0]: c for c in FC.within_cases()}[key]
    w = FC.within_inputs(*case[1:], kind)
    return near_pairs_hp(w["ctrs"], w["axes_inv"], w["x"], kind)


def all_keys():
    import friends_cases as FC
    return [c[0] for c in FC.update_cases()], [(c[0], k) for c in FC.within_cases() for k in FC.KINDS]


def pack_fixture(urec, wrec):
    """Numeric arrays only, in the order of all_keys() (the keys are regenerated, not stored)."""
    ukeys, wkeys = all_keys()
    assert sorted(ukeys) == sorted(urec) and sorted(wkeys) == sorted(wrec)
    has = np.array(["lam_hi" in urec[k] for k in ukeys], dtype=np.int8)
    g = {"has_shape": has}
    g["dim"] = np.array([len(urec[k]["lam_hi"]) if "lam_hi" in urec[k] else 0 for k in ukeys], dtype=np.int32)
    g["npts"] = np.array([len(urec[k]["labels"]) for k in ukeys], dtype=np.int32)
    g["ncl"] = np.array([urec[k]["ncl"] for k in ukeys], dtype=np.int32)
    g["margin"] = np.array([urec[k]["margin"] for k in ukeys], dtype=np.float64)
    g["labels"] = np.concatenate([urec[k]["labels"] for k in ukeys]).astype(np.int16)
    g["lam_hi"] = np.concatenate([urec[k]["lam_hi"] for k in ukeys if "lam_hi" in urec[k]])
    g["lam_lo"] = np.concatenate([urec[k]["lam_lo"] for k in ukeys if "lam_hi" in urec[k]]).astype(np.float32)
    g["root_tri"] = np.concatenate([urec[k]["root"][np.triu_indices(len(urec[k]["lam_hi"]))]
                                    for k in ukeys if "lam_hi" in urec[k]])
    g["near_count"] = np.array([len(wrec[k][0]) for k in wkeys], dtype=np.int32)
    for i, name in enumerate(("near_probe", "near_centre", "near_gap")):
        g[name] = np.concatenate([wrec[k][i] for k in wkeys])
    return g


def load_fixture(path=None):
    """({update key: arrays}, {(within key, kind): (probe idx, centre idx, gap)}) from tests/golden/friends_hp.npz."""
    g = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "friends_hp.npz"))
    ukeys, wkeys = all_keys()
    assert len(g["dim"]) == len(ukeys) and len(g["near_count"]) == len(wkeys), \
        "tests/golden/friends_hp.npz does not belong to this list of cases: regenerate it"
    dim, npts = g["dim"].astype(np.int64), g["npts"].astype(np.int64)
    lam_at = np.concatenate([[0], np.cumsum(dim)])
    tri_at = np.concatenate([[0], np.cumsum(dim * (dim + 1) // 2)])
    lab_at = np.concatenate([[0], np.cumsum(npts)])
    urec = {}
    for i, key in enumerate(ukeys):
        rec = {"ncl": g["ncl"][i], "margin": g["margin"][i], "labels": g["labels"][lab_at[i]:lab_at[i + 1]]}
        if g["has_shape"][i]:
            d = int(dim[i])
            rec["lam_hi"], rec["lam_lo"] = g["lam_hi"][lam_at[i]:lam_at[i + 1]], g["lam_lo"][lam_at[i]:lam_at[i + 1]]
            c = np.zeros((d, d))
            c[np.triu_indices(d)] = g["root_tri"][tri_at[i]:tri_at[i + 1]]
            rec["root"] = c + np.triu(c, 1).T
        urec[key] = rec
    at = np.concatenate([[0], np.cumsum(g["near_count"].astype(np.int64))])
    wrec = {k: tuple(g[nm][at[i]:at[i + 1]] for nm in ("near_probe", "near_centre", "near_gap"))
            for i, k in enumerate(wkeys)}
    return urec, wrec


def report(r, what):
    print(f"friends_hp {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))


def assert_ok(r, what):
    report(r, what)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1: {bad}"
