"""High-precision reference of the split tree of MultiEllipsoid.update (include/dynhip.h: dh_rebuild, mode 0) and the
bounds inside which an fp64 evaluator must take the same decisions.  Plain Python over index arrays: no device code,
nothing of the operation order of csrc/, no device order of nodes.

The recursion (the reference project's _bounding_ellipsoids, as oracle/bounding_ref.py::split_tree cites it):

  node ellipsoid   ell_hp_ref.bounding_ellipsoid_hp: mpmath at 50 digits, the 1 - 1e-3 rescale, improve_covar_mat
                   (mode "mp"); or the same in np.longdouble for the rule perturbations, which need decisions only
                   (mode "ld": LDL^T pivots for ln V, a Gaussian solve for the largest Mahalanobis form)
  below 4 d points the node is a leaf
  scale            population standard deviation (ddof = 0) of the ROOT's points, per coordinate, long double
  seeds            ctr -+ axes[:, argmax(axlens)]; the axis carries the device's documented sign (include/dynhip.h:
                   largest-magnitude component positive, the first one on ties), so cluster 0 and with it the ORDER of
                   the output list (cluster 0's subtree first) is predicted, not only the set of leaves
  Lloyd            ten assign-then-update iterations on points / scale in long double; label 1 iff d1 < d0 (strict:
                   centroid 0 wins ties); an empty cluster keeps its centroid; the labels are the tenth assignment's
  child size rule  a child below 2 d points: the split is rejected and no child is built
  accept test      dec = (d (d + 3) // 2) ln(m) / m with the node's own m;
                   logaddexp(lnV0, lnV1) - lnV < -dec  or  logsumexp(lnV of the subtrees' lists) - lnV < -dec (len - 1),
                   bottom-up: the children's recursion runs BEFORE the test, whatever its verdict

nnodes.  csrc/rebuild.hip counts the tree nodes it CREATED: the root (k_root: nnodes = 1) and two per k-means node whose
children both have at least 2 d points (split_body: atomicAdd(nnodes, 2)), whether or not the accept test later keeps
them -- a child below 4 d points is created (its ellipsoid is built and read by the parent's test) and not split.
csrc/wide.hip counts the nodes its host recursion visits, which is the same set.  So
    nnodes = 1 + 2 * #{nodes that ran k-means and got two children of >= 2 d points}
= the number of node ellipsoids built: the one output that shows what happened inside discarded subtrees.

Decidability (DESIGN.md 3.3.1 has the derivations).  Every decision is recorded with margin / bound, the bound being
what an fp64 evaluator of the same rules may get wrong; nothing is fitted to device output:

  label      |d1 - d0| against  (d + 3) eps (d0 + d1)                          the two distance chains
                              + 2 eps sum_j |c0_j - c1_j| |y_j|                the division x / scale (same y in both)
                              + 2.5 eps_s (d0 + d1)                            the scale's own error (a common metric)
                              + 2 sum_j (|y_j - c0_j| dc0_j + |y_j - c1_j| dc1_j)   the centroids
             iteration 0: dc = (centre bound + major-axis bound) / scale; later: the mean bound of the label set
  accept     the distance from the threshold against the sum of the ln V bounds of the ellipsoids read
  order      the lead of the major axis's largest component over its second largest, and the leading eigenvalue gap,
             against the axis's error
  size rules integer comparisons

Granted, not proved: ell_hp_ref's C_EIG / C_ORTH / C_INV (stated there), and GRANT_AXIS below.
"""
import math
import os
from dataclasses import dataclass, replace

import mpmath as mp
import numpy as np

import ell_hp_ref as H
import split_cases as SC

LD = H.LD
EPS = H.EPS
ITERS = 10

# The eigen-free route (spd_fast in csrc/rebuild.hip) takes the major axis from repeated squaring, stopped once the
# second eigenvalue's weight is below ~5e-9 in the matrix about to be squared, i.e. below 1e-16 in the one kept, and
# the axis length from a Rayleigh quotient.  The truncation is stated in the code; the rounding of the LAST squaring
# and of the normalisation (earlier squarings' errors are squared away with everything else that is not the leading
# eigenvector) is taken as 16 d eps of a unit vector.  Granted, not derived.
GRANT_AXIS = 16.0

# decision codes of a k-means node
TOO_SMALL, ACCEPT_FIRST, ACCEPT_SECOND, REJECTED = range(4)


@dataclass(frozen=True)
class Rules:
    """The rules as they are (defaults) or one of the wrong rules of PERTURBATIONS."""
    use_scale: bool = True
    ddof: int = 0
    node_scale: bool = False
    iters: int = ITERS
    labels_after_update: bool = False
    le: bool = False
    first_only: bool = False
    len_minus: int = 1
    dec_from_root: bool = False
    min_size_add: int = 0
    split_add: int = 0
    flip_sign: bool = False


RULES = Rules()
PERTURBATIONS = {
    "no scale": replace(RULES, use_scale=False),
    "scale with ddof = 1": replace(RULES, ddof=1),
    "scale from the node": replace(RULES, node_scale=True),
    "9 iterations": replace(RULES, iters=9),
    "11 iterations": replace(RULES, iters=11),
    "labels after the last update": replace(RULES, labels_after_update=True),
    "<= in the label comparison": replace(RULES, le=True),
    "first disjunct only": replace(RULES, first_only=True),
    "len for len - 1": replace(RULES, len_minus=0),
    "dec from the root's n": replace(RULES, dec_from_root=True),
    "size rule 2 d + 1": replace(RULES, min_size_add=1),
    "split threshold 4 d + 1": replace(RULES, split_add=1),
    "opposite axis sign": replace(RULES, flip_sign=True),
}


# =========================================================================================================
# pieces
# =========================================================================================================
def canon_sign(v):
    i = int(np.argmax(np.abs(v)))
    return -v if v[i] < 0 else v


def _ld_of(x):
    hi, lo = H._hilo(x)
    return LD(hi) + LD(lo)


def _logdet_ld(a):
    """ln det of a positive definite long-double matrix: Gaussian elimination without pivoting (LDL^T pivots)."""
    a = np.array(a, dtype=LD)
    out = LD(0)
    for k in range(a.shape[0]):
        assert a[k, k] > 0
        out += np.log(a[k, k])
        f = a[k + 1:, k] / a[k, k]
        a[k + 1:] -= f[:, None] * a[k][None, :]
    return out


def top_eigenpair_ld(cov):
    """Leading eigenpair of a symmetric long-double matrix: LAPACK's fp64 vector refined by Rayleigh-quotient
    iteration in long double (cubic: two steps reach the type's precision), until the residual is at rounding."""
    d = cov.shape[0]
    _, vec = np.linalg.eigh(cov.astype(np.float64))
    v = vec[:, -1].astype(LD)
    mu = v @ cov @ v
    tol = 64 * d * np.finfo(LD).eps * np.sqrt(np.sum(cov * cov))
    for _ in range(6):
        r = cov @ v - mu * v
        if np.sqrt(r @ r) <= tol:
            return mu, v
        w = H.ld_solve(cov - mu * np.eye(d, dtype=LD), v[:, None])[:, 0]
        if not np.all(np.isfinite(w)):
            break
        v = w / np.sqrt(w @ w)
        mu = v @ cov @ v
    r = cov @ v - mu * v
    assert np.sqrt(r @ r) <= tol, "the long-double eigenvector did not converge"
    return mu, v


def node_ellipsoid(p, mode):
    """The bounding ellipsoid of the fp64 points p: dict(mu, cov (long double, unscaled), mult, lnv (long double),
    rec (the mpmath record; None in mode "ld"))."""
    n, d = p.shape
    x = H.ld(p)
    mu = x.sum(axis=0) / LD(n)
    dm = x - mu
    cov = dm.T @ dm / LD(n - 1)
    if mode == "mp":
        rec = H.bounding_ellipsoid_hp(p)
        assert rec["icm"]["good"], "a node of a split case needs improve_covar_mat's loop: not a case for this set"
        with mp.workdps(H.DPS):
            mult, lnv = _ld_of(rec["mult"]), _ld_of(rec["lnv"])
        return dict(mu=mu, cov=cov, mult=mult, lnv=lnv, rec=rec)
    q = np.sum(dm * H.ld_solve(cov, dm.T).T, axis=1)
    fmax = q.max()
    mult = fmax / LD(H.LIM) if fmax > LD(H.LIM) else LD(1)
    lnv = LD(H.logvol_prefactor(d)) + (_logdet_ld(cov) + d * np.log(mult)) / 2
    return dict(mu=mu, cov=cov, mult=mult, lnv=lnv, rec=None)


def node_bounds(p, e, handed):
    """What an fp64 evaluator may get wrong about the ellipsoid e of the points p (mode "mp"): dict(lnv: |ln V error|,
    sb: every eigenvalue of the final covariance, mb: relative error of the rescaling factor, ctr: per coordinate).
    `handed`: the centre comes from the parent's k-means sums (cluster sum of x / scale over the count, times scale:
    the sum's (m + 1) eps mean |x / scale| scale, which is mean_bound, and two more roundings of the value)."""
    n, d = p.shape
    ctr_b = H.mean_bound(p) + (2 * EPS * np.abs(e["mu"]).astype(np.float64) if handed else 0.0)
    dabs = np.abs(H.ld(p) - e["mu"])
    s = (dabs.T @ dabs / LD(n - 1)).astype(np.float64)
    b = (n + 6) * EPS * s + n / (n - 1.0) * np.outer(ctr_b, ctr_b)  # ell_hp_ref.cov_bound with e = the centre's bound
    cov64 = e["cov"].astype(np.float64)
    rho = float(np.max(np.diag(b) / np.diag(cov64)))
    delta = H.fro(b) + rho * H.fro(cov64)
    mult = float(e["mult"])
    lam = H.lam_ld(H.fixture_record(e["rec"])).astype(np.float64)  # the final spectrum, ascending
    sb = H.spectrum_bound(cov64 * mult, mult * delta)
    lsb = H.log_spectrum_bound(sb, lam)
    kappa = float(lam[-1] / lam[0])
    # the rescaling factor fmax / (1 - 1e-3): ell_hp_ref.check_bounding's "scale" bound with the true inverse
    am = H.ld_solve(e["cov"], np.eye(d, dtype=LD))
    q, sabs = H.quadforms_ld(p, e["mu"], am)
    dl = H.ld(p) - e["mu"]
    shift = 2 * np.abs(dl @ am) @ H.ld(ctr_b) + H.ld(ctr_b) @ np.abs(am) @ H.ld(ctr_b)
    mb = rho + delta / (float(lam[0]) / mult) + math.sqrt(kappa) * H.inverse_bound(d, kappa) \
        + float(np.max(H.quadform_bound(d, sabs)) + np.max(shift)) / float(q.max())
    # ln V: through the spectrum (or, for the eigen-free route, LDL^T pivots of the same matrix: the same Weyl bound
    # once more, as check_bounding grants it), its own sum, and d / 2 ln of the rescaling factor
    lnv_b = 2 * lsb + H.logvol_self_bound(d, np.sqrt(lam)) + 4 * d * EPS + 0.5 * d * (mb + 4 * EPS)
    return dict(lnv=lnv_b, sb=sb, mb=mb, ctr=ctr_b, lam=lam)


def major_axis(e, bounds=None):
    """(axis = sqrt(lam_max) v with the canonical sign, error bound of the axis as a vector norm, order ratio)."""
    lam1, v = top_eigenpair_ld(e["cov"])
    v = canon_sign(v)
    axis = np.sqrt(lam1 * e["mult"]) * v
    if bounds is None:
        return axis, None, None
    lam = bounds["lam"]
    assert abs(float(lam1 * e["mult"]) / lam[-1] - 1) < 1e-14, "long-double and mpmath leading eigenvalues differ"
    gap = float(lam[-1] - lam[-2]) if len(lam) > 1 else math.inf
    sb = bounds["sb"]
    if not sb < 0.25 * gap:
        return axis, math.inf, 0.0
    d = len(v)
    # direction: Davis-Kahan, sin(angle) <= ||E|| / (gap - ||E||) <= 2 sb / gap, plus the granted term of the
    # squaring route; length: sqrt of an eigenvalue within sb (and d eps of the Rayleigh quotient's own chain), and the
    # rescaling factor's square root
    dv = 2 * sb / gap + GRANT_AXIS * d * EPS
    top = math.sqrt(lam[-1])
    axis_b = top * dv + (sb + (d + 2) * EPS * lam[-1]) / (2 * top) + 0.5 * bounds["mb"] * top
    a = np.sort(np.abs(v).astype(np.float64))[::-1]
    lead = (a[0] - a[1]) / (2 * dv) if d > 1 else math.inf
    return axis, axis_b, min(lead, gap / (4 * sb))


def lloyd(y, seeds, rules, seed_b=None, eps_s=0.0):
    """k = 2 Lloyd iterations in long double.  Returns (labels, dict(margin, ratio, moving, empty)); ratio = the
    smallest |d1 - d0| / bound over points and iterations (None without seed_b)."""
    cen = np.array(seeds, dtype=LD)
    d = y.shape[1]
    dc = None if seed_b is None else [np.array(seed_b, dtype=np.float64), np.array(seed_b, dtype=np.float64)]
    yabs = np.abs(y).astype(np.float64)
    margin, ratio, empty = math.inf, math.inf, False
    labs = []
    niter = rules.iters + (1 if rules.labels_after_update else 0)
    for _ in range(niter):
        r0, r1 = y - cen[0], y - cen[1]
        d0, d1 = np.sum(r0 * r0, axis=1), np.sum(r1 * r1, axis=1)
        lab = (d1 <= d0) if rules.le else (d1 < d0)
        diff = np.abs(d1 - d0).astype(np.float64)
        tot = (d0 + d1).astype(np.float64)
        margin = min(margin, float(np.min(diff / tot)))
        if dc is not None:
            bound = (d + 3) * EPS * tot + 2 * EPS * (yabs @ np.abs(cen[0] - cen[1]).astype(np.float64)) \
                + 2.5 * eps_s * tot + 2 * (np.abs(r0).astype(np.float64) @ dc[0] + np.abs(r1).astype(np.float64) @ dc[1])
            ratio = min(ratio, float(np.min(diff / bound)))
        labs.append(lab)
        for c in (0, 1):
            sel = lab == bool(c)
            if np.any(sel):
                cen[c] = y[sel].sum(axis=0) / LD(int(sel.sum()))
                if dc is not None:
                    dc[c] = (int(sel.sum()) + 1) * EPS * np.mean(yabs[sel], axis=0)
            else:
                empty = True
    moving = len(labs) > 1 and not np.array_equal(labs[-1], labs[-2])
    return labs[-1].astype(np.int8), dict(margin=margin, ratio=None if dc is None else ratio, moving=moving, empty=empty)


def scale_of(p, ddof=0):
    """Per-coordinate standard deviation in long double, and the relative error an fp64 two-pass evaluation of it may
    have: half the variance's ((n + 6) eps for the sum of squares about the evaluator's mean, whose own error enters
    at second order, (e / sigma)^2), two roundings for the root and the division."""
    x = H.ld(p)
    n = len(x)
    mu = x.sum(axis=0) / LD(n)
    var = np.sum((x - mu)**2, axis=0) / LD(n - ddof)
    s = np.sqrt(var)
    e = H.mean_bound(p)
    eps_s = 0.5 * (n + 6) * EPS + 0.5 * float(np.max((e / s.astype(np.float64))**2)) + 2 * EPS
    return s, eps_s


def _lse(vals):
    v = np.array(vals, dtype=LD)
    m = v.max()
    return m + np.log(np.sum(np.exp(v - m)))


# =========================================================================================================
# the recursion
# =========================================================================================================
def split_tree_ref(pts, mode="mp", rules=RULES):
    """The split tree of the fp64 cloud pts.  dict:
         leaves   index arrays (ascending) in list order;  leaf_recs  their mpmath records (mode "mp")
         nnodes   node ellipsoids built (see the module docstring);  depth  of the deepest built node
         nodes    one dict per k-means node in pre-order: m, depth, n0, code, moving, empty, accdesc (a rejected node
                  with an accepted split below it), label_margin, and in mode "mp" the ratios margin / bound
                  label_ratio, accept_margin, accept_ratio, order_ratio"""
    pts = np.asarray(pts, dtype=np.float64)
    n, d = pts.shape
    with_bounds = mode == "mp"
    root_scale, eps_s = scale_of(pts, rules.ddof)
    state = dict(nnodes=1, depth=0)
    knodes = []

    def build(idx, handed):
        e = node_ellipsoid(pts[idx], mode)
        e["idx"] = idx
        e["b"] = node_bounds(pts[idx], e, handed) if with_bounds else None
        return e

    def rec(e, depth):
        """-> (list of leaf ellipsoids, True if a split was accepted in this subtree)"""
        idx = e["idx"]
        m = len(idx)
        state["depth"] = max(state["depth"], depth)
        min_size = 2 * d + rules.min_size_add
        if m < 4 * d + rules.split_add:
            return [e], False
        sub = pts[idx]
        axis, axis_b, order_ratio = major_axis(e, e["b"])
        if rules.flip_sign:
            axis = -axis
        if rules.node_scale:
            scale, es = scale_of(sub, rules.ddof)
        else:
            scale, es = root_scale, eps_s
        if not rules.use_scale:
            scale, es = np.ones(d, dtype=LD), 0.0
        y = H.ld(sub) / scale
        seeds = np.stack([e["mu"] - axis, e["mu"] + axis]) / scale
        seed_b = None
        if with_bounds:
            s64 = scale.astype(np.float64)
            seed_b = (e["b"]["ctr"] + axis_b) / s64 + 2 * EPS * np.max(np.abs(seeds), axis=0).astype(np.float64)
        lab, st = lloyd(y, seeds, rules, seed_b, es)
        node = dict(m=m, depth=depth, n0=int(np.sum(lab == 0)), code=TOO_SMALL, moving=st["moving"], empty=st["empty"],
                    accdesc=False, label_margin=st["margin"], label_ratio=st["ratio"], accept_margin=math.nan,
                    accept_ratio=math.inf, order_ratio=order_ratio)
        knodes.append(node)
        parts = [idx[lab == 0], idx[lab == 1]]
        if min(len(parts[0]), len(parts[1])) < min_size:
            return [e], False
        state["nnodes"] += 2
        kids = [build(parts[0], True), build(parts[1], True)]
        out0, a0 = rec(kids[0], depth + 1)
        out1, a1 = rec(kids[1], depth + 1)
        out = out0 + out1
        mm = n if rules.dec_from_root else m
        dec = LD((d * (d + 3)) // 2) * np.log(LD(mm)) / LD(mm)
        first = np.logaddexp(kids[0]["lnv"], kids[1]["lnv"]) - e["lnv"] + dec
        second = _lse([k["lnv"] for k in out]) - e["lnv"] + dec * (len(out) - rules.len_minus)
        if rules.first_only:
            second = LD(math.inf)
        accept = bool(first < 0 or second < 0)
        if with_bounds:
            mag = 8 * EPS * (abs(float(e["lnv"])) + max(abs(float(k["lnv"])) for k in out + kids) + float(dec) * len(out))
            b1 = kids[0]["b"]["lnv"] + kids[1]["b"]["lnv"] + e["b"]["lnv"] + mag
            b2 = sum(k["b"]["lnv"] for k in out) + e["b"]["lnv"] + mag
            if accept:
                node["accept_margin"] = float(max(-first, -second))
                node["accept_ratio"] = float(max(-first / b1, -second / b2))
            else:
                node["accept_margin"] = float(min(first, second))
                node["accept_ratio"] = float(min(first / b1, second / b2))
        else:
            node["accept_margin"] = float(max(-first, -second) if accept else min(first, second))
        if accept:
            node["code"] = ACCEPT_FIRST if first < 0 else ACCEPT_SECOND
            return out, True
        node["code"] = REJECTED
        node["accdesc"] = bool(a0 or a1)
        return [e], False

    root = build(np.arange(n), False)
    leaves, _ = rec(root, 0)
    return dict(leaves=[e["idx"] for e in leaves], leaf_recs=[e["rec"] for e in leaves], leaf_ells=leaves,
                nnodes=state["nnodes"], depth=state["depth"], nodes=knodes)


def signature(tree, n):
    """What a wrong rule must change: (leaf of every point in list order, nnodes)."""
    lab = np.full(n, -1, dtype=np.int64)
    for i, ix in enumerate(tree["leaves"]):
        lab[ix] = i
    return lab.tobytes(), tree["nnodes"]


# =========================================================================================================
# the fixture (tools/make_golden.py split_hp writes it; tests/test_split_hp_cpu.py regenerates the low dimensions)
# =========================================================================================================
_NODE_FIELDS = (("m", np.int32), ("depth", np.int16), ("n0", np.int32), ("code", np.int8), ("moving", np.int8),
                ("empty", np.int8), ("accdesc", np.int8), ("label_margin", np.float64), ("label_ratio", np.float64),
                ("accept_margin", np.float64), ("accept_ratio", np.float64), ("order_ratio", np.float64))
_LEAF_FIELDS = ("lam_hi", "lam_lo", "lnv", "fmax", "margins", "good", "trials")


def case_record(key):
    """The fixture arrays of one case of tests/split_cases.py: results only, every array one-dimensional."""
    pts = SC.points(key)
    n, d = pts.shape
    tree = split_tree_ref(pts, "mp")
    lab = np.full(n, -1, dtype=np.int16)
    for i, ix in enumerate(tree["leaves"]):
        lab[ix] = i
    out = {"labels": lab, "head": np.array([len(tree["leaves"]), tree["nnodes"], tree["depth"]], dtype=np.int32)}
    recs = [H.fixture_record(r, cov_scale=r["mult"]) for r in tree["leaf_recs"]]
    for name in _LEAF_FIELDS:
        out["leaf_" + name] = np.concatenate([np.atleast_1d(r[name]).ravel() for r in recs])
    out["leaf_lam_lo"] = out["leaf_lam_lo"].astype(np.float32)
    for name, dt in _NODE_FIELDS:
        out["node_" + name] = np.array([nd[name] for nd in tree["nodes"]], dtype=dt)
    return out


def pack_fixture(records, keys):
    """{key: {name: 1-D array}} -> {name: the cases end to end, name + '@': their lengths}, in the order of keys."""
    g = {}
    for name in records[keys[0]]:
        g[name] = np.concatenate([records[k][name] for k in keys])
        g[name + "@"] = np.array([len(records[k][name]) for k in keys], dtype=np.int32)
    return g


def unpack_fixture(g, keys, prefix=""):
    names = [f[len(prefix):] for f in g.files if f.startswith(prefix) and not f.endswith("@")]
    out = {k: {} for k in keys}
    for name in names:
        at = np.concatenate([[0], np.cumsum(g[prefix + name + "@"])])
        assert len(at) == len(keys) + 1, "tests/golden/split_hp.npz does not belong to this list of cases: regenerate it"
        for i, k in enumerate(keys):
            out[k][name] = g[prefix + name][at[i]:at[i + 1]]
    return out


FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_hp.npz")


def load_fixture(path=None):
    """({key: arrays} of the split cases, {key: arrays} of the bootstrap cases) from tests/golden/split_hp.npz."""
    g = np.load(path or FIXTURE)
    return (unpack_fixture(g, SC.KEYS, "split/"), unpack_fixture(g, [c[0] for c in SC.BOOT_CASES], "boot/"))


def leaf_record(fx, i, d):
    """The i-th leaf's record of a case in the layout of ell_hp_ref.fixture_record."""
    return dict(lam_hi=fx["leaf_lam_hi"][i * d:(i + 1) * d], lam_lo=fx["leaf_lam_lo"][i * d:(i + 1) * d],
                lnv=fx["leaf_lnv"][2 * i:2 * i + 2], fmax=np.float64(fx["leaf_fmax"][i]),
                margins=fx["leaf_margins"][4 * i:4 * i + 4], good=np.int32(fx["leaf_good"][i]),
                trials=np.int32(fx["leaf_trials"][i]))


def decidability(fx):
    """The smallest margin / bound over every decision of every node of a case."""
    return float(min([math.inf] + list(fx["node_label_ratio"]) + list(fx["node_accept_ratio"])
                     + list(fx["node_order_ratio"])))


def statistics(fx, d):
    """The table's columns of one case, from the fixture."""
    code = fx["node_code"]
    m, n0 = fx["node_m"], fx["node_n0"]
    small = np.minimum(n0, m - n0)
    return dict(nells=int(fx["head"][0]), nnodes=int(fx["head"][1]), depth=int(fx["head"][2]), kmeans=len(code),
                first=int(np.sum(code == ACCEPT_FIRST)), second=int(np.sum(code == ACCEPT_SECOND)),
                rejected=int(np.sum(code == REJECTED)), accdesc=int(np.sum(fx["node_accdesc"])),
                too_small=int(np.sum(code == TOO_SMALL)), moving=int(np.sum(fx["node_moving"])),
                empty=int(np.sum(fx["node_empty"])), label_margin=float(np.min(fx["node_label_margin"], initial=math.inf)),
                accept_margin=float(np.nanmin(np.abs(np.append(fx["node_accept_margin"], math.inf)))),
                smallest_child=small, multipart=int(np.sum(m > SC.part_points(d))))


# =========================================================================================================
# bootstrap expansion (dh_bootstrap_expand)
# =========================================================================================================
def boot_masks(n, ent, nboot):
    """The in-sample masks of the replicas: NumPy's Generator.integers on the streams oracle/nested_ref.py::
    boot_generator defines, with the reference's two repairs (both decided on the count before either is applied)."""
    from oracle.nested_ref import boot_generator
    out = []
    for b in range(nboot):
        idxs = boot_generator(ent, b).integers(n, size=n)
        sel = np.zeros(n, dtype=bool)
        sel[np.unique(idxs)] = True
        n_in = int(sel.sum())
        if n_in < 2:
            sel[:2] = True
        if n_in > n - 1:
            sel[0] = False
        out.append(sel)
    return out


def boot_points(key):
    _, f, d, n, _ = next(c for c in SC.BOOT_CASES if c[0] == key)
    x = SC.cloud(f, d, n)
    x.setflags(write=False)
    return x


def expand2_with_own_ellipsoids(pout, ctrs, ams):
    """max over the left-out points of the min over ellipsoids of the long-double quadratic form with the EVALUATOR'S
    centres and precision matrices, and the bound of an fp64 evaluation of it: max and min are 1-Lipschitz in the
    maximum norm, so the largest quadform_bound of any (point, ellipsoid) pair that can take part -- all of them."""
    d = pout.shape[1]
    qs, bs = [], []
    for c, a in zip(ctrs, ams):
        q, sabs = H.quadforms_ld(pout, c, a)
        qs.append(q)
        bs.append(H.quadform_bound(d, sabs))
    q, b = np.array(qs), np.array(bs)
    lo = np.max(np.min(q - b, axis=0))
    hi = np.max(np.min(q + b, axis=0))
    val = np.max(np.min(q, axis=0))
    return val, float(max(hi - val, val - lo))


def _expand2_ref(pout, ells):
    """The fully high-precision value (reference ellipsoids `ells` of the in-sample points) and what an fp64
    evaluator's may differ by.  For one (point, ellipsoid) pair, with delta = x - c, A the true precision matrix, the
    evaluator's A^ = (I + R) C^^-1, ||R|| <= inverse_bound, C^ = C + E, ||E|| <= the covariance's and the rescaling's
    error, and its centre within e:
        |q^ - q| <= quadform_bound + 1.1 (|delta| |A delta| ||R|| + |A delta|^2 ||E|| + 2 |A delta| . e)
    (first order; the factor 1.1 covers the products of the small terms).  Through min and max by their monotonicity:
    min_e q^ <= q^[e*] with e* the reference's argmin, and >= min_e (q - b); likewise for the max over points.  No
    argmax has to be decidable."""
    d = pout.shape[1]
    qs, bs = [], []
    for e in ells:
        b = e["b"]
        cfin = e["cov"] * e["mult"]
        am = H.ld_solve(cfin, np.eye(d, dtype=LD))
        q, sabs = H.quadforms_ld(pout, e["mu"], am)
        dl = H.ld(pout) - e["mu"]
        adl = dl @ am
        kappa = float(b["lam"][-1] / b["lam"][0])
        err_c = b["sb"] + b["mb"] * H.fro(cfin)
        nd = np.sqrt(np.sum(dl * dl, axis=1)).astype(np.float64)
        na = np.sqrt(np.sum(adl * adl, axis=1)).astype(np.float64)
        bound = H.quadform_bound(d, sabs) + 1.1 * (nd * na * H.inverse_bound(d, kappa) + na * na * err_c
                                                    + 2 * (np.abs(adl).astype(np.float64) @ b["ctr"]))
        qs.append(q)
        bs.append(bound)
    q, b = np.array(qs), np.array(bs)
    star = np.argmin(q, axis=0)
    col = np.arange(q.shape[1])
    qmin = q[star, col]
    beta = np.maximum(b[star, col], (qmin - np.min(q - b, axis=0)).astype(np.float64))
    val = qmin.max()
    return val, float(max(np.max(qmin + beta) - val, val - np.max(qmin - beta)))


def boot_record(key):
    """The fixture arrays of one bootstrap case: per replica the in-sample count, the reference's squared expansion
    (max over left-out points of min over ellipsoids), its bound, the number of ellipsoids and the smallest
    decidability ratio of the replica's tree."""
    _, f, d, n, multi = next(c for c in SC.BOOT_CASES if c[0] == key)
    pts = boot_points(key)
    nin, q2, q2b, nells, dec = [], [], [], [], []
    for sel in boot_masks(n, SC.boot_entropy(key), SC.BOOT_B):
        pin, pout = pts[sel], pts[~sel]
        if multi:
            tree = split_tree_ref(pin, "mp")
            ells = tree["leaf_ells"]
            ratios = [math.inf] + [nd[k] for nd in tree["nodes"] for k in ("label_ratio", "accept_ratio", "order_ratio")]
            dec.append(min(ratios))
        else:
            e = node_ellipsoid(pin, "mp")
            e["b"] = node_bounds(pin, e, False)
            ells = [e]
            dec.append(math.inf)
        val, bound = _expand2_ref(pout, ells)
        nin.append(int(sel.sum()))
        q2.append(float(val))
        q2b.append(bound + 2 * EPS * float(val))
        nells.append(len(ells))
    return dict(nin=np.array(nin, dtype=np.int32), q2=np.array(q2), q2b=np.array(q2b),
                nells=np.array(nells, dtype=np.int32), decid=np.array(dec))


# =========================================================================================================
# the checker, shared by the float64 oracle (tests/test_split_hp_cpu.py) and the device (tests/test_gpu_split_hp.py)
# =========================================================================================================
def check_tree(pts, got, fx, what, canonical=True, logvol_from_spectrum=True):
    """One MultiEllipsoid.update of pts -- got: dict(nells, nnodes, labels, ctrs, covs, ams, axes, axlens,
    logvol_ells) -- against the case's fixture fx: nells, nnodes and the leaf of every point IN LIST ORDER exact;
    every leaf ellipsoid through ell_hp_ref.check_bounding against its own leaf's record; every point inside the
    union by more than the quadratic form's bound.  Returns the worst Ratios."""
    n, d = pts.shape
    assert got["nells"] == int(fx["head"][0]), f"{what}: nells = {got['nells']}, the reference has {int(fx['head'][0])}"
    assert got["nnodes"] == int(fx["head"][1]), f"{what}: nnodes = {got['nnodes']}, the reference has {int(fx['head'][1])}"
    lab = np.asarray(got["labels"])
    if not np.array_equal(lab, fx["labels"]):
        same_sets = {frozenset(np.flatnonzero(lab == i).tolist()) for i in range(got["nells"])} == \
            {frozenset(np.flatnonzero(fx["labels"] == i).tolist()) for i in range(got["nells"])}
        raise AssertionError(f"{what}: the leaves differ from the reference's "
                             + ("in ORDER only" if same_sets else f"in {int(np.sum(lab != fx['labels']))} points"))
    worst = H.Ratios()
    qmin = np.full(n, np.inf, dtype=LD)
    qb = np.zeros(n)
    for i in range(got["nells"]):
        out = dict(ctr=got["ctrs"][i], cov=got["covs"][i], am=got["ams"][i], axes=got["axes"][i],
                   axlens=got["axlens"][i], logvol=got["logvol_ells"][i])
        worst.merge(H.check_bounding(pts[lab == i], out, leaf_record(fx, i, d), f"{what} leaf {i}", canonical=canonical,
                                     logvol_from_spectrum=logvol_from_spectrum))
        q, sabs = H.quadforms_ld(pts, got["ctrs"][i], got["ams"][i])
        better = q < qmin
        qmin = np.where(better, q, qmin)
        qb = np.where(better, H.quadform_bound(d, sabs), qb)
    assert np.all(qmin < 1 - qb), f"{what}: {int(np.sum(~(qmin < 1 - qb)))} point(s) not inside the union by their bound"
    return worst
