"""tests/friends_hp_ref.py without a device: the bounds are neither wrong nor vacuous.

  * the fixture tests/golden/friends_hp.npz is what the generator produces now (the cases with d <= 8);
  * two independent float64 implementations stay at HALF of every bound or less on every case: the oracle's route
    (oracle/friends_ref.py: scipy's pdist / single linkage, pinvh, sqrtm, KD-tree radii) and a restatement around a
    textbook Jacobi (Golub & Van Loan's rotation in the parallel ordering, vectorised per round) with brute-force
    radii -- the calibration friends_hp_ref names; the row-cyclic Jacobi of tests/test_ell_hp_cpu.py, a Python loop
    over the pairs, runs on every case with d <= 8 and on ROW_CYCLIC_LARGE;
  * nine degraded restatements are refused: eight miss a bound by the factor printed, the bit row without its last
    word fails the exact comparison;
  * every cap holds for the reference alone: all partitions decided by more than 1e-6, at most 2 % of a case's probes
    undecided (the 1e-9 ring of the width-1e-7 cloud apart, which is reported), every succeeding case a factor 30
    above pinvh's cutoff and every failing one exactly singular;
  * how far the bounds undercut the 2e-10 / 1e-9 / 1e-11 of tests/test_gpu_friends.py.
"""
import math
import os

import numpy as np
import pytest
from scipy import linalg as sla
from scipy import spatial

import friends_cases as FC
import friends_hp_ref as R
from ell_hp_ref import Ratios
from oracle import friends_ref as F
from test_ell_hp_cpu import _jacobi_textbook

EPS64 = 2.220446049250313e-16  # scipy's (and the kernels') eps in the pinvh cutoff
_EIG = {}
# the large cases that also take the row-cyclic Jacobi of tests/test_ell_hp_cpu.py (every case with d <= 8 does)
ROW_CYCLIC_LARGE = ("iso/33/64/c", "tail/60/1025/c")


def _jacobi_parallel(a, tol2=1e-31):
    """Cyclic Jacobi in float64 with the textbook rotation (Golub & Van Loan 8.5.2: theta, t, c = 1 / sqrt(1 + t^2),
    s = t c) in the parallel ordering of 8.5.5: a round of the round-robin tournament rotates floor(d / 2) disjoint
    pairs, which commute, so a round is a handful of NumPy calls and a 64 x 64 matrix takes a tenth of a second where
    the row-cyclic loop of tests/test_ell_hp_cpu.py takes two.  Until off^2 <= tol2 dia^2.  Nothing of csrc/ is in it."""
    a = np.array(a, dtype=np.float64)
    d = a.shape[0]
    v = np.eye(d)
    players = np.arange(d + d % 2)  # (the last one is a bye when d is odd)
    half = len(players) // 2
    sweeps = 0
    for sweeps in range(60):
        if d < 2 or not 2 * np.sum(np.triu(a, 1)**2) > tol2 * np.sum(np.diag(a)**2):
            break
        for _ in range(len(players) - 1):
            p, q = np.minimum(players[:half], players[:half - 1:-1]), np.maximum(players[:half], players[:half - 1:-1])
            players[1:] = np.concatenate([players[-1:], players[1:-1]])
            p, q = p[q < d], q[q < d]
            apq = a[p, q]
            live = apq != 0.0
            theta = (a[q, q] - a[p, p]) / np.where(live, 2 * apq, 1.0)
            t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1))
            c = np.where(live, 1 / np.sqrt(t * t + 1), 1.0)
            sn = np.where(live, t, 0.0) * c
            for m in (a, v):
                x, y = m[:, p].copy(), m[:, q].copy()
                m[:, p], m[:, q] = c * x - sn * y, sn * x + c * y
            x, y = a[p].copy(), a[q].copy()
            a[p], a[q] = c[:, None] * x - sn[:, None] * y, sn[:, None] * x + c[:, None] * y
            a[p[live], q[live]] = a[q[live], p[live]] = 0.0
    return np.diag(a).copy(), v, sweeps


def _jacobi(cov, solver):
    """One decomposition per matrix and solver (both kinds take the shape of one cloud)."""
    key = (cov.tobytes(), solver.__name__)
    if key not in _EIG:
        _EIG[key] = solver(cov)
    return _EIG[key]


@pytest.fixture(scope="module")
def fix():
    return R.load_fixture()


def _inputs(case):
    key, name, d, n, clustering, spec, fails = case
    return FC.cloud(name, d, n), (FC.prev_metric(name, d, n) if clustering else None), FC.masks(spec, n)


# ---- float64 implementation 1: the oracle's route ---------------------------------------------------------------------
def _kd_radius(y, kind, masks):
    p = 2 if kind == "balls" else np.inf
    if masks is None:
        return float(max(spatial.KDTree(y).query(y, k=2, eps=0, p=p)[0][:, 1]))
    best = -np.inf
    for mk in masks:
        if not (~mk).any():
            continue
        best = max(best, float(max(spatial.KDTree(y[mk]).query(y[~mk], k=1, eps=0, p=p)[0])))
    return best


_COV = {}


def oracle_update(pts, kind, prev, masks):
    d = pts.shape[1]
    key = (pts.tobytes(), prev is None)  # (both kinds take the covariance of one cloud: scipy's pdist once)
    if key not in _COV:
        _COV.clear()
        _COV[key] = F.covariance_from_clusters(pts, prev) if prev is not None else (np.cov(pts, rowvar=False), 1)
    cov, ncl = _COV[key]
    cov = np.atleast_2d(cov)
    am, axes = sla.pinvh(cov), np.atleast_2d(sla.sqrtm(cov))
    axes_inv = sla.pinvh(axes)
    r = _kd_radius(pts @ axes_inv, kind, masks)
    am_s = am / r**2
    return dict(cov=cov * r**2, am=am_s, axes=axes * r, axes_inv=axes_inv / r, rmax=r, nclusters=ncl,
                logvol=F.shape_logvol(kind, d, am_s))


# ---- float64 implementation 2: textbook Jacobi, brute force, with the flaws of the degraded restatements ---------------
def _nn_radius(y, kind, masks, flaw=None):
    n = len(y)
    dist = spatial.distance.cdist(y, y, "euclidean" if kind == "balls" else "chebyshev")  # every pair, difference first
    ncand = 64 * (n // 64) if flaw == "nn_skip_tail" else n
    best = -np.inf
    for mk in ([None] if masks is None else masks):
        if mk is None:
            ok = np.ones((n, n), dtype=bool)
            if flaw != "nn_self":
                np.fill_diagonal(ok, False)
            rows = np.arange(n)
        else:
            mk = ~mk if flaw == "nn_invert_mask" else mk
            ok = np.broadcast_to(mk[None, :], (n, n)).copy()
            rows = np.flatnonzero(~mk)
        ok[:, ncand:] = False
        if len(rows):
            best = max(best, float(np.where(ok, dist, np.inf)[rows].min(axis=1).max()))
    return best


def jacobi_update(pts, kind, labels, masks, flaw=None, solver=_jacobi_parallel):
    n, d = pts.shape
    x = pts
    if len(np.unique(labels)) > 1:
        x = pts.copy()
        for c in np.unique(labels):
            x[labels == c] -= pts[labels == c].mean(axis=0)
    ddof = 0 if flaw == "ddof0" else 1
    if flaw == "one_pass":
        mu = x.mean(axis=0)
        cov = (x.T @ x / n - np.outer(mu, mu)) * (n / (n - 1.0))
    elif flaw == "cov_f32":
        dm = x - x.mean(axis=0)
        cov = (dm[:, :, None] * dm[:, None, :]).astype(np.float32).sum(axis=0, dtype=np.float32).astype(np.float64) / (n - 1)
    else:
        dm = x - x.mean(axis=0)
        cov = dm.T @ dm / (n - ddof)
    lam, vec, _ = _jacobi(cov, solver)
    order = np.argsort(lam)
    lam, vec = lam[order], vec[:, order]
    top = np.abs(lam).max()
    keep, keep_s = np.abs(lam) > d * EPS64 * top, np.sqrt(np.maximum(lam, 0)) > d * EPS64 * math.sqrt(top)
    if not keep.all():
        raise ValueError("singular covariance")
    root = np.sqrt(lam)
    root_x = root * (1 + 1e-12 * (np.arange(d) == d // 2)) if flaw == "sqrt_eig_off" else root
    am = (vec * np.where(keep, 1 / lam, 0)) @ vec.T
    axes = (vec * root_x) @ vec.T
    axes_inv = (vec * np.where(keep_s, 1 / root, 0)) @ vec.T
    r = _nn_radius(pts @ axes_inv, kind, masks, flaw)
    if not r > 0:  # (the flaw that keeps j == i: DH_ERR_VALUE on the device, nothing to scale here)
        return dict(rmax=r)
    pre = d * math.log(2.0) + (d * math.lgamma(1.5) - math.lgamma(d / 2.0 + 1.0) if kind == "balls" else 0.0)
    return dict(cov=cov * r**2, am=am / r**2, axes=axes * r, axes_inv=axes_inv / r, rmax=r,
                nclusters=len(np.unique(labels)), logvol=pre + 0.5 * np.sum(np.log(lam)) + d * math.log(r))


def _within64(ctrs, axes_inv, x, kind, whiten_first, dtype=np.float64):
    ctrs, axes_inv, x = (a.astype(dtype) for a in (ctrs, axes_inv, x))
    t = (ctrs @ axes_inv)[None, :, :] - (x @ axes_inv)[:, None, :] if whiten_first else \
        (ctrs[None, :, :] - x[:, None, :]) @ axes_inv
    return (np.sqrt((t * t).sum(-1)) if kind == "balls" else np.abs(t).max(-1)).astype(np.float64)


# ---- the tests ---------------------------------------------------------------------------------------------------------
def test_case_list_and_fixture_size(fix):
    cases = FC.update_cases()
    assert {c[2] for c in cases if c[1] == "iso"} == set(FC.DIMS)
    assert {c[3] for c in cases if c[2] == 2} >= set(FC.N_EDGES) and {c[3] for c in cases if c[2] == 60} >= set(FC.N_EDGES)
    assert ("iso", 1, 2) in {c[1:4] for c in cases}
    assert all(c[3] > c[2] for c in cases)
    assert {c[3] for c in FC.within_cases()} == {1, 63, 64, 65, 129} and {c[4] for c in FC.within_cases()} == {1, 63, 65}
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gdir, "friends_hp.npz"))
    assert all(g[k].dtype.kind in "fi" for k in g.files)
    assert os.path.getsize(os.path.join(gdir, "friends_hp.npz")) < os.path.getsize(os.path.join(gdir, "ell_hp.npz"))


def test_fixture_is_what_the_generator_produces(fix):
    urec, wrec = fix
    n = 0
    for case in FC.update_cases():
        if case[2] > 8 or case[3] > 257:
            continue
        now, then = R.update_record(case[0]), urec[case[0]]
        assert sorted(now) == sorted(then), case[0]
        for name in now:
            np.testing.assert_array_equal(now[name], then[name], err_msg=f"{case[0]}/{name}")
        n += 1
    for case in FC.within_cases():
        if case[2] > 3:
            continue
        for kind in FC.KINDS:
            for a, b in zip(R.within_record(case[0], kind), wrec[(case[0], kind)]):
                np.testing.assert_array_equal(a, b, err_msg=f"{case[0]}/{kind}")
            n += 1
    print(f"friends_hp fixture: {n} cases regenerated and equal")
    assert n >= 40


def test_two_float64_implementations_stay_at_half_of_every_bound(fix):
    urec, _ = fix
    worst = {"oracle": Ratios(), "jacobi": Ratios(), "jacobi_row_cyclic": Ratios()}
    where = {}
    for case in FC.update_cases():
        key, name, d, n, clustering, spec, fails = case
        pts, prev, masks = _inputs(case)
        rec = urec[key]
        for kind in FC.KINDS:
            impls = {"oracle": lambda: oracle_update(pts, kind, prev, masks),
                     "jacobi": lambda: jacobi_update(pts, kind, rec["labels"], masks)}
            if d <= 8 or key in ROW_CYCLIC_LARGE:  # (a Python loop over the pairs: two seconds at d = 60)
                impls["jacobi_row_cyclic"] = lambda: jacobi_update(pts, kind, rec["labels"], masks,
                                                                   solver=_jacobi_textbook)
            for impl, run in impls.items():
                if fails:
                    with pytest.raises(ValueError):
                        run()
                    continue
                r = R.check_update(pts, kind, masks, run(), rec, rec["labels"])
                for k, v in r.items():
                    if v > worst[impl].get(k, 0.0):
                        where[(impl, k)] = f"{key}/{kind}"
                worst[impl].merge(r)
    for impl, r in worst.items():
        R.report(r, f"FLOAT64 {impl} worst error / bound")
        print("    at " + "  ".join(f"{k}: {where[(impl, k)]}" for k in r))
        bad = {k: (v, where[(impl, k)]) for k, v in r.items() if not v <= 0.5}
        assert not bad, f"{impl} is above half of a bound: {bad}"


@pytest.mark.parametrize("kind", FC.KINDS)
def test_membership_bound_holds_for_both_float64_routes(fix, kind):
    """Subtract-then-whiten (the oracle's friends_within) and whiten-then-subtract in float64: the distance of every
    pair within half of its decision bound; all caps on the undecided probes."""
    _, wrec = fix
    worst = Ratios()
    for key, name, d, n, m in FC.within_cases():
        w = FC.within_inputs(name, d, n, m, kind)
        gap, bound = R.within_reference(w["ctrs"], w["axes_inv"], w["x"], kind, wrec[(key, kind)])
        for route, first in (("subtract_first", False), ("whiten_first", True)):
            dist = _within64(w["ctrs"], w["axes_inv"], w["x"], kind, first)
            worst.add(route, np.max(np.abs((dist - 1.0) - gap) / bound), 1.0)
        # the oracle's own answer on every decided probe; the caps
        fr = F.Friends(kind, None, None, w["axes"], w["axes_inv"], 0.0, w["ctrs"])
        decided = np.all(np.abs(gap) > bound, axis=1)
        for p in np.flatnonzero(decided):
            assert np.array_equal(F.friends_within(fr, w["x"][p]), np.flatnonzero(gap[p] <= 0)), (key, p)
        free = (np.abs(w["ring"]) <= 1e-9) & (w["ring"] != 0) if name == "late" else np.zeros(m, dtype=bool)
        share = float(np.mean(~decided & ~free))
        assert share <= 0.02, (key, kind, share, np.flatnonzero(~decided & ~free))
        if name == "late":
            own = np.abs(gap).min(axis=1)
            print(f"friends_hp MEMBERSHIP {key}/{kind}: decision distance median {np.median(bound.min(axis=1)):.3g} "
                  f"max {bound.max():.3g}; undecided on the 1e-9 ring {int(np.sum(~decided & free))} of {int(free.sum())}; "
                  f"ring gaps reached {np.sort(own[w['ring'] != 0])[:3]}")
        # the ring probes are where they were aimed: a shape's surface within the offset (another centre's may be nearer)
        for off in (1e-3, 1e-6, 1e-9):
            sel = np.abs(w["ring"]) == off
            if sel.any() and (name != "late" or off > 1e-9):
                own = np.abs(gap[sel]).min(axis=1)
                assert np.all(own < off * (1 + 1e-3)) and np.median(own) > off * (1 - 1e-3), (key, kind, off, own)
    R.report(worst, f"FLOAT64 membership {kind} worst distance error / decision bound")
    assert all(v <= 0.5 for v in worst.values()), worst


def _factor(r):
    return max(r.values())


def test_degraded_restatements_miss_a_bound(fix):
    urec, wrec = fix
    shown = {}

    def upd(key, kind, flaw):
        case = {c[0]: c for c in FC.update_cases()}[key]
        pts, prev, masks = _inputs(case)
        rec = urec[key]
        good = R.check_update(pts, kind, masks, jacobi_update(pts, kind, rec["labels"], masks), rec, rec["labels"])
        assert _factor(good) <= 0.5, (key, good)
        out = jacobi_update(pts, kind, rec["labels"], masks, flaw)
        if not out["rmax"] > 0:
            return math.inf, "rmax"  # a zero radius is DH_ERR_VALUE, not a result
        r = R.check_update(pts, kind, masks, out, rec, rec["labels"])
        worst = max(r, key=r.get)
        return r[worst], worst

    shown["float32 accumulator in the covariance"] = upd("iso/8/255/c/boot5", "balls", "cov_f32")
    shown["one-pass covariance"] = upd("late/3/130/c", "balls", "one_pass")
    shown["ddof = 0"] = upd("iso/8/255/c/boot5", "cubes", "ddof0")
    shown["square root with one eigenvalue off by 1e-12"] = upd("iso/8/10", "balls", "sqrt_eig_off")
    shown["nearest neighbour without the last partial tile"] = upd("tail/2/65/c", "balls", "nn_skip_tail")
    shown["nearest neighbour without the last partial tile (replicas)"] = upd("iso/8/255/c/boot5", "cubes", "nn_skip_tail")
    shown["nearest neighbour that keeps j == i"] = upd("iso/2/4", "balls", "nn_self")
    shown["nearest neighbour with the mask inverted"] = upd("iso/2/256/c/single", "cubes", "nn_invert_mask")
    # membership: a row that drops its last word, and float32 whiten-then-subtract
    for key, kind in (("w/iso/1/65/65", "balls"), ("w/iso/3/129/63", "cubes")):
        case = {c[0]: c for c in FC.within_cases()}[key]
        w = FC.within_inputs(*case[1:], kind)
        gap, bound = R.within_reference(w["ctrs"], w["axes_inv"], w["x"], kind, wrec[(key, kind)])
        n = case[3]
        inside = _within64(w["ctrs"], w["axes_inv"], w["x"], kind, True) <= 1.0
        bits = np.packbits(np.pad(inside, ((0, 0), (0, 64 * ((n + 63) // 64) - n))), axis=1, bitorder="little").view(np.uint64)
        R.check_within(inside.sum(axis=1), bits, gap, bound, w["ring"], key)
        lost = bits.copy()
        lost[:, -1] = 0
        with pytest.raises(AssertionError):
            R.check_within(inside.sum(axis=1), lost, gap, bound, w["ring"], key)
        nwrong = int(np.sum(bits[:, -1] != 0))
        print(f"friends_hp DEGRADED membership row without its last word ({key}): {nwrong} probes with a wrong row, "
              "refused by check_within")
        assert nwrong > 0
        d32 = _within64(w["ctrs"], w["axes_inv"], w["x"], kind, True, np.float32)
        shown[f"float32 whiten-then-subtract ({key})"] = (float(np.max(np.abs((d32 - 1.0) - gap) / bound)), "distance")
    for name, (factor, what) in shown.items():
        print(f"friends_hp DEGRADED {name}: {factor:.3g} x bound ({what})")
    for name, (factor, what) in shown.items():
        assert factor > 3.0, f"{name} passes (error / bound = {factor:.3g}, {what})"


def test_caps_hold_for_the_reference_alone(fix):
    urec, _ = fix
    nclustered = 0
    for key, name, d, n, clustering, spec, fails in FC.update_cases():
        rec = urec[key]
        if clustering:
            assert rec["margin"] > 1e-6, (key, rec["margin"])  # the partition is decided
            want = {"blobs2": 2, "blobs5": 5}.get(name, 1)
            assert int(rec["ncl"]) == want, (key, int(rec["ncl"]))
            nclustered += want > 1
        pts = FC.cloud(name, d, n)
        if fails:  # exactly singular: a zero row and column, no rounding involved
            _, cov = R.cov_of_points_ld(R.recentred_ld(pts, rec["labels"]))
            assert np.all(cov[-1] == 0) and np.all(cov[:, -1] == 0), key
            continue
        lam = R.lam_of(rec).astype(np.float64)
        assert lam[0] > 30 * d * EPS64 * lam[-1], (key, lam[0] / lam[-1])  # pinvh(cov) keeps everything ...
        assert math.sqrt(lam[0]) > 30 * d * EPS64 * math.sqrt(lam[-1]), key  # ... and so does pinvh(sqrtm(cov))
        b, cov = R.friends_cov_bound(pts, rec["labels"])
        sb = R.H.spectrum_bound(cov.astype(np.float64), R.fro(b))
        assert sb < 0.25 * lam[0], (key, sb / lam[0])  # every eigenvalue a ln V bound divides by is determined
        if name.startswith("corr"):
            k = float(name[4:])
            assert 0.5 * k < lam[-1] / lam[0] < 2 * k, (key, lam[-1] / lam[0])
    assert nclustered == 6
    for spec, n in (("full1of5", 255), ("single", 256), ("tile64", 65), ("tile64", 1025), ("block256", 257)):
        m = FC.masks(spec, n)
        out = [np.flatnonzero(~row) for row in m]
        if spec == "full1of5":
            assert len(out[2]) == 0 and all(len(o) for i, o in enumerate(out) if i != 2)
        if spec == "single":
            assert len(out[0]) == 1
        if spec == "tile64":
            assert len(out[0]) and out[0].min() >= 64 * ((n - 1) // 64)
        if spec == "block256":
            assert len(out[0]) and out[0].min() >= 256 * ((n - 1) // 256)


def test_bounds_undercut_the_hand_set_tolerances(fix):
    """tests/test_gpu_friends.py compares matrices at 2e-10 max|golden|, ln V at 1e-9 and the radius at 1e-11 r: the
    derived bounds of the same quantities on the isotropic cases (the only kind of cloud that file has)."""
    urec, _ = fix
    worst = {}
    for key, name, d, n, clustering, spec, fails in FC.update_cases():
        if name != "iso" or n < 3 * d:
            continue
        pts, _, masks = _inputs((key, name, d, n, clustering, spec, fails))
        rec = urec[key]
        lam = R.lam_of(rec).astype(np.float64)
        b, cov = R.friends_cov_bound(pts, rec["labels"])
        c64 = cov.astype(np.float64)
        sb = R.H.spectrum_bound(c64, R.fro(b))
        o = oracle_update(pts, "balls", None, masks)
        rr = o["rmax"]
        t = {"cov": float(np.max(b)) / (2e-10 * np.abs(c64).max()),
             "axes": R.sqrt_error_bound(R.fro(b) + R.sqrt_residual_bound(c64, o["axes"] / rr), lam[0])
             / (2e-10 * np.sqrt(lam[-1])),
             "logvol": R.logvol_bound(d, sb, lam, float(R.logvol_prefactor_mp(d)), math.lgamma(d / 2 + 1), math.log(rr)) / 1e-9,
             "rmax": R.radius_bound(pts, o["axes_inv"] * rr, d, "balls", rr) / (1e-11 * rr)}
        for k, v in t.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("friends_hp TIGHTNESS derived bound / hand-set tolerance, worst over the isotropic cases: "
          + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v < 1.0 for v in worst.values()), worst


def test_clustering_limit_is_stated_once():
    """The constant of friends.hip, the sentence of include/dynhip.h and the case list name one limit for clustering,
    and it is the largest d whose adjacency tile fits 160 KB of LDS (the message prints the constant:
    tests/test_gpu_friends_hp.py::test_clustering_limit reads it from the device)."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "dynesty_amd", "csrc", "friends.hip")).read()
    hdr = " ".join(open(os.path.join(root, "include", "dynhip.h")).read().replace("*", " ").split())
    limit = int(re.search(r"kFrClusterMaxD\s*=\s*(\d+)", src).group(1))
    assert limit == FC.CLUSTER_DMAX
    assert f"with clustering (am_prev != NULL) d <= {limit}" in hdr

    def lds(d):
        return (d * d + 4 * (d + 64 * d)) * 8
    assert lds(limit) <= 160 * 1024 < lds(limit + 1)
