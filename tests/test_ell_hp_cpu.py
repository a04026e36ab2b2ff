"""tests/ell_hp_ref.py without a device: the bounds are neither wrong nor vacuous.

  * the fixture tests/golden/ell_hp.npz is what the generator produces now (every case with D <= 10);
  * the float64 oracle (oracle.bounding_ref: NumPy / LAPACK) passes every bound on every case -- the worst
    error / bound per bound is printed; a failure here means a derivation is wrong, not a constant too small;
  * degraded restatements (float32 eigen-system, a Jacobi stopped at off^2 <= 1e-20 dia^2, a one-pass covariance,
    a float32 inverse) are rejected;
  * for the flat, kappa = 1e3 and kappa = 1e6 families the derived bounds are below the tolerances the existing
    device tests apply to the same quantities;
  * every decision case has a margin above the uncertainty its own bound gives an fp64 evaluator, so that the device
    test skips none;
  * the membership reference alone puts every boundary point on the intended side.
"""
import math

import numpy as np
import pytest

import ell_cases as EC
import ell_hp_ref as H
from oracle import bounding_ref as B


@pytest.fixture(scope="module")
def fix():
    return H.load_fixture()


@pytest.fixture(autouse=True)
def oracle_with_a_backward_stable_eigh(monkeypatch):
    """The oracle's own routines with LAPACK's divide-and-conquer driver (dsyevd) in place of SciPy's default, the
    MRRR driver dsyevr.  MRRR trades orthogonality for speed inside clusters of eigenvalues: on the clustered spectra
    here (a leading pair 1e-3 apart over seven equal eigenvalues in 9-D) it measures ||U^T U - I|| = 41 and a residual
    29 times C_EIG D eps, where dsyevd and dsyev (QL) stay below 0.4 of it on every case -- so the bound is held
    against the backward-stable drivers, which is what C_EIG's derivation speaks of, and MRRR's figure is evidence
    that it is not loose."""
    import types
    from scipy import linalg as sla
    shim = types.SimpleNamespace(eigh=lambda a, **kw: sla.eigh(a, driver="evd", **kw), LinAlgError=sla.LinAlgError,
                                 norm=sla.norm)
    monkeypatch.setattr(B, "sla", shim)


def _all_clouds():
    return EC.cloud_cases() + EC.wide_cases()


def _oracle_out(pts):
    e = B.bounding_ellipsoid(pts)
    return dict(ctr=e.ctr, cov=e.cov, am=e.am, axes=e.axes, axlens=e.axlens, logvol=e.logvol)


def test_case_list_is_complete(fix):
    keys = H.all_case_keys()
    assert len(keys) == len(set(keys))
    assert sorted(fix) == sorted(keys)
    for d in EC.DIMS + (25,):
        kinds = {c[1] for c in EC.cloud_cases() if c[2] == d}
        assert {"flat", "dup6", "flat@1e-7"} <= kinds
        if d >= 5:
            assert kinds == set(EC.CLOUD_KINDS)
    # numeric arrays only, and smaller than the largest fixture tests/golden/ already holds
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ell_hp.npz"))
    assert all(g[k].dtype.kind in "fi" for k in g.files)
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ell_hp.npz")) < 2**20


def test_fixture_is_what_the_generator_produces(fix):
    n = 0
    for key in H.all_case_keys():
        if int(key.split("/")[1]) > 10:
            continue
        now, then = H.case_record(key), H.fixture_case(fix, key)
        assert sorted(now) == sorted(then), key
        for name in now:
            np.testing.assert_array_equal(now[name], then[name], err_msg=f"{key}/{name}")
        n += 1
    print(f"ell_hp fixture: {n} cases regenerated and equal")
    assert n > 250


def test_float64_oracle_passes_every_bound(fix):
    worst = {"bounding": H.Ratios(), "ell_from_cov": H.Ratios(), "improve_covar_mat": H.Ratios()}
    failures = []

    def take(group, key, r):
        worst[group].merge(r)
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        if bad:
            failures.append((key, bad))

    for key, kind, d, n in _all_clouds():
        pts = EC.cloud(kind, d, n)
        take("bounding", key, H.check_bounding(pts, _oracle_out(pts), H.fixture_case(fix, key), key, canonical=False))
    for d in EC.MAT_DIMS:
        for key, kind in EC.matrix_cases(d):
            a, rec = EC.matrix(kind, d), H.fixture_case(fix, key)
            good, cov, am, axes = B.regularize_cov(a)
            take("improve_covar_mat", key, H.check_improve_covar_mat(a, good, cov, am, axes, rec, canonical=False))
            if EC.is_positive_kind(kind):
                e = B.make_ell(np.zeros(d), a)
                take("ell_from_cov", key, H.check_ell_from_cov(a, e.axes, e.axlens, e.am, e.logvol, rec,
                                                               canonical=False))
    for group, r in worst.items():
        print(f"ell_hp ORACLE worst error / bound, {group}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert not failures, f"the float64 oracle is outside a bound in {len(failures)} case(s): {failures[:6]}"
    # the calibration ell_hp_ref.C_EIG / C_ORTH / C_INV name: LAPACK stays below half of the unproved factors
    for group in worst.values():
        assert max(group["eig_res"], group["orth"]) <= 0.5 and group["inv_res"] <= 0.5


def _jacobi_stopped_early(a, tol2=1e-20):
    """Cyclic Jacobi in float64 that stops as soon as off^2 <= tol2 * dia^2 (checked after every rotation)."""
    a = np.array(a, dtype=np.float64)
    d = a.shape[0]
    v = np.eye(d)
    for _ in range(60):
        for p in range(d - 1):
            for q in range(p + 1, d):
                off2 = np.sum(a * a) - np.sum(np.diag(a)**2)
                if off2 <= tol2 * np.sum(np.diag(a)**2):
                    return np.diag(a).copy(), v
                if a[p, q] == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2 * a[p, q])
                t = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(theta * theta + 1))
                c = 1 / math.sqrt(t * t + 1)
                s = t * c
                j = np.eye(d)
                j[p, p] = j[q, q] = c
                j[p, q], j[q, p] = s, -s
                a = j.T @ a @ j
                v = v @ j
    return np.diag(a).copy(), v


def _jacobi_textbook(a, tol2=1e-31):
    """Cyclic Jacobi in float64 as the textbooks state it (Golub & Van Loan 8.5.2: theta, t, c = 1 / sqrt(1 + t^2),
    s = t c; row-cyclic order; rotations applied to rows, columns and V), until off^2 <= tol2 dia^2.  Nothing of
    csrc/ is in it."""
    a = np.array(a, dtype=np.float64)
    d = a.shape[0]
    v = np.eye(d)
    sweeps = 0
    for sweeps in range(60):
        if not 2 * np.sum(np.triu(a, 1)**2) > tol2 * np.sum(np.diag(a)**2):
            break
        for p in range(d - 1):
            for q in range(p + 1, d):
                if a[p, q] == 0.0:
                    continue
                theta = (a[q, q] - a[p, p]) / (2 * a[p, q])
                t = math.copysign(1.0, theta) / (abs(theta) + math.sqrt(theta * theta + 1))
                c = 1 / math.sqrt(t * t + 1)
                s = t * c
                for m, ax in ((a, 0), (a, 1), (v, 1)):
                    x, y = np.take(m, p, axis=ax).copy(), np.take(m, q, axis=ax).copy()
                    if ax == 0:
                        m[p], m[q] = c * x - s * y, s * x + c * y
                    else:
                        m[:, p], m[:, q] = c * x - s * y, s * x + c * y
                a[p, q] = a[q, p] = 0.0
    return np.diag(a).copy(), v, sweeps


def test_textbook_jacobi_stays_below_half_of_the_eigen_bounds():
    """The calibration ell_hp_ref.C_EIG and C_ORTH name, for the solver class the kernels belong to: a converged
    textbook Jacobi stays below half of the residual and the orthogonality bound -- and is ABOVE 8 D eps in
    orthogonality at D = 43, which is why that bound grows like D^1.5 (column norms drift with the number of
    rotations a column takes part in)."""
    worst = H.Ratios()
    above_linear = 0.0
    for d in (25, 43):
        for kind in ("flat", "geo1e6", "geo1e11", "gap1e-12"):
            cov = np.cov(EC.cloud(kind, d), rowvar=False)
            lam, vec, sweeps = _jacobi_textbook(cov)
            order = np.argsort(lam)
            lam, vec = lam[order], vec[:, order]
            r = H.Ratios()
            r.add("eig_res", H.fro(H.ld(cov) - (H.ld(vec) * H.ld(lam)) @ H.ld(vec).T), H.eig_residual_bound(cov))
            g = H.fro(H.ld(vec).T @ H.ld(vec) - np.eye(d))
            r.add("orth", g, H.orth_bound(d))
            print(f"ell_hp JACOBI {d}/{kind}: {sweeps} sweeps  " + "  ".join(f"{k} {x:.3g}" for k, x in r.items())
                  + f"  orth / (8 D eps) {g / (8 * d * H.EPS):.3g}")
            worst.merge(r)
            above_linear = max(above_linear, g / (8 * d * H.EPS))
    assert worst["eig_res"] <= 0.5 and worst["orth"] <= 0.5, worst
    assert above_linear > 1.0


@pytest.mark.parametrize("kind", ["flat", "geo1e6"])
def test_degraded_restatements_fail(kind):
    d = 25
    pts = EC.cloud(kind, d)
    cov = B.bounding_ellipsoid(pts).cov
    shown = {}
    # an eigen-system computed in float32 and cast up
    lam, vec = np.linalg.eigh(cov.astype(np.float32))
    lam = np.maximum(lam.astype(np.float64), 1e-30)
    r = H.Ratios()
    H.check_eigen(r, cov, vec.astype(np.float64) * np.sqrt(lam), np.sqrt(lam), canonical=False)
    shown["float32 eigen-system"] = max(r["eig_res"], r["orth"])
    # a cyclic Jacobi stopped while off^2 > 1e-20 dia^2
    lam, vec = _jacobi_stopped_early(cov)
    order = np.argsort(lam)
    r = H.Ratios()
    H.check_eigen(r, cov, vec[:, order] * np.sqrt(lam[order]), np.sqrt(lam[order]), canonical=False)
    shown["Jacobi stopped early"] = r["eig_res"]
    # a precision matrix formed in float32
    r = H.Ratios()
    am = np.linalg.inv(cov.astype(np.float32)).astype(np.float64)
    lam = np.linalg.eigvalsh(cov)
    H.check_inverse(r, cov, am, lam[-1] / lam[0])
    shown["float32 inverse"] = r["inv_res"]
    # a one-pass covariance sum x x^T / n - mu mu^T on the live set of width 1e-7
    narrow = EC.cloud(kind + "@1e-7", d)
    n = len(narrow)
    mu = narrow.mean(axis=0)
    one_pass = (narrow.T @ narrow / n - np.outer(mu, mu)) * (n / (n - 1.0))
    b, cov_ld, _ = H.cov_bound(narrow, mu)
    shown["one-pass covariance"] = float(np.max(np.abs(H.ld(one_pass) - cov_ld).astype(np.float64) / b))
    # ... which the two-pass form of the oracle passes
    two_pass = np.cov(narrow, rowvar=False)
    assert float(np.max(np.abs(H.ld(two_pass) - cov_ld).astype(np.float64) / b)) <= 1.0
    print(f"ell_hp DEGRADED {kind}: " + "  ".join(f"{k}: {v:.3g}" for k, v in shown.items()))
    for name, ratio in shown.items():
        assert ratio > 1.0, f"{name} on {kind} passes its bound (error / bound = {ratio:.3g})"


def test_bounds_are_tighter_than_the_hand_set_tolerances(fix):
    """Flat, kappa = 1e3 and kappa = 1e6 families: every derived bound against what tests/test_gpu_rebuild.py and
    tests/test_gpu_small_kernels.py apply to the same quantity -- 1e-9 relative (plus 1e-9 max|cov|) on cov, 1e-10
    max|cov| on axes @ axes.T, 1e-9 relative on axlens, 1e-8 max|am| on am.

    Two of them carry kappa eps by nature and no normwise-stable solver (LAPACK included) does better: the relative
    error of the SMALLEST axis length, spectrum_bound / (2 lam_min), and the precision matrix, inverse_bound ||am||.
    They are below the old figures for flat and kappa = 1e3 at every D, and for kappa = 1e6 up to the D printed
    below; beyond it they are held against kappa-free forms of the same tolerances (1e-9 lam_max, 1e-8 kappa-scaled)
    -- the old suite never applied its figures to a matrix of that condition at all."""
    worst = {}
    beyond = []
    for key, kind, d, n in EC.cloud_cases():
        if kind not in EC.TIGHT_FAMILIES:
            continue
        pts = EC.cloud(kind, d, n)
        o = _oracle_out(pts)
        b, cov_ld, rho = H.cov_bound(pts, o["ctr"])
        cov = cov_ld.astype(np.float64)
        t_cov = float(np.max((b + rho * np.abs(cov)) / (1e-9 * (np.abs(cov) + np.abs(cov).max()))))
        t_res = H.eig_residual_bound(o["cov"]) / (1e-10 * np.abs(o["cov"]).max())
        lam = np.sort(o["axlens"]**2)
        kappa = lam[-1] / lam[0]
        t_axl = H.spectrum_bound(o["cov"]) / (2 * lam[0]) / 1e-9
        t_am = H.inverse_bound(d, kappa) * np.linalg.norm(o["am"], 2) / (1e-8 * np.abs(o["am"]).max())
        for name, t in (("cov", t_cov), ("axes@axes.T", t_res)):
            worst[name] = max(worst.get(name, 0.0), t)
            assert t < 1.0, (key, name, t)
        for name, t in (("axlens", t_axl), ("am", t_am)):
            if kind == "geo1e6" and t >= 1.0:
                beyond.append((d, name, t))
                # kappa-free forms: the absolute error of any eigenvalue against 1e-9 lam_max, the residual AM C - I
                # against 1e-8
                assert H.spectrum_bound(o["cov"]) < 1e-9 * lam[-1] and H.inverse_bound(d, kappa) < 1e-6, (key, name)
                continue
            worst[name + "/" + kind] = max(worst.get(name + "/" + kind, 0.0), t)
            assert t < 1.0, (key, name, t)
    print("ell_hp TIGHTNESS derived bound / hand-set tolerance, worst: "
          + "  ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    print("ell_hp TIGHTNESS kappa = 1e6 cases whose kappa eps terms exceed the old figures (D, quantity, ratio): "
          + ", ".join(f"({d}, {nm}, {t:.2g})"
                      for d, nm, t in sorted({(d, nm): (d, nm, t) for d, nm, t in beyond}.values())))


def test_decision_margins(fix):
    """No case sits where an fp64 evaluator could decide differently from the reference: the distance of
    lam_min / lam_max from 1e-12, over every trial of the loop, exceeds the uncertainty the bounds give that ratio;
    kappa within 10^+-0.5 of 1e12 is not used; every eigenvalue a ln V bound divides by is determined.  The cap on
    cases left out is zero: the device test runs them all."""
    checked = 0
    for key, kind, d, n in _all_clouds():
        rec = H.fixture_case(fix, key)
        pts = EC.cloud(kind, d, n)
        b, cov_ld, rho = H.cov_bound(pts, H.cov_of_points_ld(pts)[0].astype(np.float64))
        top = float(np.linalg.eigvalsh(cov_ld.astype(np.float64))[-1])
        unc = H.decision_uncertainty(d, H.fro(cov_ld) / top, H.fro(b) / top)
        m = rec["margins"]
        assert m[H.MARGIN_R] > unc, (key, m[H.MARGIN_R], unc)
        assert math.isnan(m[H.MARGIN_LOGK]) or abs(m[H.MARGIN_LOGK]) > 0.5, key
        lam = H.lam_ld(rec).astype(np.float64)
        mult = float(rec["fmax"]) / H.LIM
        assert H.spectrum_bound(cov_ld.astype(np.float64) * mult, mult * H.fro(b)) < 0.25 * lam[0], key
        checked += 1
    for d in EC.MAT_DIMS:
        for key, kind in EC.matrix_cases(d):
            rec = H.fixture_case(fix, key)
            a = EC.matrix(kind, d)
            top = float(np.abs(np.linalg.eigvalsh(a)).max())
            rel = H.fro(a) / top if top > 0 else math.sqrt(d)
            unc = H.decision_uncertainty(d, rel) + 4 * (int(rec["trials"]) + 1) * H.EPS * (rel + math.sqrt(d))
            m = rec["margins"]
            assert m[H.MARGIN_R] > unc, (key, m[H.MARGIN_R], unc)
            assert math.isnan(m[H.MARGIN_LOGK]) or abs(m[H.MARGIN_LOGK]) > 0.5, key
            checked += 1
    assert checked == len(H.all_case_keys())
    print(f"ell_hp MARGINS: {checked} decision cases, none left out")


def test_cases_reach_the_routes_they_are_meant_for(fix):
    """tr(cov) tr(cov^-1) on either side of 1e7, the leading pairs as close as their names say, the floored and the
    blended matrices floored and blended."""
    for key, kind, d, n in EC.cloud_cases():
        rec = H.fixture_case(fix, key)
        m = rec["margins"]
        if kind == "trlo":
            assert 1e6 < m[H.MARGIN_TRTR] < 1e7, (key, m)
        if kind == "trhi":
            assert 1e7 < m[H.MARGIN_TRTR] < 1e8, (key, m)
        if kind in EC.GAPS:
            want = float(kind[3:])
            assert want / 3 < m[H.MARGIN_GAP] < want * 3, (key, m)
        if kind == "iso":
            assert m[H.MARGIN_LOGK] < -11.9 and (d == 1 or m[H.MARGIN_GAP] < 1e-13), (key, m)
        assert bool(rec["good"]) == (kind not in ("geo1e13", "rank3")), key
        assert ("cov_out" in rec) == (kind in ("geo1e13", "rank3")), key
    for d in EC.MAT_DIMS:
        for key, kind in EC.matrix_cases(d):
            rec = H.fixture_case(fix, key)
            if kind == "neg":  # a positive top over a negative eigenvalue: floored in the first trial
                assert not rec["good"] and int(rec["trials"]) == 1 and "cov_out" in rec, (key, int(rec["trials"]))
            if kind == "negdef":  # blended until the top eigenvalue is positive, then floored (or accepted)
                assert not rec["good"] and 50 < int(rec["trials"]) < 99, (key, int(rec["trials"]))
            if kind == "zero":
                assert int(rec["trials"]) == 1 and np.all(rec["ab"] == [0, 0, 1e-10, 0]) or \
                    (int(rec["trials"]) == 1 and abs(rec["ab"][2] - 1e-10) < 1e-25), key
            if kind == "geo1e13":
                assert "cov_out" in rec and int(rec["trials"]) == 1, key
            if EC.is_positive_kind(kind):
                assert rec["good"], key


@pytest.mark.parametrize("d", H.CONTAINS_DIMS)
def test_membership_reference_puts_every_point_on_its_side(d):
    c = H.contains_case(d)
    x, q, b = c["x"], c["q"], c["bound"]
    assert x.min() > 0 and x.max() < 1
    k = len(x)
    own = np.repeat([0, 1], k // 2)
    dist = (q - 1).astype(np.float64)
    # decidable for BOTH ellipsoids: nothing within its own bound of a boundary
    assert np.all(np.abs(dist) > b)
    mine, bm = dist[np.arange(k), own], b[np.arange(k), own]
    assert np.all(np.sign(mine) == np.sign(c["target"] - 1))
    near = np.abs(c["target"] - 1) < 1e-7
    assert near.sum() == k // 2
    # "4 bounds" as near as the fp64 grid allows: never below 2, and some as near as 8 for either ellipsoid
    assert np.all(np.abs(mine[near]) >= 2 * bm[near])
    for a in (0, 1):
        assert np.min(np.abs(mine[near & (own == a)]) / bm[near & (own == a)]) <= 8
    far = ~near
    np.testing.assert_allclose(np.abs(mine[far]), 1e-6, rtol=1e-3)
    print(f"ell_hp CONTAINS D={d}: |q - 1| / bound of the near points: min {np.min(np.abs(mine[near]) / bm[near]):.2f} "
          f"median {np.median(np.abs(mine[near]) / bm[near]):.2f} max {np.max(np.abs(mine[near]) / bm[near]):.1f}")
