"""tests/scale_hp_ref.py and tests/scale_cases.py without a device: the reference against mpmath, the fixture, the share
of decided cases, the float64 oracles inside every bound, and NumPy evaluations with one defect each outside one.
tests/test_gpu_scale_hp.py holds scale_logvol_kernel to the same checks."""
import mpmath as mp
import numpy as np
import pytest

import scale_cases as C
import scale_hp_ref as H
from oracle import bounding_ref as B

SMALL = [(f, d) for f, d in C.CASES if d <= 25]


def np_scale(cov, am, axes, axlens, logvol, target, defect=None):
    """The formulas of scale_hp_ref's docstring in float64 NumPy, on the stored axes; `defect` plants one fault."""
    D = len(axlens)
    exp = (lambda v: np.exp(np.asarray(v, dtype=np.float32)).astype(np.float64)) if defect == "exp32" else np.exp
    logf = target - logvol
    cap = np.log(np.sqrt(D)) if defect == "cap" else np.log(np.sqrt(D) / 2)
    lax = np.log(axlens)
    if lax.max() < cap - logf / D:
        f = np.float64(exp(logf / D))
        return dict(cov=cov * f**2, am=am * (1 / f if defect == "am_f" else 1 / f**2), axes=axes * f, axlens=axlens * f,
                    logvol=target)
    delta = np.zeros(D)
    left, nleft = logf, D
    for k in (np.argsort(lax) if defect == "smallest_first" else np.argsort(lax)[::-1]):
        dk = min(cap - lax[k], left / (D if defect == "left_D" else nleft))
        delta[k] = dk if defect == "no_max" else max(dk, 0.0)
        left -= delta[k]
        nleft -= 1
    fax = exp(delta)
    v = axes / axlens
    l1 = axlens**2 * fax**2
    return dict(cov=(v * (axlens**2 if defect == "cov_l" else l1)) @ v.T, am=(v / l1) @ v.T,
                axes=axes if defect == "axes" else axes * fax, axlens=axlens * fax, logvol=target)


DEFECTS = ("cap", "left_D", "no_max", "smallest_first", "am_f", "axes", "exp32", "cov_l")


def run(c, fn):
    m = len(c["targets"])
    with np.errstate(all="ignore"):  # (a planted defect may overflow)
        outs = [fn(c["covs"][e].copy(), c["ams"][e].copy(), c["axess"][e].copy(), c["axlenss"][e].copy(),
                   float(c["logvols"][e]), float(c["targets"][e])) for e in range(m)]
    return {n: [o[n] for o in outs] for n in H.FIELDS}


def test_log_exp_allowance_is_calibrated():
    """The ulp granted per log / exp holds for a float64 evaluator that is not the device's."""
    for name, ulps in H.calibrate().items():
        print(f"[scale_hp] numpy {name}: {ulps:.3f} ulp against long double")
        assert ulps <= 1.0, name


@pytest.mark.parametrize("family,d", [(f, d) for f, d in C.CASES if d <= 5])
def test_reference_against_mpmath(family, d):
    """Round trips at 50 digits: ln fax = delta, the deltas spend logf exactly unless every axis is capped, no axis
    grows past the cap, and cov' / am' / axes' of the long-double part equal the same sums in mpmath to its own bound."""
    c = C.case(family, d)
    with mp.workdps(H.DPS):
        cap = mp.log(mp.sqrt(d) / 2)
        for e, (val, bnd, sc) in enumerate(c["ref"]):
            own = H.own(sc)
            delta = [mp.mpf(h) + mp.mpf(l) for h, l in own["delta"].T]
            fax = [mp.mpf(h) + mp.mpf(l) for h, l in own["fax"].T]
            a = [mp.mpf(float(v)) for v in c["axlenss"][e]]
            logf = mp.mpf(float(c["targets"][e])) - mp.mpf(float(c["logvols"][e]))
            for k in range(d):
                assert abs(mp.log(fax[k]) - delta[k]) < mp.mpf(10) ** -30
                if delta[k] > 0:
                    assert mp.log(a[k]) + delta[k] <= cap + mp.mpf(10) ** -30
                elif not sc["iso"]:
                    assert delta[k] == 0
            capped = [abs(mp.log(a[k]) + delta[k] - cap) < mp.mpf(10) ** -30 or mp.log(a[k]) > cap for k in range(d)]
            if sc["iso"] or (logf > 0 and not all(capped)):
                assert abs(sum(delta) - logf) < mp.mpf(10) ** -28 * max(1, abs(logf)), (c["name"], c["labels"][e])
            else:  # every axis at the cap, or a shrinking target on the greedy branch: nothing (more) to spend
                assert 0 <= sum(delta) <= max(logf, 0)
            X = [[mp.mpf(float(v)) for v in row] for row in c["axess"][e]]
            for i in range(d):
                for j in range(d):
                    if sc["iso"]:
                        want_c = mp.mpf(float(c["covs"][e][i, j])) * fax[0] ** 2
                        want_a = mp.mpf(float(c["ams"][e][i, j])) / fax[0] ** 2
                        s_c, s_a = abs(want_c), abs(want_a)
                    else:
                        want_c = sum(X[i][k] * X[j][k] * fax[k] ** 2 for k in range(d))
                        want_a = sum(X[i][k] * X[j][k] / (a[k] ** 4 * fax[k] ** 2) for k in range(d))
                        s_c = sum(abs(X[i][k] * X[j][k]) * fax[k] ** 2 for k in range(d))
                        s_a = sum(abs(X[i][k] * X[j][k]) / (a[k] ** 4 * fax[k] ** 2) for k in range(d))
                    for name, want, s in (("cov", want_c, s_c), ("am", want_a, s_a)):
                        got = mp.mpf(float(val[name][i, j])) + mp.mpf(float(val[name][i, j] - H.LD(float(val[name][i, j]))))
                        assert abs(got - want) <= (d + 8) * H.U_LD * s, (c["name"], c["labels"][e], name, i, j)
                    got = mp.mpf(float(val["axes"][i, j])) + mp.mpf(float(val["axes"][i, j] - H.LD(float(val["axes"][i, j]))))
                    assert abs(got - X[i][j] * fax[j]) <= 3 * H.U_LD * abs(got)
            assert val["logvol"] == c["targets"][e] and bnd["logvol"] == 0.0


def test_fixture_pins_the_reference():
    """tests/golden/scale_hp.npz: the per-axis delta (two doubles), the verdicts and the targets of every case."""
    g = np.load(C.GOLDEN)
    now = C.golden_arrays()
    assert list(g["names"]) == list(now["names"])
    for key in ("offsets", "iso", "decided", "targets", "delta_hi", "delta_lo"):
        assert np.array_equal(g[key], now[key]), key
    assert np.allclose(g["margin_over_bound"], now["margin_over_bound"], rtol=1e-6, atol=0)


def test_every_case_is_decided_with_margin():
    """Every ellipsoid but the +-1/8 pair of each `edge` case is decided by the reference, on the intended side; the
    edge cases sit where their labels say."""
    total = decided = 0
    for f, d in C.CASES:
        c = C.case(f, d)
        for e, (_, _, sc) in enumerate(c["ref"]):
            total += 1
            decided += sc["decided"]
            assert sc["decided"] != C.must_be_undecided(c, e), (c["name"], c["labels"][e], sc["margin"], sc["dec_bound"])
            if f == "edge":
                k = float(c["labels"][e][2:])
                assert abs(sc["margin"] / sc["dec_bound"] - k) < 0.01 * abs(k), (c["name"], k, sc["margin"] / sc["dec_bound"])
                assert sc["iso"] == (k > 0)
            lax = np.sort(sc["lax"])
            gaps = np.diff(lax)
            assert np.all((gaps == 0) | (gaps > 1e-9)), (c["name"], c["labels"][e])
    n_edge = sum(1 for f, d in C.CASES if f == "edge")
    print(f"[scale_hp] decided {decided} of {total} ellipsoids; undecided on purpose {2 * n_edge}")
    assert total - decided == 2 * n_edge and decided / total > 0.93
    branches = [sc["iso"] for f, d in C.CASES for _, _, sc in C.case(f, d)["ref"]]
    assert 0.3 < np.mean(branches) < 0.7  # both branches are exercised about equally


@pytest.mark.parametrize("family", C.FAMILIES)
def test_numpy_restatement_inside_every_bound(family):
    worst = dict.fromkeys(H.FIELDS, 0.0)
    for f, d in C.CASES:
        if f != family:
            continue
        c = C.case(f, d)
        w = C.check(c, run(c, np_scale), "numpy")
        for n in H.FIELDS:
            worst[n] = max(worst[n], w[n])
            assert w[n] <= 1.0, (c["name"], n, w[n])
    print(f"scale_hp WORST numpy {family}: " + "  ".join(f"{n} {worst[n]:.3g}" for n in H.FIELDS))


@pytest.mark.parametrize("name", C.CLOUDS)
def test_golden_clouds_inside_every_bound(name):
    """The inputs of test_gpu_small_kernels' anisotropic cases at the derived bounds (NumPy on the stored axes)."""
    c = C.cloud_case(name)
    assert c["ref"][0][2]["decided"] and not c["ref"][0][2]["iso"]
    w = C.check(c, run(c, np_scale), "numpy")
    assert max(w.values()) <= 1.0, (name, w)


def test_flat10_loose_tolerance_is_the_inputs_conditioning():
    """flat10 is rank-3 data in 10-D: seven eigenvalues of 1.1e-13 sit 1e-11 below the largest, so the rounding of the
    stored cov itself (2^-53 of its largest element) moves them by parts in 1e6.  The function evaluated on a 50-digit
    eigen-system of the stored cov therefore differs from the function on the stored axes in am' by parts in 1e6 of
    the largest element -- the 1e-5 / 1e-3 of test_gpu_small_kernels.py cover an evaluator that decomposes cov afresh
    -- while cov' agrees to rounding, and the derived bound on the stored axes is seven orders tighter."""
    c = C.cloud_case("flat10")
    cov, am, axl = c["covs"][0], c["ams"][0], c["axlenss"][0]
    val, bnd, _ = c["ref"][0]
    D = len(axl)
    with mp.workdps(H.DPS):
        E, Q = mp.eigsy(mp.matrix(cov.tolist()))
        lam = np.array([float(E[i]) for i in range(D)])
        Xe = np.array([[float(Q[i, j] * mp.sqrt(E[j])) for j in range(D)] for i in range(D)])
        ae = np.array([float(mp.sqrt(E[j])) for j in range(D)])
    v2, _, sc2 = H.reference(cov, am, Xe, ae, c["logvols"][0], c["targets"][0])
    assert not sc2["iso"] and sc2["decided"]
    big = {n: float(np.abs(val[n]).max()) for n in ("cov", "am")}
    diff = {n: float(np.abs(v2[n] - val[n]).max()) / big[n] for n in ("cov", "am")}
    room = {n: float(bnd[n].max()) / big[n] for n in ("cov", "am")}
    dlam = float(np.max(np.abs(np.sort(axl**2) - lam) / lam))
    print(f"[scale_hp] flat10: eigenvalues of the stored cov against axlens^2 {dlam:.3g}; 50-digit eigen-system against "
          f"stored axes, of the largest element: cov' {diff['cov']:.3g}  am' {diff['am']:.3g}; derived bound on the stored "
          f"axes: cov' {room['cov']:.3g}  am' {room['am']:.3g}")
    assert diff["cov"] < 1e-13 and 1e-7 < diff["am"] < 1e-3 and 1e-7 < dlam < 1e-4
    assert room["cov"] < 1e-13 and room["am"] < 1e-11


def oracle_scale(cov, am, axes, axlens, logvol, target):
    """oracle.bounding_ref.scale_ell_to_logvol.  It pairs eigh's ascending eigenvalues with axlens by index, so it is
    handed the columns in ascending order and its outputs are put back."""
    D = len(axlens)
    p = np.argsort(axlens, kind="stable")
    ell = B.Ell(np.zeros(D), cov, am, np.ascontiguousarray(axes[:, p]), axlens[p].copy(), logvol)
    B.scale_ell_to_logvol(ell, target)
    inv = np.argsort(p)
    return dict(cov=ell.cov, am=ell.am, axes=ell.axes[:, inv], axlens=ell.axlens[inv], logvol=ell.logvol)


@pytest.mark.parametrize("family", C.FAMILIES)
def test_oracle_inside_every_bound(family):
    """axlens', axes' and logvol' are the same function in the oracle on both branches and are held to the reference's
    bounds everywhere, cov' and am' on the isotropic branch.  On the greedy branch the oracle takes a fresh eigh(cov),
    another function of the input, and its cov' and am' are held, in the Frobenius norm, to
    scale_hp_ref.fresh_eigh_bounds, which adds the conditioning of that decomposition: every decided greedy case that
    is posed for such an evaluator.  The ones that are not (the perturbation of the stored cov reaches an eigenvalue
    gap between axes with different factors) all have an axis ratio of 1e6."""
    worst = dict.fromkeys(H.FIELDS, 0.0)
    fresh = dict.fromkeys(("cov", "am"), 0.0)
    n_greedy = n_posed = 0
    for f, d in C.CASES:
        if f != family or d > 128:  # (at 512 the reference exists on 48 rows only)
            continue
        c = C.case(f, d)
        out = run(c, oracle_scale)
        for e, (val, bnd, sc) in enumerate(c["ref"]):
            r = H.ratios({n: out[n][e] for n in H.FIELDS}, val, bnd, c["rows"])
            elementwise = sc["iso"] and sc["decided"]
            for n in H.FIELDS:
                if n in fresh and not elementwise:
                    continue
                worst[n] = max(worst[n], r[n])
                assert r[n] <= 1.0, (c["name"], c["labels"][e], n, r[n])
            if sc["iso"] or not sc["decided"]:
                continue
            n_greedy += 1
            own = H.own(sc)
            posed, b_cov, b_am = H.fresh_eigh_bounds(c["covs"][e], c["axess"][e], c["axlenss"][e], H.join(*own["fax"]), own["r"])
            if not posed:
                assert f == "kappa" and c["labels"][e].startswith("1e+06"), (c["name"], c["labels"][e])
                continue
            n_posed += 1
            for n, b in (("cov", b_cov), ("am", b_am)):
                err = float(np.sqrt(np.sum((np.asarray(out[n][e]).astype(H.LD) - val[n]) ** 2)))
                fresh[n] = max(fresh[n], err / b)
                assert err <= b, (c["name"], c["labels"][e], n, err / b)
    print(f"scale_hp WORST oracle {family}: " + "  ".join(f"{n} {worst[n]:.3g}" for n in H.FIELDS) +
          f"   greedy branch, fresh eigh(cov), Frobenius error / bound: cov {fresh['cov']:.3g}  am {fresh['am']:.3g}"
          f"  ({n_posed} of {n_greedy} decided greedy cases posed)")


@pytest.mark.parametrize("defect", DEFECTS)
def test_one_defect_fails(defect):
    """Each NumPy evaluation with one planted fault leaves a bound on at least one case."""
    failed = []
    for f, d in SMALL:
        c = C.case(f, d)
        out = run(c, lambda *a: np_scale(*a, defect=defect))
        for e, (val, bnd, sc) in enumerate(c["ref"]):
            r = H.ratios({n: out[n][e] for n in H.FIELDS}, val, bnd, c["rows"])
            if max(r.values()) > 1.0:
                failed.append((c["name"], c["labels"][e], max(r, key=r.get), max(r.values())))
    print(f"[scale_hp] defect {defect}: fails {len(failed)} ellipsoids, first {failed[:1]}")
    assert failed, defect
