"""The bounding-ellipsoid linear algebra of the device (covariance, eigen-system, precision matrix, log-volume, the
1 - 1e-3 rescaling, improve_covar_mat, the quadratic forms of dh_contains) held to the high-precision reference of
tests/ell_hp_ref.py at its derived bounds, on the cases of tests/ell_cases.py: spectra that walk the condition number
through kFastCond, kFastSquarings, kMaxCond and the identity blend; every dimension at which jacobi_block, spd_fast,
the MFMA forms, jacobi_wave and the wide path change route; live sets of width 1e-7.

No mpmath runs here: the reference's side is tests/golden/ell_hp.npz (tools/make_golden.py ell_hp) and long-double
residuals taken against the device's own returned covariance.  Every case prints error / bound for every bound; a
test fails if any ratio is above 1.  tests/test_ell_hp_cpu.py shows, without a device, that the float64 oracle passes
the same checks and that degraded restatements do not.
"""
import numpy as np
import pytest

import ell_cases as EC
import ell_hp_ref as H

pytestmark = pytest.mark.gpu

ALL_D = sorted(set(EC.DIMS) | {25})


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def fix():
    return H.load_fixture()


def _out(got, i=0):
    return dict(ctr=got["ctrs"][i], cov=got["covs"][i], am=got["ams"][i], axes=got["axes"][i],
                axlens=got["axlens"][i], logvol=got["logvol_ells"][i])


def _clouds_of(d):
    return [c for c in EC.cloud_cases() if c[2] == d]


def _report(failures, worst, key, r):
    print(f"ell_hp {key}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
    worst.merge(r)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    if bad:
        failures.append((key, bad))


def _finish(failures, worst, what):
    print(f"ell_hp WORST {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not failures, f"{what}: error / bound above 1 in {len(failures)} case(s): {failures[:6]}"


@pytest.mark.parametrize("d", ALL_D)
def test_rebuild_single(ctx, fix, d):
    """Ellipsoid.update (mode 1): the reference's route -- Jacobi eigh inside improve_covar_mat's loop."""
    failures, worst = [], H.Ratios()
    for key, kind, _, n in _clouds_of(d):
        pts = EC.cloud(kind, d, n)
        got = ctx.rebuild(pts, multi=False)
        assert got["nells"] == 1
        _report(failures, worst, key, H.check_bounding(pts, _out(got), H.fixture_case(fix, key), key))
    _finish(failures, worst, f"rebuild single D={d}")


@pytest.mark.parametrize("d", ALL_D)
def test_rebuild_multi_root_kept(ctx, fix, d):
    """MultiEllipsoid.update (mode 0) on the unimodal clouds whose root the oracle keeps: the eigen-free root (LDL^T,
    explicit inverse, ln V from the pivots) where its certificate holds, and the eigen-system of the output from
    k_out_eig / k_root_eig."""
    failures, worst = [], H.Ratios()
    used = 0
    for key, kind, _, n in _clouds_of(d):
        rec = H.fixture_case(fix, key)
        if not rec["multi_ok"]:
            continue
        used += 1
        pts = EC.cloud(kind, d, n)
        got = ctx.rebuild(pts, multi=True)
        assert got["nells"] == 1, f"{key}: the oracle keeps the root, the device returned {got['nells']} ellipsoids"
        _report(failures, worst, key, H.check_bounding(pts, _out(got), rec, key, logvol_from_spectrum=False))
    assert used > 0
    _finish(failures, worst, f"rebuild multi D={d}")


def test_rebuild_many_mixed_batch_d25(ctx, fix):
    """One ragged batch of every D = 25 cloud (mixed spectra, sizes 130 to 513): bit for bit the single calls, in both
    modes, and inside the bounds."""
    cases = _clouds_of(25)
    sets = [EC.cloud(kind, 25, n) for _, kind, _, n in cases]
    failures, worst = [], H.Ratios()
    for multi in (False, True):
        keep = [i for i, c in enumerate(cases) if not multi or H.fixture_case(fix, c[0])["multi_ok"]]
        res = ctx.rebuild_many([sets[i] for i in keep], multi=multi)
        for i, r in zip(keep, res):
            one = ctx.rebuild(sets[i], multi=multi)
            assert r["nells"] == one["nells"] == 1
            for k in ("ctrs", "covs", "ams", "axes", "axlens", "logvol_ells"):
                np.testing.assert_array_equal(r[k], one[k], err_msg=f"{cases[i][0]} {k} multi={multi}")
            _report(failures, worst, f"{cases[i][0]} multi={multi}",
                    H.check_bounding(sets[i], _out(r), H.fixture_case(fix, cases[i][0]), cases[i][0],
                                     logvol_from_spectrum=not multi))
    _finish(failures, worst, "rebuild_many D=25")


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("d", EC.WIDE_DIMS)
def test_rebuild_wide(ctx, fix, d, split, monkeypatch):
    """The wide path (wide.hip) in single mode through both of its eigensolver forms: the multi-workgroup one-sided
    block Jacobi and the single-launch two-sided solver (DH_WIDE_EIG=0)."""
    if not split:
        monkeypatch.setenv("DH_WIDE_EIG", "0")
    failures, worst = [], H.Ratios()
    for key, kind, _, n in [c for c in EC.wide_cases() if c[2] == d]:
        pts = EC.cloud(kind, d, n)
        got = ctx.rebuild(pts, multi=False)
        assert got["nells"] == 1
        _report(failures, worst, key, H.check_bounding(pts, _out(got), H.fixture_case(fix, key), key))
    _finish(failures, worst, f"rebuild wide D={d} split={split}")


@pytest.mark.parametrize("d", EC.MAT_DIMS)
def test_ell_from_cov(ctx, fix, d):
    cases = [(k, kind) for k, kind in EC.matrix_cases(d) if EC.is_positive_kind(kind)]
    stack = np.array([EC.matrix(kind, d) for _, kind in cases])
    axes, axlens, ams, lvs = ctx.ell_from_cov(stack)
    failures, worst = [], H.Ratios()
    for i, (key, _) in enumerate(cases):
        _report(failures, worst, key, H.check_ell_from_cov(stack[i], axes[i], axlens[i], ams[i], lvs[i],
                                                           H.fixture_case(fix, key)))
    _finish(failures, worst, f"ell_from_cov D={d}")


@pytest.mark.parametrize("d", EC.MAT_DIMS)
def test_improve_covar_mat(ctx, fix, d):
    cases = EC.matrix_cases(d)
    stack = np.array([EC.matrix(kind, d) for _, kind in cases])
    good, cov, am, axes = ctx.improve_covar_mat(stack)
    failures, worst = [], H.Ratios()
    for i, (key, _) in enumerate(cases):
        _report(failures, worst, key, H.check_improve_covar_mat(stack[i], good[i], cov[i], am[i], axes[i],
                                                                H.fixture_case(fix, key)))
    _finish(failures, worst, f"improve_covar_mat D={d}")


def test_hip_ellipsoid_update(ctx, fix):
    """The class path: HipEllipsoid.update on one cloud (kappa = 1e6 in 13-D)."""
    from dynesty_amd import backend
    from dynesty_amd.bounding import HipEllipsoid
    key, kind, d, n = "cl/13/geo1e6", "geo1e6", 13, EC.cloud_size("geo1e6", 13)
    pts = EC.cloud(kind, d, n)
    backend.set_backend(ctx)
    try:
        e = HipEllipsoid(d)
        e.update(pts)
    finally:
        backend.set_backend(None)
    out = dict(ctr=e.ctr, cov=e.cov, am=e.am, axes=e.axes, axlens=e.axlens, logvol=e.logvol)
    H.check_bounding(pts, out, H.fixture_case(fix, key), key).assert_ok("HipEllipsoid.update " + key)


@pytest.mark.parametrize("d", H.CONTAINS_DIMS)
def test_contains_next_to_the_boundary(ctx, d):
    """dh_contains' quadratic forms against the long-double ones at (D^2 + 4) eps sum |d_i| |A_ij| |d_j|, and
    membership held exactly, in both modes (q < 1 strict; sqrt(q) <= 1), for points 4 bounds and 1e-6 either side of
    the boundary of a kappa = 1e3 and a kappa = 1e9 ellipsoid."""
    c = H.contains_case(d)
    inside = (c["q"] < 1).sum(axis=1)
    r = H.Ratios()
    for mode in (0, 1):
        count, _, quad = ctx.contains(c["x"], c["ctrs"], c["ams"], mode=mode, want_quad=True)
        err = np.abs(H.ld(quad) - c["q"]).astype(np.float64)
        r.add(f"quad_mode{mode}", np.max(err / c["bound"]), 1.0)
        np.testing.assert_array_equal(count, inside, err_msg=f"membership, mode {mode}")
    r.assert_ok(f"contains D={d}")
