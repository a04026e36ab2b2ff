"""Run-level analysis of a merged run on the host (dynesty_amd/errors.py on ensemble.MergedRun):
the divergence from the run to its realizations and bootstraps (utils.kld_error), the weight function and the stopping
function (dynamicsampler.py) against the reference's records (tests/golden/merge_dynamic.npz) and the long-double
restatement with its derived bounds (tests/merge_dynamic_ref.py).  tests/test_gpu_merge_dynamic.py holds the device to
the same."""
import os
import warnings

import numpy as np
import pytest

import bootstrap_cases as bc
import merge_cases
import merge_dynamic_ref as dr
from merge_hp_ref import U
from test_merge_errors_cpu import reference_gates

SEED, NDIST = 1234, 2000  # the distribution gates' seed and size
MODES = ("jitter", "resample", "simulate")
STOP_ARGS = ({}, dict(pfrac=0.5, evid_thresh=0.05, target_n_effective=2000), dict(pfrac=0.0, evid_thresh=0.2))


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(bc.GOLD, "merge_dynamic.npz")), np.load(os.path.join(bc.GOLD, "merge_bootstrap.npz"))


_RUNS = {}


def run_of(name):
    if name not in _RUNS:
        _RUNS[name] = bc.host_run(name)
    return _RUNS[name]


def check_weight_grid(run, m, fix, name, chain, label):
    """Bounds and indices of `run` equal to the reference's on the whole grid; every index decided by the restatement."""
    g = fix[0]
    worst = np.inf
    for i, pf in enumerate(g["pfrac"]):
        h = dr.weights_hp(m, pf)
        b = dr.weight_bounds(h, float(pf), chain)
        for j, mf in enumerate(g["maxfrac"]):
            want, margin = dr.decide(h, b["w"], float(mf))
            worst = min(worst, margin)
            assert margin > 1, (name, pf, mf, margin)
            assert want == tuple(g[f"{name}/idx"][i, j])
            for k, pad in enumerate(g[f"{name}/pad"]):
                bounds, idx = run._err_weight_function(float(pf), float(mf), int(pad))
                assert idx == want, (name, pf, mf, pad, idx, want)
                assert bounds == tuple(g[f"{name}/bounds"][i, j, k]), (name, pf, mf, pad)
                assert run.weight_function(float(pf), float(mf), int(pad)) == bounds
    print(f"[merge dynamic {label}] smallest margin / allowance of an index = {worst:.3g}")


def check_weights(got, m, fix, name, chain, label):
    """(pweight, zweight, weight) at pfrac 0.8 within bound of the restatement and of the reference's arrays.  The
    reference's arrays are functions of the HOST's merged run (the Results tools/make_golden.py built), `got` of the run
    `m`; where that is the device's, whose logwt, logz and logvol differ from the host's by their own rounding, the
    exact values of the two differ, and by how much is the restatement's own difference between the two inputs."""
    h = dr.weights_hp(m, 0.8)
    mr = run_of(name)
    hr = h if m is mr else dr.weights_hp(mr, 0.8)
    b, bh = dr.weight_bounds(h, 0.8, chain), dr.weight_bounds(hr, 0.8, mr.niter + 16)
    worst = 0.0
    for arr, k in zip(got, ("pw", "zw", "w")):
        worst = max(worst, dr.check(arr, h[k], b[k], f"{label} {k}"))
        ref = fix[0][f"{name}/" + dict(pw="pweight", zw="zweight", w="weight")[k]]
        dr.check(ref, hr[k], bh[k] + (0 if k == "pw" else bh["ref_zw"]), f"{label} {k}: the reference against the restatement")
        shift = np.abs(np.asarray(h[k] - hr[k], dtype=np.float64)) * (1 + 2 * U) + 1e-320
        dr.check(arr, ref, b[k] + bh[k] + (0 if k == "pw" else bh["ref_zw"]) + shift, f"{label} {k} vs reference")
    return worst


@pytest.mark.parametrize("name", bc.NAMES)
def test_weight_function_against_reference(fix, name):
    m = run_of(name)
    check_weight_grid(m, m, fix, name, m.niter + 16, f"host {name}")
    (lo, hi), w = m.weight_function(return_weights=True)
    assert (lo, hi) == tuple(fix[0][f"{name}/bounds"][2, 0, 1])
    check_weights(w, m, fix, name, m.niter + 16, f"host {name}")


def reference_allowance(h, b):
    """The reference's own float64 arithmetic: sequential sums (host chains, `b`), its volume steps log(n / (n + 1))
    rounded at full size (u absolute per step: 2 M' u in ln w and in ln Z), and logp1 - logp2 formed from two numbers
    of the size of ln Z each (u of each per term)."""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    p, lw = f(h["p"]), f(h["logwt"])
    with np.errstate(invalid="ignore"):
        d = np.where(p > 0, np.abs(f(h["e"]) - float(h["dz"])), 0.0)
        size = np.where(p > 0, 2 * np.abs(lw - float(h["logz"][-1])) + d, 0.0)
    return b["cum"] + 4 * h["M"] * U * np.cumsum(p * (1 + d)) + 2 * U * np.cumsum(p * size)


def check_resample_against_reference(run, m, fix, name, chains, label):
    """The cumulative divergence with the reference's draws.  Without ties the resampled run is the reference's point
    for point; inside a group of equal ln L the reference's unstable argsort pairs positions with other members of the
    group than the stable order does, so there the reference is held to the restatement under ITS order
    (merge_bootstrap.npz's samp_idx and samples_n) and the run to the restatement under the stable one."""
    key, S = bc.strands(m)
    worst = 0.0
    for i in range(bc.NCALLS):
        mult = bc.multiplicities(fix[0][f"{name}/{i}/draws"], S)
        np.testing.assert_array_equal(fix[0][f"{name}/{i}/draws"], fix[1][f"{name}/{i}/draws"])
        ref = fix[0][f"{name}/{i}/kld"]
        got = run.kld_error(error="resample", mult=mult)
        idx, n = dr.sequence(m, "resample", 0, 0, mult)
        h = dr.kld_hp(m, idx, n, 0, 0, False)
        b, bh = dr.kld_bounds(h, chains(h["M"])), dr.kld_bounds(h, dr.host_chains(h["M"]))
        worst = max(worst, dr.check(got, h["kld_cum"], b["cum"], f"{label} call {i}"))
        hr = dr.kld_hp(m, fix[1][f"{name}/{i}/samp_idx"].astype(np.int64), fix[1][f"{name}/{i}/samples_n"], 0, 0, False)
        allow = reference_allowance(hr, dr.kld_bounds(hr, dr.host_chains(hr["M"])))
        dr.check(ref, hr["kld_cum"], allow, f"{label} call {i}: the reference against the restatement")
        if name in bc.TIE_FREE:
            dr.check(got, ref, b["cum"] + reference_allowance(h, bh), f"{label} call {i} vs reference")
        one = run._err_kld(0, 0, 1, 1, mult)
        assert one[2][0] == len(ref)
        dr.check(one[0][0], h["kld"], b["batch"], f"{label} call {i} batch")
    return worst


@pytest.mark.parametrize("name", bc.NAMES)
def test_resample_divergence_with_the_references_draws(fix, name):
    m = run_of(name)
    check_resample_against_reference(m, m, fix, name, dr.host_chains, f"host {name}")


def test_expected_volumes_have_no_divergence():
    """The realization at the expected volumes is the merged run itself: the divergence is the run's own rounding --
    within bound of the restatement, whose value is within the bound too (|e_p| <= b_wt[p], |dz| <= b_lnZ, both inside
    it) after the merge's volume steps (2 M u)."""
    from dynesty_amd import errors
    for name in ("golden", "g_span", "b_plateau"):
        m = run_of(name)
        kld, lz = errors.kld_host(m.logl, m.samples_n, m.logwt, m.logz[-1], 0, 0, 1, jitter=False)
        h = dr.kld_hp(m, np.arange(m.niter), m.samples_n, 0, 0, False)
        b = dr.kld_bounds(h, dr.host_chains(m.niter))["batch"]
        dr.check(kld[0], h["kld"], b, f"host {name} expected volumes")
        print(f"[merge dynamic host {name}] divergence at the expected volumes {kld[0]:.3g} (bound {2 * b + 4 * m.niter * U:.3g})")
        assert abs(kld[0]) <= 2 * b + 4 * m.niter * U
        assert lz[0] == m.logz_realizations(1, jitter=False)["logz"][0]


def check_modes(run, m, name, chains, indices, label, seed=77):
    """Batch and cumulative divergence of `run` within bound of the restatement; the last cumulative value against the
    batch; logz and npoints those of the existing calls."""
    worst = dict(batch=0.0, cum=0.0)
    for mode in MODES:
        for index in indices:
            idx, n = dr.sequence(m, mode, seed, index)
            h = dr.kld_hp(m, idx, n, seed, index, mode != "resample")
            b = dr.kld_bounds(h, chains(h["M"]))
            one = run.kld_realizations(1, seed, index, mode)
            cum = run.kld_error(seed, index, mode)
            lab = f"{label} {mode} {index}"
            assert len(cum) == len(idx) and np.isfinite(one["kld"]).all()
            worst["batch"] = max(worst["batch"], dr.check(one["kld"][0], h["kld"], b["batch"], lab + " batch"))
            worst["cum"] = max(worst["cum"], dr.check(cum, h["kld_cum"], b["cum"], lab + " cumulative"))
            dr.check(cum[-1], one["kld"][0], b["cum"][-1] + b["batch"], lab + " cumulative against batch")
            if mode == "jitter":
                assert "npoints" not in one
                assert one["logz"][0] == run.logz_realizations(1, seed, index)["logz"][0]
            else:
                old = run.bootstrap_realizations(1, seed, index, jitter=mode == "simulate")
                assert one["npoints"][0] == old["npoints"][0] == len(idx) and one["logz"][0] == old["logz"][0]
            part = run.kld_error(seed, index, mode, first=3, count=5)
            np.testing.assert_array_equal(part, cum[3:8])
    return worst


@pytest.mark.parametrize("name", ["golden", "b_plateau", "g_span", "i_endties"])
def test_batch_and_cumulative_against_restatement(name):
    m = run_of(name)
    check_modes(m, m, name, dr.host_chains, (0, 2 ** 32 + 5), f"host {name}")


def test_batch_is_a_function_of_seed_and_index():
    m = run_of("c_ragged")
    for mode in MODES:
        single = [m.kld_realizations(1, 9, 7 + i, mode) for i in range(5)]
        a = m.kld_realizations(5, 9, 7, mode)
        for k in a:
            np.testing.assert_array_equal(a[k], np.concatenate([s[k] for s in single]))


def distribution_gates(run, fix, label):
    g = fix[0]
    jit = run.kld_realizations(NDIST, SEED)["kld"]
    res = run.kld_realizations(NDIST, SEED, error="resample")["kld"]
    assert (jit >= 0).all()  # (the jitter divergence is a true one: both distributions normalised over the same points)
    assert res.min() < 0 < res.mean()  # (the bootstrap's is not, as the reference's: never clamped)
    reference_gates(jit, g["golden/jitter_approx/kld"], f"{label} kld jitter vs approx=True")
    reference_gates(jit, g["golden/jitter_exact/kld"], f"{label} kld jitter vs exact")
    reference_gates(res, g["golden/resample/kld"], f"{label} kld resample")


def test_distributions_against_reference(fix):
    distribution_gates(run_of("golden"), fix, "host")


def check_stopping(run, fix, label):
    for i, args in enumerate(STOP_ARGS):
        flag, vals = run.stopping_function(return_vals=True, **args)
        want = fix[0][f"golden/stop/{i}"]
        np.testing.assert_allclose(vals, want[:3], rtol=1e-12, atol=0)
        assert flag == bool(want[3]) and run.stopping_function(**args) == flag
    np.testing.assert_allclose(run.stopping_function(return_vals=True)[1], (13.2850, 2.5499, 13.2850), rtol=2e-5)
    for error in MODES:
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # (n_mc >= 20: no warning)
            flag, (post, evid, stop) = run.stopping_function(pfrac=0.3, evid_thresh=0.02, n_mc=24, error=error, seed=5,
                                                             return_vals=True)
        lz = (run.logz_realizations(24, 5) if error == "jitter" else
              run.bootstrap_realizations(24, 5, jitter=error == "simulate"))["logz"]
        assert evid == np.std(lz) / 0.02 and post == 10000 / run._err_summary()[1]
        assert stop == 0.3 * post + (1. - 0.3) * evid and flag == (stop <= 1.)
    print(f"[merge dynamic {label}] stopping function {run.stopping_function(return_vals=True)}")


def test_stopping_function(fix):
    check_stopping(run_of("golden"), fix, "host")


def check_argument_rules(run):
    for kw in (dict(pfrac=-0.1), dict(pfrac=1.1), dict(pfrac=np.nan), dict(maxfrac=-0.1), dict(maxfrac=1.5),
               dict(maxfrac=np.nan), dict(pad=-1)):
        with pytest.raises(ValueError):
            run.weight_function(**kw)
    with pytest.raises(ValueError, match="largest"):
        run.weight_function(maxfrac=1.0)
    for kw in (dict(pfrac=1.5), dict(pfrac=0.5, evid_thresh=-1.), dict(target_n_effective=-1), dict(n_mc=-1),
               dict(error="bootstrap")):
        with pytest.raises(ValueError):
            run.stopping_function(**kw)
    with pytest.warns(UserWarning, match="small number"):
        run.stopping_function(n_mc=3)
    with pytest.raises(ValueError):
        run.kld_realizations(2, error="other")
    with pytest.raises(ValueError):
        run.kld_realizations(0)
    with pytest.raises(ValueError):
        run.kld_realizations(65537)
    with pytest.raises(ValueError):
        run.kld_realizations(1, first=-1)
    with pytest.raises(ValueError):
        run.kld_realizations(1, seed=-1)
    with pytest.raises(ValueError):
        run.kld_error(error="jitter", mult=np.ones(3, dtype=np.int64))
    with pytest.raises(ValueError):
        run.kld_error(error="resample", mult=np.ones(3, dtype=np.int64))
    with pytest.raises(ValueError):
        run.kld_error(first=run.niter, count=1)
    with pytest.raises(ValueError):
        run.kld_error(index=-1)


def test_argument_rules():
    m = run_of("golden")
    check_argument_rules(m)
    # a point of weight 0 adds nothing; a positive weight where the run's own is 0 is an infinite divergence
    from dynesty_amd import errors
    lw = np.array([-1.0, -np.inf, -2.0])
    assert np.isfinite(errors._kld_of(lw[None, :], np.array([-1.0, -np.inf, -2.0]), 0.0)[0][0])
    assert errors._kld_of(lw[None, :], np.array([-1.0, -3.0, -np.inf]), 0.0)[0][0] == np.inf
    assert errors._kld_cum(lw, np.array([-1.0, -3.0, -np.inf]), 0.0)[-1] == np.inf
    assert np.isfinite(errors._kld_cum(lw, np.array([-1.0, -np.inf, -2.0]), 0.0)).all()


def degenerate_args():
    args = merge_cases.make(np.random.default_rng(3), [50, 60], 20, 2)
    args["dead_logl"] = [np.full(len(d), -1.e300) for d in args["dead_logl"]]
    args["live_logl"][:] = -1.e300
    return args


def test_degenerate_run_has_equal_zweights():
    """All ln L = -1e300: the cumulative ln Z cannot move (the reference's np.ptp(logz) == 0 branch)."""
    m = merge_cases.host_merge(degenerate_args(), prior_transform=lambda u: 20.0 * u - 10.0)
    assert m.logz[0] == m.logz[-1]
    (lo, hi), (pw, zw, w) = m.weight_function(pfrac=0.0, return_weights=True)
    np.testing.assert_array_equal(zw, np.full(m.niter, 1.0 / m.niter))
    np.testing.assert_array_equal(w, zw)
    assert (lo, hi) == (-np.inf, np.inf)
    assert dr.weights_hp(m, 0.0)["degenerate"]
