"""Dynamic batches folded into the merged run on the device (csrc/merge_fold.hip, dh_merged_fold; DESIGN.md section
3.8.5): the reference's own dynamic run (tests/golden/batch_combine.npz) fold after fold; synthetic bases and batches
(tests/fold_cases.py) against the host's one-pass form dynamic.merge_strands -- order, integer fields and unit-cube rows
exactly, the float fields at the project's tolerances (logvol 1e-11, logwt / logz 1e-10, information 1e-9, logzerr rtol
1e-7 + 1e-10) and at the bounds the long-double restatement (tests/fold_hp_ref.py) derives; the error paths, which leave
the base run in place; the calls that go on working on a folded run against the same calls on its host copy; and
run_dynamic(merge='device') against merge='host'.  Every test prints its worst error over the tolerance; the table is in
DESIGN.md section 3.8.5."""
import os

import numpy as np
import pytest

import fold_cases
import fold_hp_ref
import inputs
import marginals_hp_ref as mq
import merge_cases
import merge_dynamic_ref as dr
import merge_errors_ref as er
import merge_hp_ref as hp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_combine.npz")
# field -> (rtol, atol): tests/test_dynamic_cpu.py's
TOL = dict(logvol=(0., 1e-11), logwt=(0., 1e-10), logz=(0., 1e-10), information=(0., 1e-9), logzerr=(1e-7, 1e-10))
INT_FIELDS = ("samples_n", "samples_batch", "samples_seq", "samples_run")
PT_FIELDS = ("samples_id", "samples_it", "ncall")


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def problem_for(D):
    from dynesty_amd import problems
    return inputs.problem("C1") if D == 3 else problems.gauss_iid(D, 10.0, f"I{D}")


def check_tolerances(got, want, label):
    """Every float field within its tolerance of `want` (a dict of arrays); prints the worst error / tolerance."""
    for k, (rtol, atol) in TOL.items():
        w = np.asarray(want[k], dtype=np.float64)
        err, tol = np.abs(np.asarray(got[k]) - w), atol + rtol * np.abs(w)
        print(f"[fold {label}] {k}: worst error / tolerance = {float(np.max(err / tol)):.3g} (max error {err.max():.3g})")
        assert (err <= tol).all(), (label, k, int(np.argmax(err / tol)), float(err.max()))


def check_bounds(got, weights, ref, label):
    """The device's floats within the restatement's derived bounds; prints the worst error / bound."""
    b = fold_hp_ref.bounds(ref)
    for k in ("logvol", "logwt", "logz", "information", "logzerr", "weights"):
        err = np.abs(np.asarray(weights if k == "weights" else got[k]) - np.asarray(ref[k], dtype=np.float64))
        print(f"[fold {label}] {k}: worst error / derived bound = {float(np.max(err / np.maximum(b[k], 1e-300))):.3g}")
        assert (err <= b[k]).all(), (label, k, int(np.argmax(err / np.maximum(b[k], 1e-300))), float(err.max()))
    return b


def test_golden_chain_fold_after_fold(ctx):
    """The reference's dynamic run: the base (one static run: 533 dead points and 50 final live ones) merged on the
    device, then its three batches folded one after the other, each compared with the reference's saved run after it."""
    g = np.load(GOLDEN)
    prob = inputs.problem("C1")
    f = {k: g[f"0/base/{k}"] for k in ("logl", "id", "it", "nc", "u")}
    K, N = len(f["logl"]) - 50, 50
    slot = f["id"][K:]
    assert sorted(slot) == list(range(N)) and (f["nc"][K:] == 1).all()
    live_l, live_u, live_it = np.empty((1, N)), np.empty((1, N, 3)), np.empty((1, N), dtype=np.int64)
    live_l[0, slot], live_u[0, slot], live_it[0, slot] = f["logl"][K:], f["u"][K:], f["it"][K:]
    d = ctx.merge_runs(prob, [K], [f["logl"][:K]], live_l, [f["u"][:K]], live_u, dead_id=[f["id"][:K]],
                       dead_it=[f["it"][:K]], dead_nc=[f["nc"][:K]], live_it=live_it)
    np.testing.assert_array_equal(d.field("samples_id"), f["id"])
    np.testing.assert_array_equal(d.field("samples_batch"), np.zeros(K + N, dtype=np.int32))  # no batch yet
    assert d.batch_nlive == [] and d.batch_bounds == []
    for b in range(3):
        s = {k: g[f"{b}/new/{k}"] for k in ("logl", "id", "it", "nc", "u")}
        k = len(s["logl"]) - N
        slot = s["id"][k:]
        live_l[0, slot], live_u[0, slot], live_it[0, slot] = s["logl"][k:], s["u"][k:], s["it"][k:]
        lmin, lmax = g[f"{b}/new_bounds"]
        old = d
        d = ctx.merged_fold(old, prob, [k], [s["logl"][:k]], live_l, [s["u"][:k]], live_u, dead_id=[s["id"][:k]],
                            dead_it=[s["it"][:k]], dead_nc=[s["nc"][:k]], live_it=live_it, logl_min=lmin, logl_max=lmax)
        with pytest.raises(ValueError, match="no longer on the device"):
            old.field("logl", 0, 1)
        m = d.to_merged_run()

        def ref(key):
            return g[f"{b}/after/{key}"]
        np.testing.assert_array_equal(m.logl, ref("logl"))
        np.testing.assert_array_equal(m.samples_n, ref("n"))
        np.testing.assert_array_equal(m.samples_id, ref("id"))
        np.testing.assert_array_equal(m.samples_batch, ref("batch"))
        np.testing.assert_array_equal(m.samples_it, ref("it"))
        np.testing.assert_array_equal(m.ncall, ref("nc"))
        np.testing.assert_array_equal(m.samples_u, ref("u"))
        np.testing.assert_array_equal(m.samples_run, np.zeros(len(m.logl), dtype=np.int64))
        check_tolerances(m, dict(logvol=ref("logvol"), logwt=ref("logwt"), logz=ref("logz"), information=ref("h"),
                                 logzerr=np.sqrt(ref("logzvar"))), f"golden batch {b}")
        np.testing.assert_array_equal(m.samples, ctx.problem_eval(prob, m.samples_u)[0])
        assert d.batch_nlive == m.batch_nlive == ref("batch_nlive").tolist()
        np.testing.assert_array_equal(np.array(d.batch_bounds), ref("batch_bounds"))
        assert d.niter == len(ref("logl")) and d.summary["logz"] == m.logz[-1] and d.summary["ncall"] == int(ref("nc").sum())
        assert int(d.field("final").sum()) == N * (b + 2)


def fold_case(ctx, name):
    """(base handle's host copy as one run, folded device run, host's one-pass fold, problem, case arguments)."""
    from dynesty_amd import dynamic
    kw = fold_cases.CASES[name]
    base, new, lmin, lmax = fold_cases.make(**kw)
    prob = problem_for(kw["D"])
    d0 = ctx.merge_runs(prob, **base)
    mb = dynamic.single_run(d0.to_merged_run())
    pt = kw.get("pt", True)
    if not pt:  # (the host's forms want ids: zeros, left out of the comparison)
        mb["samples_id"] = np.zeros(len(mb.logl), dtype=np.int64)
    strands = fold_cases.host_strands(new, kw["strand_nlive"], lambda u: ctx.problem_eval(prob, u)[0])
    want = dynamic.merge_strands(mb, strands, lmin, lmax)
    d = ctx.merged_fold(d0, prob, logl_min=lmin, logl_max=lmax, **new)
    return mb, d, want, prob, kw


@pytest.mark.parametrize("name", sorted(fold_cases.CASES))
def test_synthetic_cases_against_the_host_one_pass_form(ctx, name):
    mb, d, want, prob, kw = fold_case(ctx, name)
    pt = kw.get("pt", True)
    m = d.to_merged_run()
    T = len(want.logl)
    assert d.niter == T > 2048 and d.have_pt == pt
    np.testing.assert_array_equal(m.logl, want.logl)
    np.testing.assert_array_equal(m.samples_u, want.samples_u)
    np.testing.assert_array_equal(m.samples, want.samples)  # old rows moved, new rows dh_problem_eval's: bit for bit
    np.testing.assert_array_equal(m.samples, ctx.problem_eval(prob, m.samples_u)[0])
    for k in INT_FIELDS + (PT_FIELDS if pt else ()):
        np.testing.assert_array_equal(m[k], want[k], err_msg=k)
    if not pt:
        for k in PT_FIELDS:
            with pytest.raises(ValueError):
                d.field(k)
    assert d.batch_nlive == want.batch_nlive and d.batch_bounds == want.batch_bounds
    assert int(d.field("final").sum()) == 3 * kw["base_nlive"] + kw["R"] * kw["strand_nlive"]
    for lo, hi in kw["plateaus"]:  # the plateaus lie where the case says, base and strand points in each
        assert (m.logl[lo:hi] == m.logl[lo]).all() and set(m.samples_batch[lo:hi] > 0) == {False, True}
    check_tolerances(m, want, name)
    ref = fold_hp_ref.fold_hp(m.logl, m.samples_n, samples=m.samples)
    b = check_bounds(m, d.importance_weights(), ref, name)
    mean, cov = d.mean_and_cov()
    b_mean, b_cov = hp.moment_bounds(ref, b["rel_w"])
    e_mean, e_cov = np.abs(mean - np.asarray(ref["mean"], dtype=np.float64)), np.abs(cov - np.asarray(ref["cov"], dtype=np.float64))
    print(f"[fold {name}] mean: worst error / bound = {np.max(e_mean / b_mean):.3g}; cov: {np.max(e_cov / b_cov):.3g}")
    assert (e_mean <= b_mean).all() and (e_cov <= b_cov).all()
    s = d.summary
    assert s["logz"] == m.logz[-1] and s["logzerr"] == m.logzerr[-1] and s["h"] == m.information[-1]
    assert s["ncall"] == (int(want.ncall.sum()) if pt else 0)


def small_base(ctx, seed=11):
    rng = np.random.default_rng(seed)
    prob = problem_for(3)
    return prob, ctx.merge_runs(prob, **merge_cases.make(rng, [100, 90], 20, 3)), rng


def snapshot(d):
    return {k: d.field(k) for k in ("logl", "logz", "samples_n", "samples_id", "samples_u", "samples_batch")}


def test_errors_leave_the_base_run_in_place(ctx):
    from dynesty_amd import _lib
    prob, d, rng = small_base(ctx)
    before, summary = snapshot(d), dict(d.summary)

    def intact():
        assert d.summary == summary
        for k, v in snapshot(d).items():
            np.testing.assert_array_equal(v, before[k], err_msg=k)
    top = float(before["logl"][-1])
    lmin = float(before["logl"][50])
    good = merge_cases.make(rng, [30, 25], 10, 3)
    for k in ("dead_logl",):
        good[k] = [x + top + 40.0 for x in good[k]]
    good["live_logl"] = good["live_logl"] + top + 40.0
    # a strand point at logl_min; an over-long plateau (12 equal values above the base's end, entered at n = 2 x 10)
    low = {k: (list(v) if isinstance(v, list) else v.copy()) for k, v in good.items()}
    low["dead_logl"][0] = np.concatenate([[lmin], good["dead_logl"][0][1:]])
    flat = {k: (list(v) if isinstance(v, list) else v.copy()) for k, v in good.items()}
    flat["dead_logl"] = [np.full(30, top + 1.0), np.full(25, top + 1.0)]
    for bad, msg in ((low, "logl_min"), (flat, "plateau")):
        with pytest.raises(ValueError, match=msg):
            ctx.merged_fold(d, prob, logl_min=lmin, logl_max=np.inf, **bad)
        intact()
    down = {k: (list(v) if isinstance(v, list) else v.copy()) for k, v in good.items()}
    down["dead_logl"][1] = good["dead_logl"][1][::-1].copy()
    nan = {k: (list(v) if isinstance(v, list) else v.copy()) for k, v in good.items()}
    nan["live_logl"][0, 3] = np.nan
    for bad in (down, nan):
        with pytest.raises(ValueError):
            ctx.merged_fold(d, prob, logl_min=lmin, logl_max=np.inf, **bad)
        intact()
    # shapes and arguments: nothing is touched
    no_pt = {k: v for k, v in good.items() if k not in ("dead_id", "dead_it", "dead_nc", "live_it")}
    half = dict(no_pt, dead_id=good["dead_id"])
    wrong_u = dict(good, live_u=good["live_u"][:, :, :2])
    other = problem_for(33)
    for call in (lambda: ctx.merged_fold(d, prob, logl_min=lmin, logl_max=np.inf, **no_pt),
                 lambda: ctx.merged_fold(d, prob, logl_min=lmin, logl_max=np.inf, **half),
                 lambda: ctx.merged_fold(d, prob, logl_min=lmin, logl_max=np.inf, **wrong_u),
                 lambda: ctx.merged_fold(d, other, logl_min=lmin, logl_max=np.inf, **dict(good, live_u=np.zeros((2, 10, 33)),
                                                                                          dead_u=[np.zeros((30, 33)), np.zeros((25, 33))])),
                 lambda: ctx.merged_fold(d, prob, logl_min=lmin, logl_max=lmin, **good),
                 lambda: ctx.merged_fold(d, prob, logl_min=np.nan, logl_max=np.inf, **good),
                 lambda: ctx.merged_fold(d, prob, logl_min=np.inf, logl_max=np.inf, **good)):
        with pytest.raises(ValueError):
            call()
        intact()
    P = _lib._ptr
    nit, ll, lu = np.array([0], dtype=np.int64), np.full((1, 4), top + 1.0), np.full((1, 4, 3), 0.5)
    h, past = ctx.problem(prob), np.array([d.niter], dtype=np.int64)
    for rc in (ctx.lib.dh_merged_fold(ctx.handle, h, 0, 4, 0, P(nit), None, P(ll), None, P(lu), None, None, None, None, lmin, np.inf, None),
               ctx.lib.dh_merged_fold(ctx.handle, h, 1, 0, 0, P(nit), None, P(ll), None, P(lu), None, None, None, None, lmin, np.inf, None),
               ctx.lib.dh_merged_fold(ctx.handle, h, 1, 4, 0, P(nit), None, P(ll), None, P(lu), None, None, None, None, -np.inf, np.inf, None),
               ctx.lib.dh_merged_fold(ctx.handle, h, 1, 4, 0, P(nit), None, P(ll), None, P(lu), None, None, None, None, lmin, lmin, None),
               ctx.lib.dh_merged_fold(ctx.handle, h, 1, 4, 0, P(nit), None, P(ll), None, P(lu), None, None, None, None, lmin, np.inf, None),
               ctx.lib.dh_merged_gather_rows(ctx.handle, 0, 1, P(nit), P(ll)),
               ctx.lib.dh_merged_gather_rows(ctx.handle, 7, 1, P(past), P(ll))):
        assert rc == _lib.ERR_ARG  # (the fifth: id / it / nc on the merged run's side only)
    intact()
    # a fold that succeeds: the old handle is stale; the strand bootstrap is refused on the folded run
    assert np.isfinite(d.bootstrap_realizations(2, seed=1)["logz"]).all()
    new = ctx.merged_fold(d, prob, logl_min=lmin, logl_max=np.inf, **good)
    with pytest.raises(ValueError, match="no longer on the device"):
        d.field("logl", 0, 1)
    assert new.niter == len(before["logl"]) + 30 + 25 + 20 and new.batch_nlive == [40, 10, 10]
    np.testing.assert_array_equal(new.field("logl")[:len(before["logl"])], before["logl"])  # (the strands lie above)
    with pytest.raises(ValueError, match="dynamic batches"):
        new.bootstrap_realizations(2, seed=1)
    with pytest.raises(ValueError, match="dynamic batches"):
        new.kld_error(1, 0, "resample")
    with pytest.raises(ValueError, match="dynamic batches"):
        new.resample_run(seed=1)
    assert np.isfinite(new.logz_realizations(4, seed=1)["logz"]).all()
    # no merged run at all
    from dynesty_amd import _lib as lib2
    c2 = lib2.Context(0)
    rc = c2.lib.dh_merged_fold(c2.handle, c2.problem(prob), 1, 4, 0, P(nit), None, P(ll), None, P(lu), None, None, None, None,
                               lmin, np.inf, None)
    assert rc == _lib.ERR_ARG


@pytest.fixture(scope="module")
def folded():
    """One folded run on a context of its own, with its host copy."""
    from dynesty_amd import _lib
    _, d, _, prob, _ = fold_case(_lib.Context(0), "three_strands_d33")
    return d, d.to_merged_run()


def test_follow_up_calls_on_the_folded_run_against_its_host_copy(folded):
    d, m = folded
    # the volume realizations: both are float64 evaluations of one exact value, each within its own chains' bound
    dev, host = d.logz_realizations(3, 31, 5, means=True), m.logz_realizations(3, 31, 5, means=True)
    worst = 0.0
    for i in range(3):
        ref = er.realization_hp(m.logl, m.samples_n, 31, 5 + i, True, None, m.samples)
        bd, bh = er.bounds(ref, er.device_chains(ref["M"])), er.bounds(ref, er.host_chains(ref["M"]))
        for k, bk in (("logz", "logz_last"), ("information", "information"), ("ess", "ess"), ("mean", "mean")):
            worst = max(worst, er.check(dev[k][i], host[k][i], bd[bk] + bh[bk], f"fold device vs host r+{i} {k}"))
    print(f"[fold follow-up] volume realizations: worst error / bound against the host form {worst:.3g}")
    # the weight function: the weights within bound of the restatement, the indices decided by it, the bounds the host's
    chain = dr.device_chains(d.niter)["scan"]
    h = dr.weights_hp(m, 0.8)
    b = dr.weight_bounds(h, 0.8, chain)
    worst = max(dr.check(arr, h[k], b[k], f"fold weights {k}") for arr, k in zip(d._err_weights(0.8), ("pw", "zw", "w")))
    want, margin = dr.decide(h, b["w"], 0.8)
    assert margin > 1
    bounds, idx = d._err_weight_function(0.8, 0.8, 1)
    assert idx == want and bounds == m._err_weight_function(0.8, 0.8, 1)[0] == d.weight_function() == m.weight_function()
    print(f"[fold follow-up] weight function: worst error / bound of the weights {worst:.3g}, index margin {margin:.3g}")
    # quantiles: each within its own backward-error budget, the ends equal
    q = [0, 0.025, 0.5, 0.975, 1]
    got_d, got_h = d.quantile(q), m.quantile(q)
    cols = range(d.ndim)
    rd = mq.worst(m.samples, d.importance_weights(), cols, q, got_d, "device")
    rh = mq.worst(m.samples, m.importance_weights(), cols, q, got_h, "reference")
    print(f"[fold follow-up] quantiles: worst backward error / budget device {rd[0]:.3g}, host {rh[0]:.3g}")
    assert rd[0] <= 1 and rh[0] <= 1
    np.testing.assert_array_equal(got_d[:, [0, -1]], got_h[:, [0, -1]])
    # the moments against the host copy's rows and weights in long double (the bound: the synthetic cases' test)
    mean, cov = d.mean_and_cov()
    ref = hp.moments_hp(m.samples, m.importance_weights())
    np.testing.assert_allclose(mean, np.asarray(ref["mean"], dtype=np.float64), rtol=0, atol=1e-11)
    np.testing.assert_allclose(cov, np.asarray(ref["cov"], dtype=np.float64), rtol=1e-9, atol=1e-11)
    # the seeds' rows by a gather
    idx = np.array([0, d.niter - 1, 2047, 2048, 17, 17, 3000])
    np.testing.assert_array_equal(d.gather(idx, "samples_u"), m.samples_u[idx])
    np.testing.assert_array_equal(d.gather(idx, "samples"), m.samples[idx])
    np.testing.assert_array_equal(d.gather(idx), m.samples[idx])
    with pytest.raises(ValueError):
        d.gather(idx, "logl")
    with pytest.raises(ValueError):
        d.gather([d.niter], "samples_u")
    # equal-weight samples: the device's indices are the host's search over the same cumulative weights
    pick = d.resample_indices(0.37, 500)
    assert (np.diff(pick) >= 0).all() and 0 <= pick[0] and pick[-1] < d.niter
    np.testing.assert_array_equal(d.gather(pick), m.samples[pick])


def test_run_dynamic_on_the_device_equals_the_host_route(ctx):
    """A 3-D Gaussian, 2 base runs of 100 live points, 2 batches of 2 strands of 100: both routes choose the same seeds
    (the same Generator calls on weights that agree to the last bit where the choice is concerned -- were that to fail,
    the strands would differ and the exact comparisons below with them) and run the same PCG64 streams, so the order,
    the integer fields and the unit-cube rows are equal exactly and the floats within the tolerances."""
    from dynesty_amd import backend, dynamic, problems
    prob = problems.Problem(3, problems.LIKE_GAUSS_IID, [0.0], problems.PRIOR_AFFINE, [10.0, 0.0], name="gauss3_unnormalised")
    backend.set_backend(ctx)
    try:
        kw = dict(pfrac=0.8, entropy=(21, 3), queue_size=25, stop_kwargs=dict(target_n_effective=10 ** 9))
        mh, log_h = dynamic.run_dynamic(prob, 2, 100, 2, 100, 2, **kw)
        md, log_d = dynamic.run_dynamic(prob, 2, 100, 2, 100, 2, merge='device', **kw)
    finally:
        backend.set_backend(None)
    assert len(log_h) == len(log_d) == 3
    for a, b in zip(log_h[1:], log_d[1:]):
        assert a["bounds"] == b["bounds"] and a["prior"] == b["prior"] and a["niter"] == b["niter"] and a["ncall"] == b["ncall"]
    m = md.to_merged_run()
    np.testing.assert_array_equal(m.logl, mh.logl)
    np.testing.assert_array_equal(m.samples_u, mh.samples_u)
    np.testing.assert_array_equal(m.samples, mh.samples)
    for k in INT_FIELDS + PT_FIELDS:
        np.testing.assert_array_equal(m[k], mh[k], err_msg=k)
    assert md.batch_nlive == mh.batch_nlive and md.batch_bounds == mh.batch_bounds
    check_tolerances(m, mh, "run_dynamic device vs host")
