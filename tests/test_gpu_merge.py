"""The combiner on the device (csrc/merge.hip, dh_merge_runs): the merged run's order and integer fields are exact
against the reference's merged run (tests/golden/merge.npz) and the host combiner; the floating-point fields are held
to the long-double restatement (tests/merge_hp_ref.py) at the bounds it derives; moments and equal-weight samples
against the reference's (tests/golden/merge_device.npz).

Worst measured error / bound per field is recorded in DESIGN.md section 3.8."""
import os

import numpy as np
import pytest

import inputs
import merge_cases
import merge_hp_ref as hp

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOAT_FIELDS = ("logvol", "logwt", "logz", "information", "logzerr", "weights")


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "merge.npz")), np.load(os.path.join(GOLD, "merge_device.npz"))


def golden_args(g):
    di = g["static/dead_i"]
    return dict(niter=g["static/nit"], dead_logl=g["static/dead_l"], live_logl=g["static/live_l"],
                dead_u=g["static/dead_u"], live_u=g["static/live_u"], dead_id=di[0], dead_it=di[1], dead_nc=di[2],
                live_it=g["static/live_it"])


def problem_for(D):
    from dynesty_amd import problems
    return inputs.problem("C1") if D == 3 else problems.gauss_corr(D, 0.4, 5.0, f"G{D}")


def check_floats(m, ref, label):
    """Every floating-point field within its derived bound of the long-double value; prints the worst ratio."""
    b = hp.bounds(ref)
    for k in FLOAT_FIELDS:
        want = np.asarray(ref[k], dtype=np.float64)
        got = np.asarray(m[k] if k != "weights" else m["weights"])
        err = np.abs(got - want)
        ok = err <= b[k]
        ratio = float(np.max(err / np.maximum(b[k], 1e-300)))
        print(f"[merge {label}] {k}: worst error / bound = {ratio:.3g} (max error {err.max():.3g})")
        assert ok.all(), (label, k, int(np.argmin(ok)), float(err[np.argmin(ok)]), float(b[k][np.argmin(ok)]))
    return b


@pytest.fixture(scope="module")
def gold_device(gold):
    """The golden case merged once; everything downloaded once.  A context holds one merged run, and the tests below
    go on asking this one for moments and samples, so it has a context of its own: `ctx` is for the tests that
    merge."""
    from dynesty_amd import _lib
    g, _ = gold
    d = _lib.Context(0).merge_runs(inputs.problem("C1"), **golden_args(g))
    m = d.to_merged_run()
    m["weights"] = d.importance_weights()
    return d, m


def test_golden_fields_match_reference(ctx, gold, gold_device):
    """Every assertion of test_merge_static_runs_matches_reference_fields, at that file's tolerances."""
    g, _ = gold
    d, m = gold_device

    def ref(k):
        return g["ref/" + k]
    np.testing.assert_array_equal(m.samples_id, ref("samples_id"))
    np.testing.assert_array_equal(m.samples_it, ref("samples_it"))
    np.testing.assert_array_equal(m.ncall, ref("ncall"))
    assert m.niter == ref("niter") == d.summary["niter"]
    np.testing.assert_array_equal(m.logl, ref("logl"))
    np.testing.assert_array_equal(m.samples_n, ref("samples_n"))
    np.testing.assert_array_equal(m.samples_u, ref("samples_u"))
    np.testing.assert_allclose(m.samples, ref("samples"), rtol=0, atol=1e-14)
    np.testing.assert_allclose(m.logvol, ref("logvol"), rtol=0, atol=1e-11)
    np.testing.assert_allclose(m.logwt, ref("logwt"), rtol=0, atol=1e-10)
    np.testing.assert_allclose(m.logz, ref("logz"), rtol=0, atol=1e-10)
    np.testing.assert_allclose(m.information, ref("information"), rtol=0, atol=1e-9)
    np.testing.assert_allclose(m.logzerr, ref("logzerr"), rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(m["weights"], ref("importance_weights"), rtol=1e-9, atol=1e-300)
    assert abs(m.eff - ref("eff")) < 1e-9
    # samples are dh_problem_eval's of the same rows, bit for bit
    v, _ = ctx.problem_eval(inputs.problem("C1"), m.samples_u)
    np.testing.assert_array_equal(m.samples, v)
    s = d.summary
    assert s["logz"] == m.logz[-1] and s["logzerr"] == m.logzerr[-1] and s["h"] == m.information[-1]
    assert s["ncall"] == int(ref("ncall").sum())
    assert abs(s["ess"] - 1. / np.sum(m["weights"] ** 2)) <= 1e-12 * s["ess"]


def test_golden_floats_within_derived_bounds(gold, gold_device):
    g, _ = gold
    _, m = gold_device
    ref = hp.merge_hp(g["static/dead_l"], g["static/nit"], g["static/live_l"])
    check_floats(m, ref, "golden")


def test_golden_fetch_in_unaligned_slices(gold_device):
    d, m = gold_device
    M = d.niter
    cuts = [0, 1, 67, 300, 301, 1029, M - 1, M]
    for name, key in (("logz", "logz"), ("samples", "samples"), ("samples_n", "samples_n"), ("samples_u", "samples_u")):
        parts = [d.field(name, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        np.testing.assert_array_equal(np.concatenate(parts), m[key])
    assert len(d.field("logl", M, 0)) == 0
    with pytest.raises(ValueError):
        d.field("logl", M - 1, 2)
    with pytest.raises(ValueError):
        d.field("nothing")


def test_golden_logz_set(ctx, gold):
    """merge.npz logz/*: 4 runs, N = 100 (values only: the coordinates are not part of that set)."""
    g, _ = gold
    nit = g["logz/nit"]
    R, N = g["logz/live"].shape
    rng = np.random.default_rng(3)
    d = ctx.merge_runs(inputs.problem("C1"), nit, g["logz/dead"], g["logz/live"],
                       rng.random((R, g["logz/dead"].shape[1], 3)), rng.random((R, N, 3)))
    np.testing.assert_allclose(d.summary["logz"], g["logz/logz"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(d.summary["logzerr"], g["logz/logzerr"], rtol=1e-9)
    assert d.summary["ncall"] == 0
    with pytest.raises(ValueError):
        d.field("ncall")


def test_moments_match_reference(gold, gold_device):
    g, gd = gold
    d, m = gold_device
    ref = hp.merge_hp(g["static/dead_l"], g["static/nit"], g["static/live_l"], samples=g["ref/samples"])
    b = hp.bounds(ref)
    b_mean, b_cov = hp.moment_bounds(ref, b["rel_w"])
    mean, cov = d.mean_and_cov()
    # the device's samples differ from the reference's by <= 1e-14 (prior transform): that enters the mean as is
    # and the covariance through sum w |dx|
    slack_mean = 1e-14
    slack_cov = 2e-14 * np.add.outer(np.asarray(ref["abs_dx"], dtype=np.float64), np.asarray(ref["abs_dx"], dtype=np.float64)) * float(ref["norm"])
    e_mean = np.abs(mean - np.asarray(ref["mean"], dtype=np.float64))
    e_cov = np.abs(cov - np.asarray(ref["cov"], dtype=np.float64))
    print(f"[merge golden] mean: worst error / bound = {np.max(e_mean / (b_mean + slack_mean)):.3g}; "
          f"cov: {np.max(e_cov / (b_cov + slack_cov)):.3g}")
    assert (e_mean <= b_mean + slack_mean).all(), (e_mean, b_mean)
    assert (e_cov <= b_cov + slack_cov).all(), (e_cov, b_cov)
    # and the reference's own float64 values at a tolerance no laxer than the bounds' scale
    np.testing.assert_allclose(mean, gd["mean"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(cov, gd["cov"], rtol=0, atol=1e-12)


def test_resample_equal_matches_reference_row_for_row(gold, gold_device):
    g, gd = gold
    d, m = gold_device
    for s in range(4):
        got = d.resample_equal(rstate=np.random.default_rng(s))
        want = gd[f"resample/{s}"]
        # the reference's rows are its own samples (1e-14 from the device's): compare the rows' identities exactly
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-14)
        rs = np.random.default_rng(s)
        idx = d.resample_indices(rs.random(), d.niter)[rs.permutation(d.niter)]
        np.testing.assert_array_equal(got, m.samples[idx])
        np.testing.assert_array_equal(g["ref/samples"][idx], want)


def test_resample_multiplicities(gold_device):
    """With n_out = 3 M + 1 every point's multiplicity lies within 1 of w_j n_out."""
    d, m = gold_device
    n = 3 * d.niter + 1
    for u0 in (0.0, 0.37, 0.999999):
        idx = d.resample_indices(u0, n)
        assert (np.diff(idx) >= 0).all() and idx[0] >= 0 and idx[-1] < d.niter
        mult = np.bincount(idx, minlength=d.niter)
        assert (np.abs(mult - m["weights"] * n) < 1 + 1e-6).all()
    # the indices stay on the device: a gather without indices returns the same rows
    ctx = d.ctx
    out = np.empty((5, 3))
    ctx._check_merge(ctx.lib.dh_merged_gather(ctx.handle, 5, None, out.ctypes.data))
    np.testing.assert_array_equal(out, m.samples[idx[:5]])


CASES = merge_cases.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_synthetic_cases(ctx, name):
    """Ties and edges: order and integer fields exact against the host combiner, the rest against the long-double
    values at the derived bounds."""
    args = CASES[name]
    D = args["live_u"].shape[2]
    prob = problem_for(D)
    host = merge_cases.host_merge(args)
    d = ctx.merge_runs(prob, **args)
    m = d.to_merged_run()
    m["weights"] = d.importance_weights()
    assert m.niter == host.niter == int(args["niter"].sum()) + args["live_logl"].size
    for k in ("logl", "samples_n", "samples_run", "samples_seq", "samples_id", "samples_it", "ncall", "samples_u"):
        np.testing.assert_array_equal(m[k], host[k], err_msg=k)
    fin = d.field("final")
    np.testing.assert_array_equal(fin, (host.samples_seq >= args["niter"][host.samples_run]).astype(np.int32))
    if name == "d_single":
        np.testing.assert_array_equal(m.samples_seq, np.arange(m.niter))
    v, _ = ctx.problem_eval(prob, m.samples_u)
    np.testing.assert_array_equal(m.samples, v)
    ref = hp.merge_hp(args["dead_logl"], args["niter"], args["live_logl"], samples=m.samples)
    b = check_floats(m, ref, name)
    if name == "g_span":
        # a scan that subtracted the global maximum would underflow where the long-double value is finite
        finite = np.isfinite(np.asarray(ref["logz"], dtype=np.float64))
        assert finite.all() and np.isfinite(m.logz[finite]).all() and np.isfinite(m.logwt).all()
        assert m.logz[0] < m.logz[-1] - 1500
    mean, cov = d.mean_and_cov()
    b_mean, b_cov = hp.moment_bounds(ref, b["rel_w"])
    e_mean = np.abs(mean - np.asarray(ref["mean"], dtype=np.float64))
    e_cov = np.abs(cov - np.asarray(ref["cov"], dtype=np.float64))
    print(f"[merge {name}] mean: worst error / bound = {np.max(e_mean / b_mean):.3g}; cov: {np.max(e_cov / b_cov):.3g}")
    assert (e_mean <= b_mean).all() and (e_cov <= b_cov).all()
    # ESS = 1 / sum w^2: twice the weights' relative bound, and the chain of the chunked sum
    c = hp.moment_chain(m.niter, D + 2)
    assert abs(d.summary["ess"] - float(ref["ess"])) <= (4 * float(np.max(b["rel_w"])) + (c + 4) * hp.U) * d.summary["ess"]


def test_errors(ctx, gold):
    g, _ = gold
    prob = inputs.problem("C1")
    args = golden_args(g)
    bad = dict(args, dead_logl=args["dead_logl"].copy())
    bad["dead_logl"][1, 5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        ctx.merge_runs(prob, **bad)
    with pytest.raises(ValueError):  # id / it / nc come together
        ctx.merge_runs(prob, **dict(args, dead_nc=None))
    with pytest.raises(ValueError):  # problem of another dimension
        ctx.merge_runs(problem_for(7), **args)
    first = ctx.merge_runs(prob, **args)
    second = ctx.merge_runs(prob, **merge_cases.cases()["d_single"])
    with pytest.raises(ValueError):  # a second merge replaces the first
        first.field("logl")
    assert second.field("logl").shape == (second.niter,)
    with pytest.raises(ValueError, match="kept"):  # a call rejected for its arguments touches nothing
        ctx.merge_kept(prob)
    assert second.field("logl").shape == (second.niter,)
    down = dict(args, dead_logl=args["dead_logl"].copy())
    down["dead_logl"][0, :2] = down["dead_logl"][0, 1::-1]  # -99.7 before -103.5
    with pytest.raises(ValueError, match="decrease"):  # found on the device: the earlier merged run is gone
        ctx.merge_runs(prob, **down)
    with pytest.raises(ValueError):
        second.field("logl")
    second.release()
    with pytest.raises(ValueError):
        second.field("logl")
    with pytest.raises(ValueError):  # nothing on the device any more
        ctx._check_merge(ctx.lib.dh_merged_fetch(ctx.handle, 0, 0, 0, None))


def test_merge_kept_needs_a_kept_ensemble():
    from dynesty_amd import _lib
    c = _lib.Context(0)
    with pytest.raises(ValueError, match="kept"):
        c.merge_kept(inputs.problem("C1"))
    c.close()
