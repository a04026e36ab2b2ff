"""dh_ns_continue: a kept ensemble taken further.  With PCG64 streams any chain of legs that ends under criteria C
gives, run for run and bit for bit, what ONE ns_ensemble call under C gives -- whether the earlier legs were ended by
max_fills, maxiter, maxcall, logl_max or a looser dlogz.  The comparator is the uninterrupted ns_ensemble path."""
import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

RUNS, NLIVE, K, DLOGZ, MAX_ITER = 5, 200, 64, 0.1, 20000
RECORD = ("logz", "logzerr", "niter", "ncall", "h", "nbound", "status", "eff")
DEAD = ("dead_logl", "dead_u", "dead_id", "dead_it", "dead_nc")
LIVE = ("live_logl", "live_u", "live_it")

CONFIGS = {
    "rwalk-multi": ("G5", dict(sample="rwalk", bound="multi", walks=20)),
    "rslice-single": ("C1", dict(sample="rslice", bound="single")),
    "unif-multi-boot5": ("G5", dict(sample="unif", bound="multi", bootstrap=5)),
    "unif-balls-boot5": ("G5", dict(sample="unif", bound="balls", bootstrap=5)),
    "rwalk-multi-late": ("G5", dict(sample="rwalk", bound="multi", walks=20, forced_exact=False)),
}
STOPS = ["max_fills=3", "max_fills=9", "maxiter=150", "maxcall=6000", "dlogz=5.0", "logl_max=median"]


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def base_kw(cfg, runs=RUNS, first_run=0):
    pname, kw = CONFIGS[cfg]
    return inputs.problem(pname), dict(runs=runs, nlive=NLIVE, queue_size=K, entropy=[31, 4], first_run=first_run,
                                       max_iter=MAX_ITER, rebuild_sync=False, **kw)


_full = {}


def full_run(ctx, cfg):
    """the uninterrupted run of a configuration: computed once, shared, never changed"""
    if cfg not in _full:
        prob, kw = base_kw(cfg)
        r = ctx.ns_ensemble(prob, dlogz=DLOGZ, want_samples=True, **kw)
        assert (r["status"] == 0).all(), r["status"]
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _full[cfg] = r
    return _full[cfg]


def assert_same_runs(got, ref, rows=None):
    """records, dead ln L / u / id / it / nc (the rows each run produced) and the final live ln L / u / it"""
    sel = slice(None) if rows is None else rows
    for f in RECORD:
        np.testing.assert_array_equal(got[f], ref[f][sel], err_msg=f)
    for f in LIVE:
        np.testing.assert_array_equal(got[f], ref[f][sel], err_msg=f)
    for i, n in enumerate(got["niter"]):
        for f in DEAD:
            np.testing.assert_array_equal(got[f][i, :n], ref[f][sel][i, :n], err_msg=f"{f} of run {i}")


def first_leg_args(ctx, cfg, stop):
    name, val = stop.split("=")
    if name == "max_fills":
        return dict(dlogz=DLOGZ, max_fills=int(val))
    if name == "maxiter":
        return dict(dlogz=DLOGZ, maxiter=int(val))
    if name == "maxcall":
        return dict(dlogz=DLOGZ, maxcall=int(val))
    if name == "dlogz":
        return dict(dlogz=float(val))
    ref = full_run(ctx, cfg)
    dead = np.concatenate([ref["dead_logl"][i, :n] for i, n in enumerate(ref["niter"])])
    return dict(dlogz=DLOGZ, logl_max=float(np.median(dead)))


@pytest.mark.parametrize("stop", STOPS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_continued_equals_uninterrupted(ctx, cfg, stop):
    ref = full_run(ctx, cfg)
    prob, kw = base_kw(cfg)
    leg = ctx.ns_ensemble(prob, keep=True, **first_leg_args(ctx, cfg, stop), **kw)
    try:
        # the first leg really stopped short
        assert (leg["niter"] < ref["niter"]).all(), (leg["niter"], ref["niter"])
        if stop.startswith("maxiter"):
            assert (leg["niter"] == 151).all(), leg["niter"]
        if stop.startswith("max_fills"):
            assert (leg["status"] == 1).all() and leg["nfills"] == int(stop.split("=")[1])
        else:
            assert (leg["status"] == 0).all(), leg["status"]
        got = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    print(cfg, stop, "first leg niter", leg["niter"], "nbound", leg["nbound"], "rest", got["rest"], "fills",
          leg["nfills"], "+", got["nfills"])
    # ... and something was resumed: a criterion stop leaves queue entries behind, a max_fills stop none
    if stop.startswith("max_fills"):
        assert (got["rest"] == 0).all(), got["rest"]
    else:
        assert (got["rest"] >= 0).all() and (got["rest"] > 0).any(), got["rest"]
    assert_same_runs(got, ref)


def test_three_legs(ctx):
    ref = full_run(ctx, "rwalk-multi")
    prob, kw = base_kw("rwalk-multi")
    try:
        a = ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, max_fills=2, **kw)
        b = ctx.ns_continue(dlogz=DLOGZ, maxiter=400)
        assert (a["status"] == 1).all() and (b["niter"] == 401).all() and (b["status"] == 0).all()
        got = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    assert_same_runs(got, ref)


def test_unchanged_criteria_are_a_noop(ctx):
    prob, kw = base_kw("rwalk-multi")
    try:
        a = ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, maxiter=700, want_samples=True, **kw)
        assert (a["niter"] == 701).all()
        b = ctx.ns_continue(dlogz=DLOGZ, maxiter=700, want_samples=True)
        assert b["nfills"] == 0 and (b["rest"] == 0).all()
        assert_same_runs(b, a)
        # ... as often as one likes, and the ensemble is still the one that goes on to the uninterrupted result
        c = ctx.ns_continue(dlogz=DLOGZ, maxiter=700, want_samples=True)
        assert c["nfills"] == 0
        assert_same_runs(c, a)
        got = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    assert_same_runs(got, full_run(ctx, "rwalk-multi"))


def test_continued_shard_equals_rows_of_the_whole(ctx):
    ref = full_run(ctx, "rwalk-multi")
    prob, kw = base_kw("rwalk-multi", runs=2, first_run=3)
    try:
        leg = ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, maxiter=150, **kw)
        assert (leg["niter"] == 151).all()
        got = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    assert_same_runs(got, ref, rows=slice(3, 5))


def two_legs(ctx, prob, kw, first, final):
    ref = ctx.ns_ensemble(prob, dlogz=final, want_samples=True, **kw)
    assert (ref["status"] == 0).all(), ref["status"]
    try:
        leg = ctx.ns_ensemble(prob, keep=True, dlogz=final, **first, **kw)
        assert (leg["niter"] < ref["niter"]).all(), (leg["niter"], ref["niter"])
        got = ctx.ns_continue(dlogz=final, want_samples=True)
    finally:
        ctx.release_kept()
    return leg, got, ref


def test_large_live_set(ctx):
    """nlive 8200: ns_consume selects the K + 1 smallest live points first (its compact form) -- the slots the saved
    fill lists are then translated ones"""
    kw = dict(runs=2, nlive=8200, queue_size=64, sample="rwalk", bound="single", walks=20, entropy=[8, 2],
              max_iter=120000, rebuild_sync=False)
    leg, got, ref = two_legs(ctx, inputs.problem("C1"), kw, dict(maxiter=3000), 1.0)
    assert (leg["niter"] == 3001).all()
    assert_same_runs(got, ref)


def test_wide_walkers(ctx):
    """40-D: the wave-per-walker kernels of wide.hip write the queue's rows"""
    from dynesty_amd import problems
    kw = dict(runs=2, nlive=160, queue_size=32, sample="rslice", bound="single", entropy=[40], max_iter=MAX_ITER,
              rebuild_sync=False)
    leg, got, ref = two_legs(ctx, problems.gauss_iid(40), kw, dict(maxiter=200), 1.0)
    assert (leg["niter"] == 201).all()
    assert_same_runs(got, ref)


def test_philox_max_fills_legs_are_exact(ctx):
    prob, kw = base_kw("rwalk-multi")
    kw["rng"] = "philox"
    ref = ctx.ns_ensemble(prob, dlogz=DLOGZ, want_samples=True, **kw)
    try:
        a = ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, max_fills=5, **kw)
        b = ctx.ns_continue(dlogz=DLOGZ, max_fills=6)
        assert (a["status"] == 1).all() and (b["status"] == 1).all() and b["nfills"] == 6
        got = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    assert (got["rest"] == 0).all()
    assert_same_runs(got, ref)


def test_philox_criterion_chain_is_deterministic_and_unbiased(ctx):
    """After a criterion stop a Philox run resumes at a later ensemble fill than it would have reached uninterrupted:
    another draw, not the same one.  Twice the same bits; ln Z within the gate test_ensemble_logz applies to the
    uninterrupted loop at this shape."""
    prob = inputs.problem("G5")
    kw = dict(runs=16, nlive=400, queue_size=64, walks=25, bound="multi", entropy=[7, 7], rng="philox")

    def chain():
        try:
            a = ctx.ns_ensemble(prob, keep=True, dlogz=1.0, **kw)
            assert (a["status"] == 0).all()
            return a, ctx.ns_continue(dlogz=0.05, want_dead_logl=True)
        finally:
            ctx.release_kept()
    a, r1 = chain()
    _, r2 = chain()
    assert (r1["niter"] > a["niter"]).all() and (r1["status"] == 0).all()
    for f in RECORD + ("live_logl",):
        np.testing.assert_array_equal(r1[f], r2[f], err_msg=f)
    lz = r1["logz"]
    se = lz.std(ddof=1) / np.sqrt(len(lz))
    print("philox chain: mean ln Z", lz.mean(), "truth", prob.logz_truth, "se", se)
    assert abs(lz.mean() - prob.logz_truth) < 5 * se + 0.08, (lz.mean(), se)


def test_failed_runs_stay_failed(ctx):
    prob, kw = base_kw("rwalk-multi")
    kw["max_iter"] = 300
    try:
        a = ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, want_samples=True, **kw)
        assert (a["status"] == -1).all() and (a["niter"] == 300).all()
        b = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    assert b["nfills"] == 0
    assert_same_runs(b, a)


def test_status_one_continues_to_status_zero(ctx):
    prob, kw = base_kw("rwalk-multi")
    try:
        a = ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, max_fills=12, **kw)
        assert (a["status"] == 1).all()
        b = ctx.ns_continue(dlogz=DLOGZ, want_samples=True)
    finally:
        ctx.release_kept()
    assert (b["status"] == 0).all()
    assert_same_runs(b, full_run(ctx, "rwalk-multi"))


def plain(ctx):
    prob, kw = base_kw("rwalk-multi")
    return ctx.ns_ensemble(prob, dlogz=1.0, want_samples=True, **kw)


def test_errors_leave_the_context_usable():
    """each of these raises, leaks no option into a later call, and leaves a kept ensemble as it was"""
    from dynesty_amd import _lib
    fresh = plain(_lib.Context(0))
    c = _lib.Context(0)
    with pytest.raises(ValueError):
        c.ns_continue(dlogz=DLOGZ)  # nothing kept
    assert_same_runs(plain(c), fresh)
    prob, kw = base_kw("rwalk-multi")
    c.ns_ensemble(prob, keep=True, dlogz=DLOGZ, maxiter=150, **kw)
    c.release_kept()
    with pytest.raises(ValueError):
        c.ns_continue(dlogz=DLOGZ)  # released
    # (straight to the library: the method would not even try)
    c._kept_shape = (RUNS, NLIVE, prob.ndim, MAX_ITER)
    with pytest.raises(ValueError, match="no kept ensemble"):
        c.ns_continue(dlogz=DLOGZ, maxiter=10)
    c._kept_shape = None
    assert_same_runs(plain(c), fresh)  # (maxiter = 10 did not leak)
    ref = full_run(c, "rwalk-multi")
    c.ns_ensemble(prob, keep=True, dlogz=DLOGZ, maxiter=150, **kw)
    for key, val in ((0, 500.0), (1, 100.0), (2, 5.0), (7, 0.0)):  # update_interval, first_update (2), forced_exact
        c._check(c.lib.dh_ns_set_option(c.handle, key, val))
        with pytest.raises(ValueError, match="fixed by the ensemble's first call"):
            c.ns_continue(dlogz=DLOGZ)
    bc = np.ones(prob.ndim, dtype=np.int8)
    c._check(c.lib.dh_ns_set_boundary(c.handle, prob.ndim, bc.ctypes.data))
    with pytest.raises(ValueError, match="fixed by the ensemble's first call"):
        c.ns_continue(dlogz=DLOGZ)
    # the kept ensemble is still the one that goes on to the uninterrupted result, with nothing of the above in it
    got = c.ns_continue(dlogz=DLOGZ, want_samples=True)
    c.release_kept()
    assert_same_runs(got, ref)
    assert_same_runs(plain(c), fresh)
    c.close()


MERGED = ("logl", "logwt", "samples_n")


def test_merge_of_a_continued_ensemble(ctx):
    from dynesty_amd import backend, ensemble
    prob, kw = base_kw("rwalk-multi")
    try:
        ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, **kw)
        m = ctx.merge_kept(prob)
        want = dict(m.summary), {f: m.field(f) for f in MERGED}
    finally:
        ctx.release_kept()
    try:
        ctx.ns_ensemble(prob, keep=True, dlogz=DLOGZ, maxiter=150, **kw)
        ctx.ns_continue(dlogz=DLOGZ)
        m = ctx.merge_kept(prob)
        assert dict(m.summary) == want[0]
        for f in MERGED:
            np.testing.assert_array_equal(m.field(f), want[1][f], err_msg=f)
    finally:
        ctx.release_kept()
    # ... and through the ensemble layer: merged after the first leg, kept, continued, merged again
    prev = backend._active
    backend.set_backend(ctx)
    try:
        run_kw = {k: v for k, v in kw.items() if k not in ("runs", "nlive", "queue_size", "entropy", "max_iter")}
        m0 = ensemble.run_ensemble_merged(prob, RUNS, NLIVE, K, entropy=kw["entropy"], max_iter=MAX_ITER,
                                          merge="device", release=False, dlogz=DLOGZ, maxiter=150, **run_kw)
        assert (m0["runs"]["niter"] == 151).all()
        ctx.ns_continue(dlogz=DLOGZ)
        m = ctx.merge_kept(prob)
        assert dict(m.summary) == want[0]
        for f in MERGED:
            np.testing.assert_array_equal(m.field(f), want[1][f], err_msg=f)
    finally:
        ctx.release_kept()
        backend.set_backend(prev)
