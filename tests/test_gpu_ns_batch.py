"""Dynamic batches on the device (dh_ns_batch, csrc/ns.hip; dynesty_amd/dynamic.py).

Exactness: a strand inside dh_ns_batch against its host mirror (tests/batch_mirror.py) -- the start set, start_nc,
seed_ncall and the generator at the hand-over, then the first 150 deaths (ln L, slot, it, nc), bit for bit, for each of
the three strands: both sides
take every proposal from the same device kernels on the same streams.  Invariants on every case; 4 strands equal
2 + 2; every refused request leaves the context as a fresh one; run_dynamic end to end against the analytic ln Z.

Shapes: D = 5, nlive_new = 50, K = 16 (the last of the four seed fills takes 2 of its 16 entries), nlive_new = 64 = 4 K
(no partial fill), and the wide form at D = 40, nlive_new = 96, K = 32 with rslice."""
import math

import numpy as np
import pytest

from batch_mirror import mirror_strand

pytestmark = pytest.mark.gpu

ENT = (3, 1)


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def base5(ctx):
    """A finished 5-D run (two static runs of 100 live points, merged) and the bounds its weight function asks for."""
    from dynesty_amd import backend, problems
    from dynesty_amd.ensemble import run_ensemble_merged
    prob = problems.gauss_corr(5, 0.3, 5.0, "corr5")
    backend.set_backend(ctx)
    try:
        m = run_ensemble_merged(prob, 2, 100, 16, entropy=ENT, walks=10, dlogz=0.1, max_iter=20000)
    finally:
        backend.set_backend(None)
    return prob, m, m.weight_function()


def seeds_for(m, bounds, nlive, strands, seed=5):
    from dynesty_amd import dynamic
    rs = np.random.default_rng(seed)
    ss = [dynamic.batch_seed(m, bounds, nlive, rs) for _ in range(strands)]
    s0 = ss[0]
    assert not s0["prior"]
    return (np.stack([m["samples_u"][s["idx"]] for s in ss]), np.stack([m["logl"][s["idx"]] for s in ss]), s0["logl_min"],
            s0["logl_max"], np.array(list(s0["start"]) + [1.0]))


def check_invariants(out, logl_min, logl_max, nlive):
    assert (out["status"] == 0).all(), out["status"]
    for r in range(len(out["niter"])):
        n = int(out["niter"][r])
        d = out["dead_logl"][r, :n]
        assert (out["start_logl"][r] > logl_min).all()              # every start point above the bound
        assert n > 0 and (np.diff(d) >= 0).all() and (d > logl_min).all()
        assert d[0] == out["start_logl"][r].min()                   # the first death is the start set's worst
        if math.isfinite(logl_max):
            assert d[-1] > logl_max and (d[:-1] <= logl_max).all()  # the last dead point is the first above logl_max
        live = out["live_logl"][r]
        assert live.shape == (nlive,) and (live >= d[-1]).all()    # nlive_new final live points follow it
        assert int(out["start_nc"][r].sum()) <= int(out["seed_ncall"][r])
        # The record's calls are the seeding phase's plus every death's nc, exactly.  The loop's convention charges
        # the entries popped after a fill's last death to the NEXT death (the carry); a run that a stop rule ends --
        # every run here: status 0 by dlogz or logl_max -- is charged up to the entry that replaced its last dead
        # point and no further, so no carry is outstanding when it ends.
        assert int(out["ncall"][r]) == int(out["seed_ncall"][r]) + int(out["dead_nc"][r, :n].sum())
        assert (out["dead_it"][r, :n] >= 0).all() and (out["dead_it"][r, :n] <= n).all()
        assert (out["dead_id"][r, :n] >= 0).all() and (out["dead_id"][r, :n] < nlive).all()


CASES = {"rwalk50": dict(sample="rwalk", bound="multi", nlive=50, kw=dict(walks=10), mirror=dict(enlarge=1.25, bootstrap=0)),
         "unif50": dict(sample="unif", bound="single", nlive=50, kw={}, mirror=dict(enlarge=1.0, bootstrap=5)),
         "rwalk64": dict(sample="rwalk", bound="multi", nlive=64, kw=dict(walks=10), mirror=dict(enlarge=1.25, bootstrap=0))}


@pytest.mark.parametrize("name", list(CASES))
def test_strand_equals_its_host_mirror_bit_for_bit(ctx, base5, name):
    prob, m, bounds = base5
    c = CASES[name]
    K, N, ND = 16, c["nlive"], 150
    su, sl, lmin, lmax, start = seeds_for(m, bounds, N, 3)
    ent = ENT + (1,)
    out = ctx.ns_batch(prob, su, sl, lmin, start, K, entropy=ent, max_iter=20000, sample=c["sample"], bound=c["bound"],
                       rebuild_every=1, dlogz=0.01, **c["kw"])
    check_invariants(out, lmin, math.inf, N)
    assert (out["niter"] >= ND).all()
    if c["sample"] == "rwalk":
        assert (out["seed_ncall"] == -(-N // K) * K * 10).all()  # every entry of every seed fill is charged
    for r in range(3):
        mi = mirror_strand(ctx, prob, su[r], sl[r], lmin, start, K, c["kw"].get("walks", 1), c["bound"], ent, r, 0.01, ND,
                           sample=c["sample"], **c["mirror"])
        np.testing.assert_array_equal(out["start_u"][r], mi["start_u"])
        np.testing.assert_array_equal(out["start_logl"][r], mi["start_logl"])
        np.testing.assert_array_equal(out["start_nc"][r], mi["start_nc"])
        assert int(out["seed_ncall"][r]) == mi["seed_ncall"]
        np.testing.assert_array_equal(out["seed_rng"][r], mi["seed_rng"])
        np.testing.assert_array_equal(out["dead_logl"][r, :ND], np.array(mi["dead_logl"][:ND]))
        np.testing.assert_array_equal(out["dead_id"][r, :ND], np.array(mi["dead_slot"][:ND]))
        np.testing.assert_array_equal(out["dead_it"][r, :ND], np.array(mi["dead_it"][:ND]))
        np.testing.assert_array_equal(out["dead_nc"][r, :ND], np.array(mi["dead_nc"][:ND]))


@pytest.mark.parametrize("name", list(CASES))
def test_invariants_with_a_finite_logl_max(ctx, base5, name):
    prob, m, bounds = base5
    c = CASES[name]
    su, sl, lmin, lmax, start = seeds_for(m, bounds, c["nlive"], 3)
    out = ctx.ns_batch(prob, su, sl, lmin, start, 16, logl_max=lmax, entropy=ENT + (2,), max_iter=20000,
                       sample=c["sample"], bound=c["bound"], **c["kw"])
    check_invariants(out, lmin, lmax, c["nlive"])
    assert (out["nbound"] >= 2).all()  # the seeds' bound, and at least one on the strand's own points


def test_wide_strands_keep_the_invariants(ctx):
    """D = 40 (the wave-per-walker kernels and the wide bound), nlive_new = 96, K = 32, rslice."""
    from dynesty_amd import backend, problems
    from dynesty_amd.ensemble import run_ensemble_merged
    prob = problems.gauss_corr(40, 0.3, 5.0, "corr40")
    backend.set_backend(ctx)
    try:
        m = run_ensemble_merged(prob, 1, 96, 32, entropy=(4, 0), sample="rslice", slices=5, dlogz=0.5, max_iter=40000)
    finally:
        backend.set_backend(None)
    bounds = m.weight_function()
    su, sl, lmin, lmax, start = seeds_for(m, bounds, 96, 2)
    out = ctx.ns_batch(prob, su, sl, lmin, start, 32, logl_max=lmax, entropy=(4, 0, 1), max_iter=40000, sample="rslice",
                       slices=5, bound="multi")
    check_invariants(out, lmin, lmax, 96)


def test_four_strands_equal_two_plus_two(ctx, base5):
    prob, m, bounds = base5
    su, sl, lmin, lmax, start = seeds_for(m, bounds, 50, 4)
    kw = dict(logl_max=lmax, entropy=ENT + (3,), max_iter=20000, walks=10)
    whole = ctx.ns_batch(prob, su, sl, lmin, start, 16, **kw)
    parts = [ctx.ns_batch(prob, su[:2], sl[:2], lmin, start, 16, **kw),
             ctx.ns_batch(prob, su[2:], sl[2:], lmin, start, 16, first_run=2, **kw)]
    check_invariants(whole, lmin, lmax, 50)
    for k in ("logz", "logzerr", "niter", "ncall", "h", "nbound", "status", "seed_ncall", "seed_rng", "start_u",
              "start_logl", "start_nc", "live_logl", "live_u", "live_it"):
        np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in parts]), err_msg=k)
    for r in range(4):
        n, p = int(whole["niter"][r]), parts[r // 2]
        for k in ("dead_logl", "dead_u", "dead_id", "dead_it", "dead_nc"):
            np.testing.assert_array_equal(whole[k][r, :n], p[k][r % 2, :n], err_msg=k)


def test_refused_requests_leave_the_context_usable(ctx, base5):
    from dynesty_amd import _lib
    prob, m, bounds = base5
    su, sl, lmin, lmax, start = seeds_for(m, bounds, 50, 2)
    ok = dict(logl_max=lmax, entropy=ENT + (4,), max_iter=20000, walks=10)

    def refused(su_=su, sl_=sl, lmin_=lmin, start_=start, **kw):
        args = dict(ok)
        args.update(kw)
        with pytest.raises(_lib.DynHipError, match="ns_batch"):
            ctx.ns_batch(prob, su_, sl_, lmin_, start_, 16, **args)
    refused(rng="philox")                                     # the Philox samplers: rwalk ...
    refused(rng="philox", sample="rslice")
    refused(rng="philox", sample="slice")
    refused(rng="philox", sample="unif")
    refused(sample="unif", bound="balls")                     # the friends bounds
    refused(sample="unif", bound="cubes")
    refused(keep=True)                                        # dh_ns_keep
    refused(lmin_=-math.inf)                                  # a non-finite logl_min
    refused(lmin_=math.nan)
    low = sl.copy()
    low[1, 7] = lmin                                          # a seed AT logl_min
    refused(sl_=low)
    refused(su_=su[:, :1], sl_=sl[:, :1])                     # nlive_new < 2 ...
    refused(su_=su[:, :3], sl_=sl[:, :3])                     # ... and below the loop's own four live points
    big = 65536                                               # nlive_new above the loop's limit (16-bit slots)
    refused(su_=np.full((1, big, 5), 0.5), sl_=np.full((1, big), lmin + 1.0), max_iter=16)
    refused(logl_max=lmin)                                    # logl_max <= logl_min
    refused(logl_max=lmin - 1.0)
    bad = start.copy()
    bad[5] = 0.0
    refused(start_=bad)                                       # a scale of 0
    # the next ns_ensemble call gives what it gives on a fresh context (nothing one-shot is left armed: keep, options)
    args = dict(walks=10, dlogz=0.1, entropy=(9, 9), max_iter=20000, want_samples=True)
    got = ctx.ns_ensemble(prob, 2, 60, 16, **args)
    fresh = _lib.Context(0).ns_ensemble(prob, 2, 60, 16, **args)
    for k in ("logz", "logzerr", "niter", "ncall", "nbound", "status", "live_logl", "live_u"):
        np.testing.assert_array_equal(got[k], fresh[k], err_msg=k)
    # ... and a batch still runs
    out = ctx.ns_batch(prob, su, sl, lmin, start, 16, **ok)
    check_invariants(out, lmin, lmax, 50)


def test_run_dynamic_end_to_end_against_the_analytic_evidence(ctx):
    """A 3-D unit Gaussian exp(-|x|^2 / 2) under a uniform prior on [-10, 10]^3: ln Z = ln((2 pi)^1.5 / 20^3).  8 base
    runs of 100 live points, two batches of 8 strands of 100, rwalk, entropy (21, g) for 16 groups g fixed in advance.
    Gate: |mean ln Z - truth| <= max(0.05, 3 se), se the empirical error of the mean over the groups (the form and the
    floor of the resident loop's own ln Z gates)."""
    from dynesty_amd import backend, dynamic, problems
    truth = 1.5 * math.log(2.0 * math.pi) - 3.0 * math.log(20.0)
    prob = problems.Problem(3, problems.LIKE_GAUSS_IID, [0.0], problems.PRIOR_AFFINE, [10.0, 0.0], logz_truth=truth,
                            name="gauss3_unnormalised")
    R, N, S, NB = 8, 100, 8, 100
    lz = []
    backend.set_backend(ctx)
    try:
        for g in range(16):
            m, log = dynamic.run_dynamic(prob, R, N, S, NB, 2, pfrac=0.8, entropy=(21, g), queue_size=25,
                                         stop_kwargs=dict(target_n_effective=10 ** 9))
            assert len(log) == 3 and not log[-1]["stop"]
            base = log[0]["run"]
            lz.append(float(m["logz"][-1]))
            # between a batch's bounds all of its strands are active: the live count there exceeds the base's by
            # strands x nlive_batch per batch whose range holds the point
            from_base = np.flatnonzero(m["samples_batch"] == 0)
            assert len(from_base) == len(base["logl"])
            np.testing.assert_array_equal(m["logl"][from_base], base["logl"])
            extra = np.zeros(len(from_base), dtype=np.int64)
            tail = np.zeros(len(from_base), dtype=np.int64)
            for e in log[1:]:
                lo, hi = e["bounds"]
                extra += S * NB * ((base["logl"] > lo) & (base["logl"] <= hi))
                tail += S * NB * (base["logl"] > hi)  # (above hi a strand goes on to its first dead point beyond it,
                #                                        then its live points leave one by one)
            more = m["samples_n"][from_base] - np.asarray(base["samples_n"])
            exact = tail == 0
            assert (extra[exact] >= S * NB).any()
            np.testing.assert_array_equal(more[exact], extra[exact])
            assert (more >= extra).all() and (more <= extra + tail).all()
            # the batches bought something: effective sample size up, ln Z error down
            assert m._err_summary()[1] > base._err_summary()[1]
            assert m.logz_error(128, seed=g)[1] < base.logz_error(128, seed=g)[1]
    finally:
        backend.set_backend(None)
    lz = np.array(lz)
    mean, se = lz.mean(), lz.std(ddof=1) / math.sqrt(len(lz))
    print(f"run_dynamic: mean ln Z {mean:.4f} truth {truth:.4f} diff {mean - truth:+.4f} se {se:.4f}")
    assert abs(mean - truth) <= max(0.05, 3.0 * se), (mean, truth, se)
