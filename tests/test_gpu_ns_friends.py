"""The device-resident loop with RadFriends / SupFriends bounds and the uniform sampler (dh_ns_ensemble, bound code
2 / 3) against its host mirror (tests/resident_friends_mirror.py), death for death: the batched friends update, the
bootstrap replicas from the loop's streams, the enlargement and the per-run sampler on each run's live points of the
fill, around the library's single-call entry points.  Tolerances as tests/test_gpu_resident_mirror.py: slots, call,
iteration and bound-update counts exactly; ln L, u and ln Z to 1e-6."""
import numpy as np
import pytest

from resident_friends_mirror import mirror_friends_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def problem(name):
    from dynesty_amd import problems
    return problems.eggbox(2) if name == "egg" else problems.gauss_corr(4, 0.3, 5.0, "corr4")


def check_run(r, run, m):
    assert m["done"]
    n = int(r["niter"][run])
    assert m["niter"] == n, (m["niter"], n)
    np.testing.assert_array_equal(r["dead_id"][run, :n], np.array(m["dead_slot"]))
    np.testing.assert_allclose(r["dead_logl"][run, :n], np.array(m["dead_logl"]), rtol=1e-6, atol=0)
    np.testing.assert_allclose(r["live_logl"][run], m["live_logl"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(r["live_u"][run], m["live_u"], rtol=0, atol=1e-6)
    assert int(r["ncall"][run]) == m["ncall"]
    assert int(r["nbound"][run]) == m["nbound"], (r["nbound"][run], m["nbound"])
    assert abs(r["logz"][run] - m["logz"]) < 1e-6


# kind, problem, nlive, K, rebuild_every, (enlarge, bootstrap)
CASES = [("balls", "egg", 120, 8, 1, (1.0, 5)), ("cubes", "egg", 100, 1, 1, (1.0, 5)),
         ("balls", "corr4", 80, 16, 0, (1.0, 5)), ("cubes", "corr4", 150, 8, 3, (1.3, 0)),
         ("balls", "egg", 200, 16, 3, (1.3, 0)), ("cubes", "egg", 80, 8, 0, (1.0, 5)),
         ("balls", "corr4", 100, 1, 1, (1.3, 0))]


@pytest.mark.parametrize("kind,pname,nlive,K,every,eb", CASES)
def test_friends_loop_equals_its_host_mirror(ctx, kind, pname, nlive, K, every, eb):
    prob = problem(pname)
    enlarge, bootstrap = eb
    dlogz, ent = 0.5, [9, K, nlive]
    r = ctx.ns_ensemble(prob, 2, nlive, K, bound=kind, sample="unif", dlogz=dlogz, entropy=ent, rebuild_every=every,
                        enlarge=enlarge, bootstrap=bootstrap, want_samples=True, want_dead_logl=True, max_iter=20000)
    assert (r["status"] == 0).all(), r["status"]
    for run in (0, 1):
        m = mirror_friends_run(ctx, prob, nlive, K, kind, ent, run, dlogz, enlarge=enlarge, bootstrap=bootstrap)
        check_run(r, run, m)
        assert m["nbound"] >= 2
        if pname == "egg":
            assert max(m["nclusters"]) > 1  # the modes became clusters of the friends update


# (configurations of the mirror cases above: at 80-120 live points in the eggbox an occasional run's bootstrap radius
# takes the shapes far past the unit cube and the uniform sampler then needs a great many calls per point, as the
# reference's does -- these runs are known to stay clear of that)
@pytest.mark.parametrize("kind,pname,nlive,K,eb", [("balls", "egg", 120, 8, (1.0, 5)), ("cubes", "corr4", 150, 8, (1.3, 0))])
def test_friends_ensemble_equals_its_shards(ctx, kind, pname, nlive, K, eb):
    """Run r's result depends on its global index alone (first_run sharding), bit for bit."""
    prob = problem(pname)
    kw = dict(bound=kind, sample="unif", dlogz=0.5, entropy=[9, K, nlive], want_dead_logl=True, max_iter=20000,
              enlarge=eb[0], bootstrap=eb[1])
    whole = ctx.ns_ensemble(prob, 2, nlive, K, **kw)
    assert (whole["status"] == 0).all()
    for first, cnt in ((0, 1), (1, 1)):
        part = ctx.ns_ensemble(prob, cnt, nlive, K, first_run=first, **kw)
        for key in ("logz", "logzerr", "niter", "ncall", "nbound", "h"):
            np.testing.assert_array_equal(part[key], whole[key][first:first + cnt], err_msg=key)
        for j in range(cnt):
            n = int(part["niter"][j])
            np.testing.assert_array_equal(part["dead_logl"][j, :n], whole["dead_logl"][first + j, :n])


def test_friends_rebuild_sync_and_options_complete(ctx):
    """rebuild_sync=True (every bound-mode run rebuilds whenever one is due) and the loop's other options with a
    friends bound: every run ends with status 0 and a sane ln Z."""
    prob = problem("egg")
    r = ctx.ns_ensemble(prob, 8, 500, 64, bound="cubes", sample="unif", dlogz=0.5, entropy=[3, 3], rebuild_sync=True)
    assert (r["status"] == 0).all()
    assert np.all(np.abs(r["logz"] - 235.856) < 1.0), r["logz"]
    r = ctx.ns_ensemble(prob, 4, 500, 64, bound="balls", sample="unif", dlogz=0.5, entropy=[3, 4],
                        update_interval=0.5, first_update=dict(min_ncall=1000, min_eff=20.0), maxcall=20000,
                        periodic=[0], reflective=[1])
    assert (r["status"] == 0).all()
    assert (r["nbound"] > 0).all()
