"""Ensemble combiner vs the REAL reference: `ensemble.merge_logz` must give the
same ln Z and error as dynesty.utils.merge_runs (utils.py:1817-1900) for static
runs of equal nlive.  The reference's runs and merged results are stored in
tests/golden/merge.npz (tools/make_golden.py merge)."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge.npz")


@pytest.fixture(scope="module")
def golden_merge():
    return np.load(GOLDEN)


def test_merge_logz_matches_reference_merge_runs(golden_merge):
    from dynesty_amd import ensemble
    g = golden_merge
    lz, err = ensemble.merge_logz(g["logz/dead"], list(g["logz/nit"]), g["logz/live"])
    np.testing.assert_allclose(lz, g["logz/logz"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(err, g["logz/logzerr"], rtol=1e-9)


def test_merge_static_runs_matches_reference_fields(golden_merge):
    """Every per-point field of the merged run (order, live counts, volumes,
    weights, cumulative ln Z / information / error, samples) equals the
    reference's utils.merge_runs on static runs."""
    import inputs
    from dynesty_amd import ensemble
    g = golden_merge
    prob = inputs.problem("C1")
    dead_i = g["static/dead_i"]

    def ptform(u):
        return np.array([prob.prior_transform(x) for x in u])
    m = ensemble.merge_static_runs(g["static/dead_l"], list(g["static/nit"]), g["static/live_l"], g["static/dead_u"],
                                   g["static/live_u"], prior_transform=ptform, dead_id=dead_i[0], dead_it=dead_i[1],
                                   dead_nc=dead_i[2], live_it=g["static/live_it"])

    def ref(k):
        return g["ref/" + k]
    # the per-point bookkeeping _merge_two copies through (utils.py:2154-2156, 2196-2207)
    np.testing.assert_array_equal(m.samples_id, ref("samples_id"))
    np.testing.assert_array_equal(m.samples_it, ref("samples_it"))
    np.testing.assert_array_equal(m.ncall, ref("ncall"))
    assert m.niter == ref("niter")
    np.testing.assert_array_equal(m.logl, ref("logl"))
    np.testing.assert_array_equal(m.samples_n, ref("samples_n"))
    np.testing.assert_array_equal(m.samples_u, ref("samples_u"))
    np.testing.assert_allclose(m.samples, ref("samples"), rtol=0, atol=1e-14)
    np.testing.assert_allclose(m.logvol, ref("logvol"), rtol=0, atol=1e-11)
    np.testing.assert_allclose(m.logwt, ref("logwt"), rtol=0, atol=1e-10)
    np.testing.assert_allclose(m.logz, ref("logz"), rtol=0, atol=1e-10)
    np.testing.assert_allclose(m.information, ref("information"), rtol=0, atol=1e-9)
    np.testing.assert_allclose(m.logzerr, ref("logzerr"), rtol=1e-7, atol=1e-10)
    w = m.importance_weights()
    np.testing.assert_allclose(w, ref("importance_weights"), rtol=1e-9, atol=1e-300)
    assert abs(m.eff - ref("eff")) < 1e-9
