"""dh_ns_keep / dh_merge_kept: an ensemble left on the device and merged there equals the host combiner's merge of
the same call's downloaded arrays; the keep switch changes nothing else."""
import numpy as np
import pytest

import inputs
import merge_hp_ref as hp
from test_gpu_merge import check_floats

pytestmark = pytest.mark.gpu

KW = dict(walks=23, bound="single", entropy=[5, 9], dlogz=0.1, max_iter=8000)


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def kept(ctx):
    """4 C1 runs (nlive 100, K 16), kept and downloaded; merged on the device at once (the next ensemble call of the
    module would otherwise replace nothing -- only a later keep does -- but the merge belongs to this call)."""
    prob = inputs.problem("C1")
    r = ctx.ns_ensemble(prob, 4, 100, 16, want_samples=True, keep=True, **KW)
    assert (r["status"] == 0).all()
    d = ctx.merge_kept(prob)
    m = d.to_merged_run()
    m["weights"] = d.importance_weights()
    return prob, r, d, m


def test_merge_kept_equals_host_merge_of_the_download(ctx, kept):
    from dynesty_amd import ensemble
    prob, r, d, m = kept
    host = ensemble.merge_static_runs(r["dead_logl"], r["niter"], r["live_logl"], r["dead_u"], r["live_u"],
                                      prior_transform=lambda u: ctx.problem_eval(prob, u)[0], dead_id=r["dead_id"],
                                      dead_it=r["dead_it"], dead_nc=r["dead_nc"], live_it=r["live_it"])
    assert m.niter == host.niter
    for k in ("logl", "samples_n", "samples_run", "samples_seq", "samples_id", "samples_it", "ncall", "samples_u",
              "samples"):
        np.testing.assert_array_equal(m[k], host[k], err_msg=k)
    ref = hp.merge_hp([r["dead_logl"][i] for i in range(4)], r["niter"], r["live_logl"])
    check_floats(m, ref, "kept")
    assert d.summary["ncall"] == int(host.ncall.sum())


def test_keep_changes_nothing_else(ctx, kept):
    prob, r, _, _ = kept
    r2 = ctx.ns_ensemble(prob, 4, 100, 16, want_samples=True, **KW)
    for k in ("logz", "logzerr", "niter", "ncall", "h", "nbound", "status", "eff", "live_logl", "live_u", "live_it"):
        np.testing.assert_array_equal(r[k], r2[k], err_msg=k)
    for i, n in enumerate(r["niter"]):
        for k in ("dead_logl", "dead_u", "dead_id", "dead_it", "dead_nc"):
            np.testing.assert_array_equal(r[k][i, :n], r2[k][i, :n], err_msg=k)


def test_keep_without_samples_still_merges(ctx, kept):
    prob, r, d, m = kept
    r3 = ctx.ns_ensemble(prob, 4, 100, 16, want_samples=False, keep=True, **KW)
    assert not any(k in r3 for k in ("dead_logl", "dead_u", "live_u", "dead_id"))
    np.testing.assert_array_equal(r3["logz"], r["logz"])
    d3 = ctx.merge_kept(prob)
    assert d3.summary == d.summary
    np.testing.assert_array_equal(d3.field("samples"), m.samples)
    with pytest.raises(ValueError):  # the earlier merged run was replaced
        d.field("logl")
    with pytest.raises(ValueError, match="kept ensemble"):  # another problem
        ctx.merge_kept(inputs.problem("G5"))
    ctx.release_kept()
    with pytest.raises(ValueError, match="kept"):
        ctx.merge_kept(prob)


def test_run_ensemble_merged_device_against_host(ctx):
    from dynesty_amd import backend, ensemble
    prob = inputs.problem("C1")
    backend.set_backend(ctx)
    try:
        kw = dict(nlive=100, queue_size=16, entropy=[5, 9], walks=23, bound="single", dlogz=0.1)
        h = ensemble.run_ensemble_merged(prob, 4, merge='host', **kw)
        d = ensemble.run_ensemble_merged(prob, 4, merge='device', **kw)
    finally:
        backend.set_backend(None)
    np.testing.assert_array_equal(d["runs"]["logz"], h["runs"]["logz"])
    assert "dead_u" not in d["runs"]
    ref = hp.merge_hp([h["runs"]["dead_logl"][i] for i in range(4)], h["runs"]["niter"], h["runs"]["live_logl"])
    b = hp.bounds(ref)
    assert d.summary["niter"] == h.niter
    # both within their bounds of the long-double value (the host's: the project's tolerances)
    assert abs(d.summary["logz"] - float(ref["logz"][-1])) <= b["logz"][-1]
    assert abs(d.summary["logzerr"] - float(ref["logzerr"][-1])) <= b["logzerr"][-1]
    assert abs(d.summary["h"] - float(ref["information"][-1])) <= b["information"][-1]
    assert abs(d.summary["logz"] - h.logz[-1]) <= b["logz"][-1] + 1e-10
    assert abs(d.summary["logzerr"] - h.logzerr[-1]) <= b["logzerr"][-1] + 1e-7 * h.logzerr[-1] + 1e-10
    assert abs(d.summary["h"] - h.information[-1]) <= b["information"][-1] + 1e-9
