"""dynesty_amd.dynamic on the host, against the reference's own dynamic run (tests/golden/batch_combine.npz, written by
tools/make_golden.py gen_batch: a 3-D Gaussian, nlive_init = nlive_batch = 50, three batches, with spies on
_configure_batch_sampler and combine_runs).  batch_seed must give the reference's weighted choice, adjusted bounds and
vol_idx exactly; merge_batch, folded over the three batches, the reference's order, n, ids and batch indices exactly
and its volumes and integrals to the tolerances tests/test_merge_cpu.py holds merge_static_runs to against
utils.merge_runs (logvol 1e-11, logwt / logz 1e-10, information 1e-9, logzerr rtol 1e-7 + 1e-10)."""
import os

import numpy as np
import pytest

from dynesty_amd import dynamic
from dynesty_amd.ensemble import MergedRun

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_combine.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


def generator(words):
    """A numpy Generator in the stored state: [state hi, lo, inc hi, lo, has_uint32, uinteger]."""
    w = [int(x) for x in words]
    bg = np.random.PCG64()
    bg.state = dict(bit_generator="PCG64", state=dict(state=(w[0] << 64) | w[1], inc=(w[2] << 64) | w[3]),
                    has_uint32=w[4], uinteger=w[5])
    return np.random.Generator(bg)


def saved_run(g, prefix):
    f = {k: g[f"{prefix}/{k}"] for k in ("logl", "logvol", "n", "id", "it", "nc", "u", "logz", "logzvar", "h", "batch")}
    return MergedRun(niter=len(f["logl"]), logl=f["logl"], logvol=f["logvol"], logz=f["logz"], information=f["h"],
                     logzerr=np.sqrt(f["logzvar"]), samples_n=f["n"], samples_id=f["id"], samples_it=f["it"],
                     ncall=f["nc"], samples_u=f["u"], samples_batch=f["batch"])


def test_golden_has_three_batches_inside_the_run(g):
    assert int(g["nbatch"]) == 3
    for b in range(3):
        assert np.isfinite(g[f"{b}/bounds_out"]).all() and len(g[f"{b}/subset"]) == 50


@pytest.mark.parametrize("b", [0, 1, 2])
def test_batch_seed_gives_the_reference_choice(g, b):
    base = saved_run(g, f"{b}/base")
    s = dynamic.batch_seed(base, tuple(g[f"{b}/bounds_in"]), 50, generator(g[f"{b}/rstate"]))
    assert not s["prior"]
    np.testing.assert_array_equal(s["idx"], g[f"{b}/subset"])
    assert (s["logl_min"], s["logl_max"]) == tuple(g[f"{b}/bounds_out"])
    assert s["vol_idx"] == int(g[f"{b}/vol_idx"])
    i = s["vol_idx"] - 1
    want = (base.logvol[i], base.logz[i], base.information[i], g[f"{b}/base/logzvar"][i], base.logl[i])
    np.testing.assert_allclose(s["start"], want, rtol=1e-14, atol=0)
    assert (base.logl[s["idx"]] > s["logl_min"]).all()


def test_batch_seed_constructed_cases(g):
    base = saved_run(g, "0/base")
    # fewer than nlive_new points above the bound: the boundary moves down to the ln L just below the 50 highest
    s = dynamic.batch_seed(base, tuple(g["sel/0/bounds_in"]), 50, generator(g["sel/0/rstate"]))
    assert (base.logl > g["sel/0/bounds_in"][0]).sum() < 50 and not s["prior"]
    np.testing.assert_array_equal(s["idx"], g["sel/0/subset"])
    assert (s["logl_min"], s["logl_max"]) == tuple(g["sel/0/bounds_out"]) and s["logl_min"] < g["sel/0/bounds_in"][0]
    assert s["vol_idx"] == int(g["sel/0/vol_idx"])
    # a bound below every point: from the prior, no seeds, nothing drawn
    rs = generator(g["sel/1/rstate"])
    s = dynamic.batch_seed(base, tuple(g["sel/1/bounds_in"]), 50, rs)
    assert s["prior"] and s["idx"] is None and s["start"] is None
    assert (s["logl_min"], s["logl_max"]) == tuple(g["sel/1/bounds_out"]) and s["vol_idx"] == int(g["sel/1/vol_idx"])
    assert rs.bit_generator.state == generator(g["sel/1/rstate"]).bit_generator.state
    # logl_bounds=None: (-inf, ln L at the last index with logvol < logvol[-1] + ln nlive_new)
    s = dynamic.batch_seed(base, None, 50, generator(g["sel/2/rstate"]))
    assert s["prior"] and s["idx"] is None
    assert (s["logl_min"], s["logl_max"]) == tuple(g["sel/2/bounds_out"]) and s["vol_idx"] == int(g["sel/2/vol_idx"]) == 0


def test_batch_seed_errors(g):
    base = saved_run(g, "0/base")
    rs = np.random.default_rng(1)
    with pytest.raises(RuntimeError, match="Could not find live points"):
        dynamic.batch_seed(base, (float(base.logl[-1]), np.inf), 50, rs)  # no point above logl_min
    # fewer than nlive_new points of positive weight: the weights of all but the 10 highest-volume points underflow
    lv = base.logvol.copy()
    lv[10:] -= 2000.0
    far = MergedRun(base, logvol=lv)
    with pytest.raises(ValueError, match="positive weight"):
        dynamic.batch_seed(far, (float(base.logl[0]), np.inf), 50, rs)
    short = MergedRun({k: (v[:30] if isinstance(v, np.ndarray) else v) for k, v in base.items()})
    with pytest.raises(ValueError, match="positive weight"):  # fewer than nlive_new points in the whole run
        dynamic.batch_seed(short, (float(base.logl[3]), np.inf), 50, rs)


def test_merge_batch_folds_the_three_batches_like_combine_runs(g):
    m = saved_run(g, "0/base")
    for b in range(3):
        strand = {k: g[f"{b}/new/{k}"] for k in ("logl", "n", "id", "it", "nc", "u")}
        lmin, lmax = g[f"{b}/new_bounds"]
        m = dynamic.merge_batch(m, strand, lmin, lmax)

        def ref(k):
            return g[f"{b}/after/{k}"]
        np.testing.assert_array_equal(m.logl, ref("logl"))
        np.testing.assert_array_equal(m.samples_n, ref("n"))
        np.testing.assert_array_equal(m.samples_id, ref("id"))
        np.testing.assert_array_equal(m.samples_batch, ref("batch"))
        np.testing.assert_array_equal(m.samples_it, ref("it"))
        np.testing.assert_array_equal(m.ncall, ref("nc"))
        np.testing.assert_array_equal(m.samples_u, ref("u"))
        np.testing.assert_allclose(m.logvol, ref("logvol"), rtol=0, atol=1e-11)
        np.testing.assert_allclose(m.logwt, ref("logwt"), rtol=0, atol=1e-10)
        np.testing.assert_allclose(m.logz, ref("logz"), rtol=0, atol=1e-10)
        np.testing.assert_allclose(m.information, ref("h"), rtol=0, atol=1e-9)
        np.testing.assert_allclose(m.logzerr, np.sqrt(ref("logzvar")), rtol=1e-7, atol=1e-10)
        assert m.batch_nlive == ref("batch_nlive").tolist()
        np.testing.assert_array_equal(np.array(m.batch_bounds), ref("batch_bounds"))
        assert m.niter == len(m.logl) and m.eff == pytest.approx(100. * len(m.logl) / ref("nc").sum())
    assert (np.diff(m.logvol) < 0).all() and set(np.unique(m.samples_batch)) == {0, 1, 2, 3}


def test_merge_batch_plateau_volumes_and_heads():
    """The volume pass's plateau rule and the walk's heads on a run small enough to follow by hand: the saved point
    comes first on a tie; below logl_min only the saved run counts; an exhausted side counts 0."""
    base = MergedRun(logl=np.array([1., 2., 2., 3.]), samples_n=np.array([2, 2, 2, 1]), samples_id=np.array([0, 1, 0, 1]),
                     logvol=np.zeros(4), logz=np.zeros(4), information=np.zeros(4), logzerr=np.zeros(4))
    strand = dict(logl=np.array([2., 2.5, 4.]), n=np.array([2, 2, 1]), id=np.array([0, 1, 1]))
    m = dynamic.merge_batch(base, strand, 1.5, np.inf)
    np.testing.assert_array_equal(m.logl, [1., 2., 2., 2., 2.5, 3., 4.])
    np.testing.assert_array_equal(m.samples_batch, [0, 0, 0, 1, 0 + 1, 0, 1])
    np.testing.assert_array_equal(m.samples_id, [0, 1, 0, 2, 3, 1, 3])
    # heads: (1 | 2) below the bound -> 2; (2 | 2) -> 4; (2 | 2) -> 4; (3 | 2) -> 1 + 2; (3 | 2.5) -> 3; (3 | 4) -> 2;
    # saved exhausted -> 0 + 1
    np.testing.assert_array_equal(m.samples_n, [2, 4, 4, 3, 3, 2, 1])
    lv = [np.log(2. / 3.)]                      # ordinary step at n = 2
    x0 = np.exp(lv[0])                          # a plateau of three at n = 4: linear steps of X / 5
    lv += [np.log(x0 * (1 - k / 5.)) for k in (1, 2, 3)]
    lv += [lv[-1] + np.log(3. / 4.), lv[-1] + np.log(3. / 4.) + np.log(2. / 3.)]
    lv += [lv[-1] + np.log(1. / 2.)]
    np.testing.assert_allclose(m.logvol, lv, rtol=0, atol=1e-14)
    with pytest.raises(ValueError, match="No new samples"):
        dynamic.merge_batch(base, dict(logl=np.zeros(0), n=np.zeros(0), id=np.zeros(0)), 1.5, np.inf)


def test_merged_batches_survive_a_round_trip_through_arrays_and_refuse_the_strand_bootstrap(g):
    """A run rebuilt from saved arrays carries batch_nlive / batch_bounds as NumPy arrays: folding goes on from them.
    The strand bootstrap reads strands off a live count that only falls, so on a run with batches it raises instead of
    resampling wrong strands; the volume realizations are a function of samples_n alone and work."""
    m = saved_run(g, "0/base")
    strand = {k: g["0/new/" + k] for k in ("logl", "n", "id", "it", "nc", "u")}
    m = dynamic.merge_batch(m, strand, *g["0/new_bounds"])
    again = MergedRun({k: (np.array(v) if isinstance(v, list) else v) for k, v in m.items()})
    assert isinstance(again["batch_nlive"], np.ndarray) and again["batch_bounds"].shape == (2, 2)
    strand = {k: g["1/new/" + k] for k in ("logl", "n", "id", "it", "nc", "u")}
    a, b = dynamic.merge_batch(m, strand, *g["1/new_bounds"]), dynamic.merge_batch(again, strand, *g["1/new_bounds"])
    np.testing.assert_array_equal(a.samples_n, b.samples_n)
    np.testing.assert_array_equal(a.samples_batch, g["1/after/batch"])
    assert a.batch_nlive == b.batch_nlive == [50, 50, 50] and a.batch_bounds == b.batch_bounds
    a["samples_run"] = np.zeros(len(a.logl), dtype=np.int64)
    with pytest.raises(ValueError, match="dynamic batches"):
        a.bootstrap_realizations(4, seed=1)
    with pytest.raises(ValueError, match="dynamic batches"):
        a.stopping_function(pfrac=0.0, n_mc=32, error="resample")
    lz = a.logz_realizations(8, seed=1)["logz"]
    assert np.isfinite(lz).all() and abs(lz.mean() - a.logz[-1]) < 1.0
