"""The long-double restatement of the combiner (tests/merge_hp_ref.py) against the real reference's merged run
(tests/golden/merge.npz, merge_device.npz) and the host combiner against it on the synthetic cases."""
import os

import numpy as np
import pytest

import merge_cases
import merge_hp_ref as hp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "merge.npz")), np.load(os.path.join(GOLD, "merge_device.npz"))


@pytest.fixture(scope="module")
def gold_hp(gold):
    g, _ = gold
    return hp.merge_hp(g["static/dead_l"], g["static/nit"], g["static/live_l"], samples=g["ref/samples"])


def test_hp_matches_reference_fields(gold, gold_hp):
    """The tolerances of tests/test_merge_cpu.py, nothing excluded."""
    g, _ = gold
    m = gold_hp
    f = lambda k: np.asarray(m[k], dtype=np.float64)  # noqa: E731
    np.testing.assert_array_equal(f("logl"), g["ref/logl"])
    np.testing.assert_array_equal(m["samples_n"], g["ref/samples_n"])
    np.testing.assert_allclose(f("logvol"), g["ref/logvol"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(f("logwt"), g["ref/logwt"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(f("logz"), g["ref/logz"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(f("information"), g["ref/information"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(f("logzerr"), g["ref/logzerr"], rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(f("weights"), g["ref/importance_weights"], rtol=1e-9, atol=1e-300)


def test_hp_logz_set(gold):
    g, _ = gold
    m = hp.merge_hp(g["logz/dead"], g["logz/nit"], g["logz/live"])
    np.testing.assert_allclose(float(m["logz"][-1]), g["logz/logz"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(float(m["logzerr"][-1]), g["logz/logzerr"], rtol=1e-9)


def test_hp_moments_and_resampling_match_reference(gold, gold_hp):
    g, d = gold
    np.testing.assert_allclose(np.asarray(gold_hp["mean"], dtype=np.float64), d["mean"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(np.asarray(gold_hp["cov"], dtype=np.float64), d["cov"], rtol=0, atol=1e-13)
    for s in range(4):
        got = hp.resample_hp(g["ref/samples"], g["ref/importance_weights"], np.random.default_rng(s))
        np.testing.assert_array_equal(got, d[f"resample/{s}"])
        assert float(d[f"u0/{s}"]) == np.random.default_rng(s).random()


def test_permutation_of_indices_is_permutation_of_rows(gold):
    """Generator.permutation draws the same for an index vector as for the row array: shuffling the indices before
    the gather (DeviceMergedRun.resample_equal) equals the reference's shuffle of the gathered rows."""
    g, d = gold
    x = g["ref/samples"]
    for s in range(4):
        a = np.random.default_rng(s).permutation(x)
        b = x[np.random.default_rng(s).permutation(len(x))]
        np.testing.assert_array_equal(a, b)


def test_resampling_indices_do_not_depend_on_the_cumsum_order(gold):
    """Seeds 0..199: np.cumsum, a 64-blocked cumsum and a long-double cumsum give the same indices for the golden
    weights, so the device comparisons exclude nothing."""
    g, _ = gold
    w = g["ref/importance_weights"]
    n = len(w)
    c0 = np.cumsum(w)
    c0 = c0 / c0[-1]
    blocks = [np.cumsum(w[i:i + 64]) for i in range(0, n, 64)]
    carry, c1 = 0.0, []
    for b in blocks:
        c1.append(b + carry)
        carry = c1[-1][-1]
    c1 = np.concatenate(c1)
    c1 = c1 / c1[-1]
    c2 = np.cumsum(w.astype(np.longdouble))
    c2 = c2 / c2[-1]
    for s in range(200):
        pos = (np.random.default_rng(s).random() + np.arange(n)) / n
        i0 = np.searchsorted(c0, pos, side='right')
        np.testing.assert_array_equal(i0, np.searchsorted(c1, pos, side='right'))
        np.testing.assert_array_equal(i0, np.searchsorted(c2, pos.astype(np.longdouble), side='right'))


def test_bounds_respect_the_projects_tolerances(gold, gold_hp):
    """Ceiling: at the golden size no derived bound exceeds what tests/test_merge_cpu.py gives the field."""
    b = hp.bounds(gold_hp)
    assert b["logvol"].max() <= 1e-11
    assert b["logwt"].max() <= 1e-10
    assert b["logz"].max() <= 1e-10
    assert b["information"].max() <= 1e-9
    err = np.asarray(gold_hp["logzerr"], dtype=np.float64)
    assert (b["logzerr"] <= 1e-7 * err + 1e-10).all()
    assert b["rel_w"].max() <= 1e-9


@pytest.mark.parametrize("name", sorted(merge_cases.cases()))
def test_host_merge_within_bounds_of_hp(name):
    """The host combiner is a float64 evaluation of the same formulas (sequential sums: chains of up to M roundings,
    and d ln X as the difference of two cumulative values, which costs it n = R N times the volume's error in logwt):
    it is held to the long-double values at the project's own tolerances for these fields."""
    args = merge_cases.cases()[name]
    m = merge_cases.host_merge(args)
    ref = hp.merge_hp(args["dead_logl"], args["niter"], args["live_logl"])
    f = lambda k: np.asarray(ref[k], dtype=np.float64)  # noqa: E731
    np.testing.assert_array_equal(m.logl, f("logl"))
    np.testing.assert_array_equal(m.samples_n, ref["samples_n"])
    np.testing.assert_allclose(m.logvol, f("logvol"), rtol=0, atol=1e-11)
    np.testing.assert_allclose(m.logwt, f("logwt"), rtol=0, atol=1e-10)
    np.testing.assert_allclose(m.logz, f("logz"), rtol=0, atol=1e-10)
    np.testing.assert_allclose(m.information, f("information"), rtol=0, atol=1e-9)
    np.testing.assert_allclose(m.logzerr, f("logzerr"), rtol=1e-7, atol=1e-10)
