"""dynamic.merge_strands -- all strands of a batch folded in one pass, the host mirror of the device's fold
(dh_merged_fold) -- against dynamic.merge_batch applied strand after strand: the order and every integer field exactly,
the float fields to 1e-12; against the reference's own dynamic run (tests/golden/batch_combine.npz) to the tolerances of
tests/test_dynamic_cpu.py; and on the plateau case of that file that can be followed by hand.  dynamic.single_run and
dynamic.fold_batch on host runs."""
import os

import numpy as np
import pytest

from dynesty_amd import dynamic
from dynesty_amd.ensemble import MergedRun

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_combine.npz")
INT_FIELDS = ("samples_n", "samples_id", "samples_batch", "samples_it", "ncall", "samples_seq", "samples_run")
FLOAT_FIELDS = ("logvol", "logwt", "logz", "information", "logzerr")


def static_run(rng, nlive, ndead, values, ndim=2):
    """One static run with ties: ln L drawn from `values`, dead points then the final live points ascending."""
    logl = np.sort(rng.choice(values, size=ndead + nlive))
    n = np.concatenate([np.full(ndead, nlive), np.arange(nlive, 0, -1)]).astype(np.int64)
    m = len(logl)
    return dict(logl=logl, n=n, id=rng.integers(0, nlive, m), it=rng.integers(0, 1000, m), nc=rng.integers(1, 9, m),
                u=rng.random((m, ndim)), v=rng.normal(size=(m, ndim)))


def base_of(s):
    zero = np.zeros(len(s["logl"]))
    return MergedRun(niter=len(s["logl"]), logl=s["logl"], samples_n=s["n"], samples_id=s["id"], samples_it=s["it"],
                     ncall=s["nc"], samples_u=s["u"], samples=s["v"], samples_run=np.zeros(len(zero), dtype=np.int64),
                     samples_seq=np.arange(len(zero)), logvol=zero, logwt=zero, logz=zero, information=zero, logzerr=zero)


def assert_same(a, b, tol=1e-12):
    np.testing.assert_array_equal(a.logl, b.logl)
    np.testing.assert_array_equal(a.samples_u, b.samples_u)
    np.testing.assert_array_equal(a.samples, b.samples)
    for k in INT_FIELDS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for k in FLOAT_FIELDS:
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=tol, err_msg=k)
    assert a.batch_nlive == b.batch_nlive and a.batch_bounds == b.batch_bounds
    assert a.niter == b.niter and a.eff == b.eff


def one_case(seed):
    """(base, strands, logl_min, logl_max): ties between base and strands and across strands (integer ln L); R in
    {1, 3, 5}; logl_min equal to a base value in two cases of three; every fourth case with the strands above the
    base's maximum, every fifth with more new points than the base holds."""
    rng = np.random.default_rng(seed)
    R = (1, 3, 5)[seed % 3]
    nlive, nnew = int(rng.integers(12, 30)), int(rng.integers(8, 20))
    big = seed % 5 == 0
    base = static_run(rng, nlive, int(rng.integers(5, 40)) if big else int(rng.integers(60, 160)), np.arange(0, 300))
    if seed % 3 == 2:
        logl_min = float(rng.integers(20, 200)) + 0.5
    else:
        logl_min = float(rng.choice(base["logl"][base["logl"] < 250]))
    lo = int(base["logl"].max()) + 1 if seed % 4 == 0 else int(np.floor(logl_min)) + 1
    strands = [static_run(rng, nnew, int(rng.integers(0, 60)) + (60 if big else 0), np.arange(lo, lo + 200))
               for _ in range(R)]
    return base_of(base), strands, logl_min, float(lo + 500)


def test_merge_strands_equals_merge_batch_strand_after_strand():
    compared, kinds = 0, set()
    for seed in range(240):
        base, strands, lmin, lmax = one_case(seed)
        try:
            want = base
            for s in strands:
                want = dynamic.merge_batch(want, s, lmin, lmax)
        except ValueError:
            continue  # a plateau longer than the live count where it starts, at some stage of the sequence
        got = dynamic.merge_strands(base, strands, lmin, lmax)
        assert_same(got, want)
        compared += 1
        new = sum(len(s["logl"]) for s in strands)
        kinds.add((len(strands), bool((base.logl == lmin).any()), bool(min(s["logl"].min() for s in strands) > base.logl.max()),
                   new > len(base.logl)))
        assert len(np.unique(got.logl)) < len(got.logl)  # ties are present
    assert compared >= 120, compared
    assert {k[0] for k in kinds} == {1, 3, 5}
    assert any(k[1] for k in kinds) and any(k[2] for k in kinds) and any(k[3] for k in kinds), kinds


def test_merge_strands_folds_the_golden_batches_like_combine_runs():
    g = np.load(GOLDEN)
    f = {k: g[f"0/base/{k}"] for k in ("logl", "logvol", "n", "id", "it", "nc", "u", "logz", "logzvar", "h", "batch")}
    m = MergedRun(niter=len(f["logl"]), logl=f["logl"], logvol=f["logvol"], logz=f["logz"], information=f["h"],
                  logzerr=np.sqrt(f["logzvar"]), samples_n=f["n"], samples_id=f["id"], samples_it=f["it"], ncall=f["nc"],
                  samples_u=f["u"], samples_batch=f["batch"])
    for b in range(3):
        strand = {k: g[f"{b}/new/{k}"] for k in ("logl", "n", "id", "it", "nc", "u")}
        lmin, lmax = g[f"{b}/new_bounds"]
        m = dynamic.merge_strands(m, [strand], lmin, lmax)

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


def test_merge_strands_plateau_volumes_and_heads():
    """tests/test_dynamic_cpu.py's hand-followed case through the one-pass form; then a group of n_i + 1 equal values,
    which leaves no positive volume: ValueError, as the strand-after-strand form raises it."""
    base = MergedRun(logl=np.array([1., 2., 2., 3.]), samples_n=np.array([2, 2, 2, 1]), samples_id=np.array([0, 1, 0, 1]),
                     logvol=np.zeros(4), logz=np.zeros(4), information=np.zeros(4), logzerr=np.zeros(4))
    strand = dict(logl=np.array([2., 2.5, 4.]), n=np.array([2, 2, 1]), id=np.array([0, 1, 1]))
    m = dynamic.merge_strands(base, [strand], 1.5, np.inf)
    np.testing.assert_array_equal(m.logl, [1., 2., 2., 2., 2.5, 3., 4.])
    np.testing.assert_array_equal(m.samples_batch, [0, 0, 0, 1, 1, 0, 1])
    np.testing.assert_array_equal(m.samples_id, [0, 1, 0, 2, 3, 1, 3])
    np.testing.assert_array_equal(m.samples_n, [2, 4, 4, 3, 3, 2, 1])
    lv = [np.log(2. / 3.)]
    x0 = np.exp(lv[0])
    lv += [np.log(x0 * (1 - k / 5.)) for k in (1, 2, 3)]
    lv += [lv[-1] + np.log(3. / 4.), lv[-1] + np.log(3. / 4.) + np.log(2. / 3.)]
    lv += [lv[-1] + np.log(1. / 2.)]
    np.testing.assert_allclose(m.logvol, lv, rtol=0, atol=1e-14)
    # five equal values entered at n = 4: the fifth would have volume 0
    long_ = dict(logl=np.array([2., 2., 2., 4.]), n=np.array([2, 2, 2, 1]), id=np.array([0, 1, 0, 1]))
    with pytest.raises(ValueError):
        dynamic.merge_batch(base, long_, 1.5, np.inf)
    with pytest.raises(ValueError):
        dynamic.merge_strands(base, [long_], 1.5, np.inf)
    with pytest.raises(ValueError, match="No new samples"):
        dynamic.merge_strands(base, [], 1.5, np.inf)
    with pytest.raises(ValueError, match="logl_min"):
        dynamic.merge_strands(base, [strand], 2.0, np.inf)


def test_single_run_renumbers_a_merge_of_static_runs():
    """id <- run * nlive + id and run <- 0, nlive read off the first live count (runs * nlive); a run that is one
    already comes back unchanged."""
    run = np.array([0, 1, 2, 1, 0, 2, 0, 1, 2])
    ids = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1])
    m = MergedRun(logl=np.arange(9.), samples_n=np.array([6, 6, 6, 6, 5, 4, 3, 2, 1]), samples_run=run.copy(),
                  samples_id=ids.copy())
    out = dynamic.single_run(m)
    np.testing.assert_array_equal(out.samples_id, run * 2 + ids)
    np.testing.assert_array_equal(out.samples_run, np.zeros(9, dtype=np.int64))
    again = dynamic.single_run(out)
    np.testing.assert_array_equal(again.samples_id, run * 2 + ids)


def test_fold_batch_on_a_host_run_is_merge_strands_of_the_result_dict():
    rng = np.random.default_rng(5)
    base = base_of(static_run(rng, 20, 100, np.arange(0, 300)))
    R, N, cap, D = 3, 10, 40, 2
    niter = np.array([40, 17, 0])
    dead_l = np.sort(rng.integers(100, 250, (R, cap)).astype(float), axis=1)
    live_l = rng.integers(250, 300, (R, N)).astype(float)
    out = dict(niter=niter, dead_logl=dead_l, live_logl=live_l, dead_u=rng.random((R, cap, D)), live_u=rng.random((R, N, D)),
               dead_id=rng.integers(0, N, (R, cap)), dead_it=rng.integers(0, 99, (R, cap)),
               dead_nc=rng.integers(1, 9, (R, cap)), live_it=rng.integers(0, 99, (R, N)))

    def ptform(u):
        return 2. * u - 1.
    got = dynamic.fold_batch(base, out, N, 50.5, 400., prior_transform=ptform)
    want = base
    for r in range(R):
        want = dynamic.merge_batch(want, dynamic.strand_of(out, r, N, prior_transform=ptform), 50.5, 400.)
    assert_same(got, want)
    assert got.batch_nlive == [20, N, N, N] and len(got.logl) == len(base.logl) + int(niter.sum()) + R * N


@pytest.mark.parametrize("name", sorted(__import__("fold_cases").CASES))
def test_device_cases_hold_what_they_promise_and_the_restatement_agrees(name):
    """tests/fold_cases.py, which the device's test runs: M + W beyond one scan chunk; a plateau across 2047 / 2048 and
    one across a multiple of 256, base and strand points mixed; base values equal to logl_min; and on them the one-pass
    form against strand after strand, and against the long-double restatement (tests/fold_hp_ref.py)."""
    import fold_cases
    import fold_hp_ref
    import merge_cases
    kw = dict(fold_cases.CASES[name], pt=True)
    base, new, lmin, lmax = fold_cases.make(**kw)

    def ptform(u):
        return 20. * u - 10.
    mb = dynamic.single_run(merge_cases.host_merge(base, prior_transform=ptform))
    assert (mb.samples_run == 0).all() and len(np.unique(mb.samples_id)) == 3 * kw["base_nlive"]
    strands = fold_cases.host_strands(new, kw["strand_nlive"], ptform)
    got = dynamic.merge_strands(mb, strands, lmin, lmax)
    want = mb
    for s in strands:
        want = dynamic.merge_batch(want, s, lmin, lmax)
    assert_same(got, want)
    T = len(got.logl)
    assert T > 2048 and (mb.logl == lmin).sum() >= 3 and got.logl[2047] == got.logl[2048]
    for lo, hi in kw["plateaus"]:
        assert (got.logl[lo:hi] == got.logl[lo]).all() and set(got.samples_batch[lo:hi] > 0) == {False, True}
    assert any(lo // 256 != (hi - 1) // 256 for lo, hi in kw["plateaus"][1:])
    if kw.get("above"):
        assert strands[-1]["logl"].min() > mb.logl.max()
    if name == "more_new_than_base":
        assert T - len(mb.logl) > len(mb.logl)
    ref = fold_hp_ref.fold_hp(got.logl, got.samples_n)
    b = fold_hp_ref.bounds(ref)
    # ln X at the restatement's bound (the host's sum is sequential: T roundings in place of the device's scan chain);
    # ln w and ln Z at the project's tolerances (the host differences cumulative volumes, the restatement does not)
    want = {k: np.asarray(ref[k], dtype=np.float64) for k in ("logvol", "logwt", "logz")}
    err = np.abs(got.logvol - want["logvol"])
    assert (err <= b["logvol"] + T * 2.0 ** -53 * np.abs(want["logvol"])).all(), float(err.max())
    np.testing.assert_allclose(got.logwt, want["logwt"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(got.logz, want["logz"], rtol=0, atol=1e-10)
