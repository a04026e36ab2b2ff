"""The strand bootstrap of a merged run on the host (dynesty_amd/errors.py through ensemble.MergedRun): the host form
given the reference's own strand draws against utils.resample_run (tests/golden/merge_bootstrap.npz, tools/make_golden.py
gen_merge_bootstrap); multiplicities of one reproduce the merged run; the strand draws against a restatement on
tests/philox_ref.py; the distribution of ln Z against the reference's resample_run and simulate_run; the argument rules.
Bounds: tests/merge_bootstrap_ref.py."""
import os

import numpy as np
import pytest

import bootstrap_cases as bc
import merge_bootstrap_ref as br

SEED = 1234  # fixed in advance: a failing gate is a finding, not a seed to change


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(bc.GOLD, "merge_bootstrap.npz"))


@pytest.fixture(scope="module")
def runs():
    return {name: bc.host_run(name) for name in bc.NAMES}


def check_against_reference(got, scalars, m, f, p, mult, key, label, chains):
    """One bootstrap with the reference's draws: got = dict of idx, samples_n, logvol, logwt, logz; scalars = (ln Z, H).
    `chains`: the chains of the form under test."""
    np.testing.assert_array_equal(got["samples_n"], f[p + "samples_n"], err_msg=label)
    ref_idx = f[p + "samp_idx"].astype(np.int64)
    assert len(got["idx"]) == len(ref_idx)
    np.testing.assert_array_equal(got["idx"], br.sort_in_ties(got["idx"], m.logl), err_msg=f"{label}: the stable order")
    np.testing.assert_array_equal(got["idx"], br.sort_in_ties(ref_idx, m.logl), err_msg=label)
    idx, n = br.expand(m.logl, key, mult)
    np.testing.assert_array_equal(idx, got["idx"])
    np.testing.assert_array_equal(n, got["samples_n"])
    h = br.hp(m, idx, n, 0, 0, False)
    b, ba = br.bounds(h, chains(h["M"])), br.reference_allowance(h)
    worst = 0.0
    for k in ("logvol", "logwt", "logz"):
        worst = max(worst, br.check(got[k], h[k], b[k], f"{label} {k}"))
        br.check(got[k], f[p + k], b[k] + ba[k], f"{label} {k} vs reference")
    worst = max(worst, br.check(scalars[0], h["logz"][-1], b["logz_last"], f"{label} ln Z"))
    br.check(scalars[0], f[p + "logz"][-1], b["logz_last"] + ba["logz_last"], f"{label} ln Z vs reference")
    worst = max(worst, br.check(scalars[1], h["information"], b["information"], f"{label} H"))
    br.check(scalars[1], f[p + "information"], b["information"] + ba["information"], f"{label} H vs reference")
    return worst


@pytest.mark.parametrize("name", bc.NAMES)
def test_host_form_with_the_references_draws(fix, runs, name):
    m = runs[name]
    key, S = bc.strands(m)
    for i in range(bc.NCALLS):
        p = f"{name}/{i}/"
        mult = bc.multiplicities(fix[p + "draws"], S)
        got = m.resample_run(mult=mult)
        lz, h, _, _, npts = m._err_bootstrap(0, 0, 1, False, mult, False)
        assert npts[0] == len(got["idx"])
        check_against_reference(got, (lz, h), m, fix, p, mult, key, f"host {name} call {i}", br.host_chains)


def test_the_new_cases_have_the_ties_they_are_for(runs, fix):
    m = runs["h_bigplateau"]
    l, cnt = np.unique(m.logl, return_counts=True)
    L = l[np.argmax(cnt)]
    final = np.concatenate([m.samples_n[:-1] - m.samples_n[1:], [1]]).astype(bool)
    assert cnt.max() == 2100 + 11 and int(final[m.logl == L].sum()) == 11
    key, S = bc.strands(m)
    for b in range(8):  # the group's positions contain a multiple of 2048
        r = m.resample_run(seed=SEED, boot=b)
        pos = np.flatnonzero(m.logl[r["idx"]] == L)
        assert pos[0] <= 2048 <= pos[-1], (b, pos[0], pos[-1])
    e = runs["i_endties"]
    ef = np.concatenate([e.samples_n[:-1] - e.samples_n[1:], [1]]).astype(bool)
    assert max(int(ef[e.logl == v].sum()) for v in np.unique(e.logl[ef])) == 40
    for name in bc.TIE_FREE:
        assert (np.diff(runs[name].logl) > 0).all(), name


@pytest.mark.parametrize("name", bc.NAMES)
def test_multiplicities_of_one_are_the_merged_run(runs, name):
    m = runs[name]
    key, S = bc.strands(m)
    r = m.resample_run(mult=np.ones(S, dtype=np.int64))
    np.testing.assert_array_equal(r["idx"], np.arange(m.niter))
    if name in bc.TIE_FREE:
        np.testing.assert_array_equal(r["samples_n"], m.samples_n)
        h = br.hp(m, r["idx"], r["samples_n"], 0, 0, False)
        b = br.bounds(h, br.host_chains(h["M"]))
        br.check(r["logvol"], m.logvol, 2 * b["logvol"], f"{name} identity logvol vs the merged run")
        br.check(r["logz"], m.logz, 2 * b["logz"], f"{name} identity logz vs the merged run")


def test_strand_draws(runs):
    from dynesty_amd import errors
    for S in (1, 40, 180, 1501):
        for seed, b in ((0, 0), (SEED, 1), (2 ** 63 + 7, 2 ** 32 + 5)):
            mu = errors.strand_multiplicities(seed, b, S)
            assert mu.shape == (S,) and mu.sum() == S and (mu >= 0).all()
            np.testing.assert_array_equal(mu, errors.strand_multiplicities(seed, b, S))
            np.testing.assert_array_equal(mu, np.bincount(br.draws(seed, b, S), minlength=S))
            if S > 1:
                assert not np.array_equal(mu, errors.strand_multiplicities(seed, b + 1, S))
    # the bootstrap is that function of (seed, b) and nothing else: alone, in a batch, at another position
    m = runs["golden"]
    a = m.bootstrap_realizations(5, seed=3, first=7, jitter=True, means=True)
    for i in (0, 4):
        one = m.bootstrap_realizations(1, seed=3, first=7 + i, jitter=True, means=True)
        for k in a:
            np.testing.assert_array_equal(a[k][i], one[k][0], err_msg=k)
    key, S = bc.strands(m)
    r = m.resample_run(seed=3, boot=7)
    np.testing.assert_array_equal(r["idx"], br.expand(m.logl, key, errors.strand_multiplicities(3, 7, S))[0])
    assert a["npoints"][0] == len(r["idx"])
    s = m.simulate_run(seed=3, boot=7)
    np.testing.assert_array_equal(s["idx"], r["idx"])
    assert s["logz"][-1] != r["logz"][-1]
    h = br.hp(m, r["idx"], r["samples_n"], 3, 7, True)
    b = br.bounds(h, br.host_chains(h["M"]))
    for k in ("logvol", "logwt", "logz"):
        br.check(s[k], h[k], b[k], f"host simulate_run {k}")
    br.check(a["logz"][0], h["logz"][-1], b["logz_last"], "host simulated ln Z")
    br.check(a["mean"][0], h["mean"], b["mean"], "host simulated mean")


def test_logz_distribution_against_the_reference(fix, runs):
    m = runs["golden"]
    n = 2000
    res = np.concatenate([m.bootstrap_realizations(500, seed=SEED, first=f)["logz"] for f in range(0, n, 500)])
    br.gates(res, fix["golden/resample/logz"], "host resample_run")
    sim = np.concatenate([m.bootstrap_realizations(500, seed=SEED, first=f, jitter=True)["logz"] for f in range(0, n, 500)])
    br.gates(sim, fix["golden/simulate/logz"], "host simulate_run")
    mean, sd = m.logz_error_sampling(64, seed=SEED)
    assert mean == res[:64].mean() and sd == res[:64].std(ddof=1)
    mean, sd = m.logz_error_total(64, seed=SEED)
    assert mean == sim[:64].mean() and sd == sim[:64].std(ddof=1)
    assert sim.std() > res.std()


def test_argument_rules(runs):
    from dynesty_amd import ensemble, errors
    m = runs["golden"]
    key, S = bc.strands(m)
    ones = np.ones(S, dtype=np.int64)
    for bad in (dict(nboot=0), dict(nboot=65537), dict(nboot=1, first=-1), dict(nboot=1, seed=-1), dict(nboot=1, seed=2 ** 64),
                dict(nboot=2, first=2 ** 63 - 1)):
        with pytest.raises(ValueError):
            m.bootstrap_realizations(**bad)
    for mult in (ones[:-1], -ones, ones.astype(np.float64), np.zeros(S, dtype=np.int64)):  # the last: M' = 0
        with pytest.raises(ValueError):
            m.resample_run(mult=mult)
    with pytest.raises(ValueError):
        m._err_bootstrap(0, 0, 2, False, ones, False)  # given multiplicities are one bootstrap
    with pytest.raises(ValueError):
        m.resample_run(boot=-1)
    big = np.zeros(S, dtype=np.int64)
    big[0] = 2 ** 31 - 1  # M' >= 2^31
    with pytest.raises(ValueError):
        m.resample_run(mult=big)
    for f in (m.logz_error_sampling, m.logz_error_total):
        with pytest.raises(ValueError):
            f(1)
    with pytest.raises(ValueError):
        errors.strand_multiplicities(0, 0, 0)
    bare = ensemble.MergedRun({k: m[k] for k in ("niter", "logl", "samples_n", "samples_run")})
    with pytest.raises(ValueError, match="bookkeeping"):
        bare.bootstrap_realizations(1)
    with pytest.raises(ValueError, match="bookkeeping"):
        bare.resample_run()
    nos = ensemble.MergedRun({k: m[k] for k in ("niter", "logl", "samples_n", "samples_run", "samples_id")})
    with pytest.raises(ValueError, match="samples"):
        nos.bootstrap_realizations(1, means=True)
    np.testing.assert_array_equal(nos.bootstrap_realizations(2, seed=5)["logz"], m.bootstrap_realizations(2, seed=5)["logz"])
    lz0 = m.logz_error(8, seed=2)  # logz_error stays as it is: the jitter alone
    r = m.logz_realizations(8, 2)["logz"]
    assert lz0 == (float(r.mean()), float(r.std(ddof=1)))
