"""Statistical errors of a merged run on the host (dynesty_amd/errors.py through ensemble.MergedRun): the package's
Philox words against tests/philox_ref.py; one realization against its long-double restatement
(tests/merge_errors_ref.py) at the bounds that derives; the distribution of ln Z against the reference's
utils.jitter_run (tests/golden/merge_errors.npz, tools/make_golden.py gen_merge_errors); reweighting against
utils.reweight_run; the argument rules."""
import os

import numpy as np
import pytest

import merge_cases
import merge_errors_ref as er
import philox_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REALS = (0, 1, 2 ** 32 + 5)
KS_CRIT = 1.95 * np.sqrt(2 / 2000)  # two samples of 2000 at level 0.001


def ks2(a, b):
    """Two-sample Kolmogorov-Smirnov statistic."""
    a, b = np.sort(a), np.sort(b)
    x = np.concatenate([a, b])
    return float(np.max(np.abs(np.searchsorted(a, x, side="right") / len(a) - np.searchsorted(b, x, side="right") / len(b))))


def ks_crit(n, m):
    return 1.95 * np.sqrt((n + m) / (n * m))


def reference_gates(lz, fix, label):
    """The three gates of the issue against one set of the reference's ln Z values."""
    ks = ks2(lz, fix)
    se = np.sqrt(lz.var(ddof=1) / len(lz) + fix.var(ddof=1) / len(fix))
    dm = abs(lz.mean() - fix.mean()) / se
    ratio = lz.std(ddof=1) / fix.std(ddof=1)
    print(f"[merge errors {label}] KS {ks:.4f} (< {KS_CRIT:.4f}), mean difference {dm:.2f} se, sd ratio {ratio:.4f}")
    assert ks < KS_CRIT
    assert dm < 4
    assert abs(ratio - 1) <= 4 / np.sqrt(2000)


def host_run(args):
    return merge_cases.host_merge(args, prior_transform=lambda u: 20.0 * u - 10.0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "merge.npz")), np.load(os.path.join(GOLD, "merge_errors.npz"))


@pytest.fixture(scope="module")
def gold_run(gold):
    """The golden merged run with the reference's own parameter rows."""
    from dynesty_amd import ensemble
    g, _ = gold
    m = ensemble.merge_static_runs(g["static/dead_l"], g["static/nit"], g["static/live_l"], g["static/dead_u"],
                                   g["static/live_u"])
    np.testing.assert_array_equal(m.logl, g["ref/logl"])
    m["samples"] = g["ref/samples"]
    return m


@pytest.fixture(scope="module")
def gold_lz(gold_run):
    return gold_run.logz_realizations(2000, seed=1234, first=0)


def test_philox_blocks_and_uniforms_match_the_restatement():
    from dynesty_amd import errors
    for seed in (0, 1234, 2 ** 63 + 7):
        for seq in (0, 1, 2 ** 32 + 5):
            for blk in (0, 1, 2 ** 32):
                w = errors.philox_blocks(seed, seq, blk)
                np.testing.assert_array_equal(w, philox_ref.philox_blocks(seed, seq, blk))
                assert tuple(int(x) for x in w) == philox_ref.philox_block_int(seed, seq, blk)
                np.testing.assert_array_equal(errors.uniform_double(w[0], w[1]), philox_ref.uniform_double(w[0], w[1]))
            u = errors.uniforms(seed, [seq], 37)[0]
            np.testing.assert_array_equal(u, er.uniforms(seed, seq, 37))
            assert ((u > 0) & (u <= 1)).all()
    assert float(errors.uniform_double(0xFFFFFFFF, 0xFFFFFFFF)) == 1.0
    assert float(errors.uniform_double(0, 0)) == 2.0 ** -53


def test_transcendental_allowance_is_calibrated():
    """The 1 ulp per log / log1p / expm1 / exp the bounds allow holds for a float64 evaluator that is not the device's."""
    for name, ulps in er.calibrate().items():
        print(f"[merge errors] numpy {name}: {ulps:.3f} ulp against long double")
        assert ulps <= 1.0, name


def check_run(m, seed, label, logrwt=None, jitter=True, reals=REALS):
    """The host form of the realizations `reals` of the merged run `m` within the host bounds of the restatement."""
    worst = 0.0
    for r in reals:
        hp = er.realization_hp(m.logl, m.samples_n, seed, r, jitter, logrwt, m.samples)
        b = er.bounds(hp, er.host_chains(hp["M"]))
        one = m.logz_realizations(1, seed, r, logrwt=logrwt, means=True, jitter=jitter)
        for k in er_fields:
            got = m.realization(k, seed, r, jitter=jitter, logrwt=logrwt)
            worst = max(worst, er.check(got, hp[k], b[k], f"{label} r={r} {k}"))
        assert np.isfinite(one["logz"]).all() and np.isfinite(one["information"]).all() and np.isfinite(one["mean"]).all()
        worst = max(worst, er.check(one["logz"], hp["logz"][-1], b["logz_last"], f"{label} r={r} ln Z"))
        worst = max(worst, er.check(one["information"], hp["information"], b["information"], f"{label} r={r} H"))
        worst = max(worst, er.check(one["ess"], hp["ess"], b["ess"], f"{label} r={r} ESS"))
        worst = max(worst, er.check(one["mean"][0], hp["mean"], b["mean"], f"{label} r={r} mean"))
        s64 = er.steps64(seed, r, m.samples_n, jitter)
        ks = np.unique(np.linspace(0, hp["M"] - 1, 16).astype(int))
        er.check(m.realization("logvol", seed, r, jitter=jitter)[ks], er.fsum_logvol(s64, ks),
                 b["logvol"][ks] + 8 * er.U * np.abs(er.fsum_logvol(s64, ks)), f"{label} r={r} ln X against fsum")
    return worst


er_fields = ("logvol", "logwt", "logz")


def test_golden_realizations_within_bounds_of_the_restatement(gold_run):
    check_run(gold_run, 1234, "golden")


@pytest.mark.parametrize("name", sorted(merge_cases.cases()))
def test_case_realizations_within_bounds_of_the_restatement(name):
    m = host_run(merge_cases.cases()[name])
    check_run(m, 99, name)
    if name == "g_span":  # 2000 nats between the first and the last point
        r = m.logz_realizations(8, 99, means=True)
        assert all(np.isfinite(r[k]).all() for k in r)


def test_a_realization_does_not_depend_on_the_batch(gold_run):
    a = gold_run.logz_realizations(5, seed=3, first=7, means=True)
    for i in range(5):
        one = gold_run.logz_realizations(1, seed=3, first=7 + i, means=True)
        for k in a:
            np.testing.assert_array_equal(a[k][i], one[k][0], err_msg=k)
    # across the host form's own tiles (nreal above the tile of this M)
    big = gold_run.logz_realizations(1500, seed=3, first=0)
    np.testing.assert_array_equal(big["logz"][7:12], a["logz"])


def test_logz_distribution_against_the_reference(gold, gold_lz):
    _, f = gold
    reference_gates(gold_lz["logz"], f["jitter/exact/logz"], "host vs exact form")
    reference_gates(gold_lz["logz"], f["jitter/approx/logz"], "host vs approx=True")


def test_information_distribution_against_the_reference(gold, gold_lz):
    _, f = gold
    for form in ("exact", "approx"):
        ks = ks2(gold_lz["information"][:200], f[f"jitter/{form}/information"])
        print(f"[merge errors] information, {form}: KS {ks:.4f} (< {ks_crit(200, 200):.4f})")
        assert ks < ks_crit(200, 200)


def test_logz_error(gold_run, gold_lz):
    mean, sd = gold_run.logz_error(2000, seed=1234)
    assert mean == gold_lz["logz"].mean() and sd == gold_lz["logz"].std(ddof=1)
    print(f"[merge errors] golden: ln Z = {mean:.4f} +- {sd:.4f} over realizations; the summary's logzerr {gold_run.logzerr[-1]:.4f}")
    with pytest.raises(ValueError):
        gold_run.logz_error(1)


def reference_allowance(hp):
    """The reference's own float64 arithmetic against the exact value: sequential sums (host chains) and its volume
    steps log(n / (n + 1)), whose quotient next to 1 is rounded at full size: u absolute per step, M u by the end."""
    b = er.bounds(hp, er.host_chains(hp["M"]))
    extra = hp["M"] * 2 * er.U
    return {k: b[k] + extra for k in b}


def test_reweight_against_the_reference(gold, gold_run):
    g, f = gold
    logp_new = f["reweight/logp_new"]
    logrwt = logp_new - gold_run.logl
    hp = er.realization_hp(gold_run.logl, gold_run.samples_n, 0, 0, False, logrwt, gold_run.samples)
    b, br = er.bounds(hp, er.host_chains(hp["M"])), reference_allowance(hp)
    rw = gold_run.reweight(logp_new)
    er.check(rw["logz"], f["reweight/logz"][-1], b["logz_last"] + br["logz_last"], "reweight ln Z vs reference")
    er.check(rw["information"], f["reweight/information"][-1], b["information"] + br["information"], "reweight H vs reference")
    er.check(rw["logz"], hp["logz"][-1], b["logz_last"], "reweight ln Z")
    er.check(rw["information"], hp["information"], b["information"], "reweight H")
    er.check(rw["ess"], hp["ess"], b["ess"], "reweight ESS")
    er.check(rw["mean"], hp["mean"], b["mean"], "reweight mean")
    for k in ("logwt", "logz"):
        got = gold_run.realization(k, jitter=False, logrwt=logrwt)
        er.check(got, f["reweight/" + k], b[k] + br[k], f"reweight {k} per point vs reference")
        er.check(got, hp[k], b[k], f"reweight {k} per point")
    # logp_old given explicitly is the same call
    again = gold_run.reweight(logp_new, logp_old=gold_run.logl)
    assert again["logz"] == rw["logz"] and again["information"] == rw["information"]


def test_expected_volumes_reproduce_the_merged_run(gold, gold_run):
    g, _ = gold
    hp = er.realization_hp(gold_run.logl, gold_run.samples_n, 0, 0, False, None, gold_run.samples)
    b = er.bounds(hp, er.host_chains(hp["M"]))
    r = gold_run.logz_realizations(1, jitter=False, means=True)
    w = gold_run.importance_weights()
    er.check(r["logz"], gold_run.logz[-1], 2 * b["logz_last"], "expected ln Z vs the merged run")
    er.check(r["information"], gold_run.information[-1], 2 * b["information"], "expected H vs the merged run")
    er.check(r["ess"], 1.0 / np.sum(w * w), 2 * b["ess"], "expected ESS vs the merged run")
    er.check(r["mean"][0], w @ gold_run.samples, 2 * b["mean"], "expected mean vs the merged run")
    for k in er_fields:
        er.check(gold_run.realization(k, jitter=False), gold_run[k], 2 * b[k], f"expected {k} vs the merged run")
    # a zero weight: -inf in logrwt drops the point and nothing else
    lr, top = np.zeros(hp["M"]), int(np.argmax(gold_run.logwt))
    lr[top] = -np.inf
    z = gold_run.logz_realizations(1, jitter=False, logrwt=lr, means=True)
    assert np.isfinite(z["logz"]).all() and np.isfinite(z["mean"]).all() and z["logz"][0] < r["logz"][0]
    assert gold_run.realization("logwt", jitter=False, logrwt=lr)[top] == -np.inf


def test_argument_rules(gold_run):
    m, M = gold_run, gold_run.niter
    for bad in (dict(nreal=0), dict(nreal=65537), dict(nreal=2, jitter=False), dict(nreal=1, first=-1),
                dict(nreal=1, seed=-1), dict(nreal=1, seed=2 ** 64), dict(nreal=1, logrwt=np.zeros(M - 1))):
        with pytest.raises(ValueError):
            m.logz_realizations(**bad)
    for v in (np.nan, np.inf):
        lr = np.zeros(M)
        lr[5] = v
        with pytest.raises(ValueError):
            m.logz_realizations(1, logrwt=lr)
        with pytest.raises(ValueError):
            m.realization("logz", logrwt=lr)
    for bad in (dict(field="logzerr"), dict(field="logz", real=-1), dict(field="logz", first=-1),
                dict(field="logz", first=M - 1, count=2), dict(field="logz", first=0, count=-1)):
        with pytest.raises(ValueError):
            m.realization(**bad)
    assert len(m.realization("logz", first=M, count=0)) == 0
    with pytest.raises(ValueError):
        m.reweight(np.zeros(M - 1))
    from dynesty_amd import ensemble
    bare = ensemble.MergedRun(logl=m.logl, samples_n=m.samples_n, niter=M)
    with pytest.raises(ValueError):  # means without samples
        bare.logz_realizations(1, means=True)
    assert np.array_equal(bare.logz_realizations(2, seed=1234)["logz"], m.logz_realizations(2, seed=1234)["logz"])
