"""Statistical errors of the merged run on the device (csrc/merge_errors.hip, dh_merged_realize / dh_merged_realization):
per-point fields and the batch results against the long-double restatement (tests/merge_errors_ref.py) at the bounds it
derives for the device's chains; a realization bit-identical alone and in any batch; the device against the host form;
the distribution of ln Z against the reference's utils.jitter_run (tests/golden/merge_errors.npz); reweighting.

Worst measured error / bound per field is recorded in DESIGN.md section 3.8.2."""
import os

import numpy as np
import pytest

import inputs
import merge_cases
import merge_errors_ref as er
from test_gpu_merge import golden_args, problem_for
from test_merge_errors_cpu import REALS, ks2, ks_crit, reference_allowance, reference_gates

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = ("logvol", "logwt", "logz")


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "merge.npz")), np.load(os.path.join(GOLD, "merge_errors.npz"))


def merge_case(ctx, name, gold):
    if name == "golden":
        return ctx.merge_runs(inputs.problem("C1"), **golden_args(gold[0]))
    args = merge_cases.cases()[name]
    return ctx.merge_runs(problem_for(args["live_u"].shape[2]), **args)


def arrays(d):
    return d.field("logl"), d.field("samples_n"), d.field("samples")


def check_batch(one, hp, b, label, scale=1.0):
    er.check(one["logz"], hp["logz"][-1], scale * b["logz_last"], f"{label} ln Z")
    er.check(one["information"], hp["information"], scale * b["information"], f"{label} H")
    er.check(one["ess"], hp["ess"], scale * b["ess"], f"{label} ESS")
    if "mean" in one:
        er.check(one["mean"][0], hp["mean"], scale * b["mean"], f"{label} mean")


@pytest.mark.parametrize("name", ["golden", "b_plateau", "c_ragged", "d_single", "e_large", "g_span"])
def test_per_point_fields_within_bounds_of_the_restatement(ctx, gold, name):
    d = merge_case(ctx, name, gold)
    logl, n, v = arrays(d)
    for r in REALS:
        hp = er.realization_hp(logl, n, 77, r, True, None, v)
        b = er.bounds(hp, er.device_chains(hp["M"]))
        run = d.jitter_run(seed=77, real=r)
        for k in FIELDS:
            er.check(run[k], hp[k], b[k], f"device {name} r={r} {k}")
        one = d.logz_realizations(1, 77, r, means=True)
        assert all(np.isfinite(one[k]).all() for k in one)
        check_batch(one, hp, b, f"device {name} r={r}")


def test_carry_stage_with_more_than_one_block(ctx):
    """More than 256 chunks: the carry stage itself loops.  ln X on both sides of every carry-block boundary against
    the exact sum of the steps; ln Z of three realizations."""
    args = merge_cases.make(np.random.default_rng(21), [140000] * 4, 100, 2)
    d = ctx.merge_runs(problem_for(2), **args)
    M = d.niter
    nblk = -(-M // 2048)
    assert nblk > 256
    logl, n, v = arrays(d)
    edges = [c * 256 * 2048 for c in range(1, -(-nblk // 256))]
    ks = sorted(set([0, 1, 2047, 2048, M - 2, M - 1] + [e + o for e in edges for o in (-2049, -2048, -1, 0, 1, 2047, 2048)]))
    ks += [int(k) for k in np.linspace(3, M - 3, 64 - len(ks)).astype(int)]
    ks = np.array(sorted(set(ks)))
    assert len(ks) >= 60 and all(e - 1 in ks and e in ks for e in edges)
    for r in REALS:
        s64 = er.steps64(5, r, n)
        want = er.fsum_logvol(s64, ks)
        got = d.realization("logvol", 5, r)[ks]
        c = er.device_chains(M)
        # the device's steps and NumPy's are float64 evaluations of the same steps: 4u relative each
        er.check(got, want, (c["scan"] + 4 + 4) * er.U * np.abs(want), f"device carry r={r} ln X against fsum")
        hp = er.realization_hp(logl, n, 5, r, True, None, v)
        b = er.bounds(hp, c)
        check_batch(d.logz_realizations(1, 5, r, means=True), hp, b, f"device carry r={r}")
        er.check(d.realization("logz", 5, r, first=M - 1, count=1), hp["logz"][-1:], b["logz"][-1:], f"device carry r={r} last logz")


@pytest.mark.parametrize("name", ["e_large", "f_wide"])
def test_batch_equals_single_bit_for_bit(ctx, gold, name):
    d = merge_case(ctx, name, gold)
    first = 7
    single = [d.logz_realizations(1, 9, first + i, means=True) for i in range(130)]
    for nreal in (1, 3, 64, 65, 130):
        a = d.logz_realizations(nreal, 9, first, means=True)
        again = d.logz_realizations(nreal, 9, first, means=True)
        plain = d.logz_realizations(nreal, 9, first)
        for k in ("logz", "information", "ess", "mean"):
            np.testing.assert_array_equal(a[k], again[k], err_msg=k)
            np.testing.assert_array_equal(a[k], np.concatenate([s[k] for s in single[:nreal]]), err_msg=f"{k} nreal={nreal}")
            if k != "mean":
                np.testing.assert_array_equal(a[k], plain[k], err_msg=f"{k} without means")
    # at another position of a batch
    off = d.logz_realizations(64, 9, first + 3, means=True)
    for k in off:
        np.testing.assert_array_equal(off[k][:60], np.concatenate([s[k] for s in single[3:63]]), err_msg=k)
    logl, n, v = arrays(d)
    for i in (0, 64, 129):
        hp = er.realization_hp(logl, n, 9, first + i, True, None, v)
        b = er.bounds(hp, er.device_chains(hp["M"]))
        last = d.realization("logz", 9, first + i, first=d.niter - 1, count=1)
        er.check(single[i]["logz"], last, b["logz"][-1:] + b["logz_last"], f"device {name} batch ln Z against the LOGZ slice")


@pytest.mark.parametrize("name", ["golden", "e_large", "f_wide", "g_span"])
def test_device_against_host_form(ctx, gold, name):
    """Realization for realization: both are float64 evaluations of one exact value, each within its own chains' bound."""
    d = merge_case(ctx, name, gold)
    m = d.to_merged_run()
    dev = d.logz_realizations(6, 31, 2 ** 32 + 3, means=True)
    host = m.logz_realizations(6, 31, 2 ** 32 + 3, means=True)
    for i in range(6):
        hp = er.realization_hp(m.logl, m.samples_n, 31, 2 ** 32 + 3 + i, True, None, m.samples)
        bd, bh = er.bounds(hp, er.device_chains(hp["M"])), er.bounds(hp, er.host_chains(hp["M"]))
        for k, bk in (("logz", "logz_last"), ("information", "information"), ("ess", "ess"), ("mean", "mean")):
            er.check(dev[k][i], host[k][i], bd[bk] + bh[bk], f"device vs host {name} r+{i} {k}")
        if i == 0:
            for k in FIELDS:
                er.check(d.realization(k, 31, 2 ** 32 + 3), m.realization(k, 31, 2 ** 32 + 3), bd[k] + bh[k],
                         f"device vs host {name} {k}")


def test_reference_gates_on_device_output(ctx, gold):
    _, f = gold
    d = merge_case(ctx, "golden", gold)
    r = d.logz_realizations(2000, seed=1234, first=0)
    reference_gates(r["logz"], f["jitter/exact/logz"], "device vs exact form")
    reference_gates(r["logz"], f["jitter/approx/logz"], "device vs approx=True")
    for form in ("exact", "approx"):
        ks = ks2(r["information"][:200], f[f"jitter/{form}/information"])
        print(f"[merge errors] device information, {form}: KS {ks:.4f} (< {ks_crit(200, 200):.4f})")
        assert ks < ks_crit(200, 200)
    mean, sd = d.logz_error(2000, seed=1234)
    assert mean == r["logz"].mean() and sd == r["logz"].std(ddof=1)
    print(f"[merge errors] device golden: ln Z = {mean:.4f} +- {sd:.4f}; the summary's logzerr {d.summary['logzerr']:.4f}")


def test_reweight_and_expected_volumes(ctx, gold):
    g, f = gold
    d = merge_case(ctx, "golden", gold)
    logl, n, v = arrays(d)
    M = d.niter
    logp_new = f["reweight/logp_new"]
    logrwt = logp_new - logl
    hp = er.realization_hp(logl, n, 0, 0, False, logrwt, v)
    b, br = er.bounds(hp, er.device_chains(M)), reference_allowance(hp)
    rw = d.reweight(logp_new)
    er.check(rw["logz"], f["reweight/logz"][-1], b["logz_last"] + br["logz_last"], "device reweight ln Z vs reference")
    er.check(rw["information"], f["reweight/information"][-1], b["information"] + br["information"], "device reweight H vs reference")
    check_batch({k: np.atleast_1d(x) if k != "mean" else x[None] for k, x in rw.items()}, hp, b, "device reweight")
    for k in ("logwt", "logz"):
        got = d.realization(k, jitter=False, logrwt=logrwt)
        er.check(got, f["reweight/" + k], b[k] + br[k], f"device reweight {k} per point vs reference")
        er.check(got, hp[k], b[k], f"device reweight {k} per point")
    # expected volumes without logrwt: the merged run's own summary and fields
    hp0 = er.realization_hp(logl, n, 0, 0, False, None, v)
    b0 = er.bounds(hp0, er.device_chains(M))
    e = d.logz_realizations(1, jitter=False, means=True)
    check_batch(e, hp0, b0, "device expected volumes")
    s = d.summary
    er.check(e["logz"], s["logz"], 2 * b0["logz_last"], "device expected ln Z vs the summary")
    er.check(e["information"], s["h"], 2 * b0["information"], "device expected H vs the summary")
    er.check(e["ess"], s["ess"], 2 * b0["ess"], "device expected ESS vs the summary")
    er.check(e["mean"][0], d.mean_and_cov()[0], 2 * b0["mean"], "device expected mean vs the moments")
    np.testing.assert_array_equal(d.realization("logvol", jitter=False), d.field("logvol"))  # the same scan
    for k in ("logwt", "logz"):
        er.check(d.realization(k, jitter=False), d.field(k), 2 * b0[k], f"device expected {k} vs the merged run")
    # a weight of zero; a NaN is refused and the merged run is still there
    lr, top = np.zeros(M), int(np.argmax(d.field("logwt")))
    lr[top] = -np.inf
    z = d.logz_realizations(1, jitter=False, logrwt=lr, means=True)
    hpz = er.realization_hp(logl, n, 0, 0, False, lr, v)
    check_batch(z, hpz, er.bounds(hpz, er.device_chains(M)), "device zero weight")
    assert z["logz"][0] < e["logz"][0] and d.realization("logwt", jitter=False, logrwt=lr)[top] == -np.inf
    zj = d.logz_realizations(3, 4, logrwt=lr, means=True)
    assert all(np.isfinite(zj[k]).all() for k in zj)
    for bad in (np.nan, np.inf):
        lr[5] = bad
        with pytest.raises(ValueError, match="logrwt"):
            d.logz_realizations(1, logrwt=lr)
        with pytest.raises(ValueError, match="logrwt"):
            d.realization("logz", logrwt=lr)
    np.testing.assert_array_equal(d.logz_realizations(1, jitter=False)["logz"], e["logz"])


def test_argument_rules(gold):
    from dynesty_amd import _lib
    c = _lib.Context(0)
    lz, mean = np.empty(4), np.empty((4, 3))
    P = _lib._ptr
    assert c.lib.dh_merged_realize(c.handle, 0, 0, 1, 1, None, 0, P(lz), None, None, None) == _lib.ERR_ARG  # no merged run
    assert c.lib.dh_merged_realization(c.handle, 0, 0, 1, None, 3, 0, 1, P(lz)) == _lib.ERR_ARG
    d = merge_case(c, "golden", gold)
    M = d.niter
    call = lambda *a: c.lib.dh_merged_realize(c.handle, *a)  # noqa: E731
    assert call(0, 0, 1, 1, None, 0, P(lz), None, None, None) == 0
    for a in ((0, 0, 0, 1, None, 0, P(lz), None, None, None), (0, 0, 65537, 1, None, 0, P(lz), None, None, None),
              (0, 0, 2, 0, None, 0, P(lz), None, None, None), (0, -1, 1, 1, None, 0, P(lz), None, None, None),
              (0, 0, 1, 1, None, 1, P(lz), None, None, None), (0, 0, 1, 1, None, 0, P(lz), None, None, P(mean)),
              (0, 0, 1, 2, None, 0, P(lz), None, None, None)):
        assert call(*a) == _lib.ERR_ARG, a
    one = lambda *a: c.lib.dh_merged_realization(c.handle, *a)  # noqa: E731
    for a in ((0, 0, 1, None, 0, 0, 1, P(lz)), (0, 0, 1, None, 4, 0, 1, P(lz)), (0, -1, 1, None, 3, 0, 1, P(lz)),
              (0, 0, 1, None, 3, -1, 1, P(lz)), (0, 0, 1, None, 3, M - 1, 2, P(lz)), (0, 0, 1, None, 3, M + 1, 0, P(lz))):
        assert one(*a) == _lib.ERR_ARG, a
    assert one(0, 0, 1, None, 3, M, 0, P(lz)) == 0
    for bad in (dict(nreal=0), dict(nreal=2, jitter=False), dict(nreal=1, first=-1), dict(nreal=1, seed=2 ** 64)):
        with pytest.raises(ValueError):
            d.logz_realizations(**bad)
    for bad in (dict(field="logzerr"), dict(field="logz", real=-1), dict(field="logz", first=M - 1, count=2)):
        with pytest.raises(ValueError):
            d.realization(**bad)
    assert d.field("logl").shape == (M,)  # still there
    d.release()
    with pytest.raises(ValueError):
        d.logz_realizations(1)


def test_logz_error_of_a_kept_ensemble(ctx):
    """tests/test_gpu_merge_kept.py's C1 shape: the realizations' mean against the summary's ln Z."""
    prob = inputs.problem("C1")
    r = ctx.ns_ensemble(prob, 4, 100, 16, want_samples=False, keep=True, walks=23, bound="single", entropy=[5, 9],
                        dlogz=0.1, max_iter=8000)
    assert (r["status"] == 0).all()
    try:
        d = ctx.merge_kept(prob)
    finally:
        ctx.release_kept()
    nreal = 256
    mean, sd = d.logz_error(nreal)
    s = d.summary
    print(f"[merge errors] kept C1: ln Z {s['logz']:.4f}, logzerr {s['logzerr']:.4f}; realizations {mean:.4f} +- {sd:.4f}")
    assert abs(mean - s["logz"]) <= 4 * sd / np.sqrt(nreal) + s["logzerr"] / np.sqrt(nreal)
