"""The strand bootstrap of the merged run on the device (csrc/merge_errors.hip, dh_merged_bootstrap / dh_merged_bootstrap_run;
DESIGN.md section 3.8.3): the device against the host form for the same (seed, b); against the reference's
utils.resample_run with its own draws injected (tests/golden/merge_bootstrap.npz); a bootstrap bit-identical alone and in
any batch; the extremes of given multiplicities; the realizations of section 3.8.2 unchanged by bootstrap calls.
Bounds: tests/merge_bootstrap_ref.py.  Worst measured error / bound per field is recorded in DESIGN.md section 3.8.3."""
import os

import numpy as np
import pytest

import bootstrap_cases as bc
import inputs
import merge_bootstrap_ref as br
from test_gpu_merge import problem_for
from test_merge_bootstrap_cpu import check_against_reference

pytestmark = pytest.mark.gpu

BOOTS = (0, 1, 2 ** 32 + 5)
FLOATS = ("logvol", "logwt", "logz")


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(bc.GOLD, "merge_bootstrap.npz")), np.load(os.path.join(bc.GOLD, "merge.npz"))


def merge_case(ctx, name, fix):
    if name == "golden":
        return ctx.merge_runs(inputs.problem("C1"), **bc.golden_args(fix[1]))
    args = bc.cases()[name]
    return ctx.merge_runs(problem_for(args["live_u"].shape[2]), **args)


@pytest.mark.parametrize("name", bc.NAMES + ("e_large",))
def test_device_against_host_form(ctx, fix, name):
    """The integers equal; every float a float64 evaluation of one exact value, each within its own chains' bound."""
    d = merge_case(ctx, name, fix)
    m = d.to_merged_run()
    for jitter in (False, True):
        for b in BOOTS:
            host = m._err_bootstrap_run(77, b, jitter, None)
            dev = d._err_bootstrap_run(77, b, jitter, None)
            np.testing.assert_array_equal(dev["idx"], host["idx"])
            np.testing.assert_array_equal(dev["samples_n"], host["samples_n"])
            assert dev["idx"].dtype == np.int64 and dev["samples_n"].dtype == np.int32
            h = br.hp(m, host["idx"], host["samples_n"], 77, b, jitter)
            bd, bh = br.bounds(h, br.device_chains(h["M"])), br.bounds(h, br.host_chains(h["M"]))
            label = f"device {name} b={b} jitter={int(jitter)}"
            for k in FLOATS:
                br.check(dev[k], h[k], bd[k], f"{label} {k}")
                br.check(dev[k], host[k], bd[k] + bh[k], f"{label} {k} vs host")
            one = d.bootstrap_realizations(1, 77, b, jitter, means=True)
            ho = m.bootstrap_realizations(1, 77, b, jitter, means=True)
            assert one["npoints"][0] == ho["npoints"][0] == len(host["idx"])
            for k, bk in (("logz", "logz_last"), ("information", "information"), ("ess", "ess"), ("mean", "mean")):
                assert np.isfinite(one[k]).all()
                br.check(one[k][0], h["logz"][-1] if k == "logz" else h[k], bd[bk], f"{label} batch {k}")
                br.check(one[k][0], ho[k][0], bd[bk] + bh[bk], f"{label} batch {k} vs host")


@pytest.mark.parametrize("name", bc.NAMES)
def test_device_with_the_references_draws(ctx, fix, name):
    d = merge_case(ctx, name, fix)
    m = d.to_merged_run()
    key, S = bc.strands(m)
    for i in range(bc.NCALLS):
        p = f"{name}/{i}/"
        mult = bc.multiplicities(fix[0][p + "draws"], S)
        got = d.resample_run(mult=mult)
        lz, h, _, _, npts = d._err_bootstrap(0, 0, 1, False, mult, False)
        assert npts[0] == len(got["idx"])
        check_against_reference(got, (lz, h), m, fix[0], p, mult, key, f"device {name} call {i}", br.device_chains)


@pytest.mark.parametrize("name", ["e_large", "h_bigplateau"])
def test_batch_equals_single_bit_for_bit(ctx, fix, name):
    d = merge_case(ctx, name, fix)
    for jitter in (False, True):
        single = [d.bootstrap_realizations(1, 9, 7 + i, jitter, means=True) for i in range(65)]
        assert len({int(s["npoints"][0]) for s in single}) > 1
        for nboot in (1, 3, 65):
            a = d.bootstrap_realizations(nboot, 9, 7, jitter, means=True)
            plain = d.bootstrap_realizations(nboot, 9, 7, jitter)
            for k in a:
                np.testing.assert_array_equal(a[k], np.concatenate([s[k] for s in single[:nboot]]), err_msg=f"{k} nboot={nboot}")
                if k != "mean":
                    np.testing.assert_array_equal(a[k], plain[k], err_msg=f"{k} without means")
        off = d.bootstrap_realizations(3, 9, 7 + 5, jitter, means=True)  # at another position of a batch
        for k in off:
            np.testing.assert_array_equal(off[k], np.concatenate([s[k] for s in single[5:8]]), err_msg=k)


def test_given_multiplicities_at_their_extremes(fix):
    from dynesty_amd import _lib
    c = _lib.Context(0)
    d = merge_case(c, "e_large", fix)
    m = d.to_merged_run()
    key, S = bc.strands(m)
    M = d.niter
    # all ones: the merged run itself
    r = d.resample_run(mult=np.ones(S, dtype=np.int64))
    np.testing.assert_array_equal(r["idx"], np.arange(M))
    np.testing.assert_array_equal(r["samples_n"], m.samples_n)
    np.testing.assert_array_equal(r["logvol"], d.realization("logvol", jitter=False))  # the same scan of the same steps
    # all S draws on one strand: each of its points S times (above the call's first carve: the arena grows)
    u = int(np.argmax(np.bincount(key, minlength=S)))
    one = np.zeros(S, dtype=np.int64)
    one[u] = S
    pts = np.flatnonzero(key == u)
    assert len(pts) * S > M + M // 4 + 2048
    r = d.resample_run(mult=one)
    hr = m.resample_run(mult=one)
    np.testing.assert_array_equal(r["idx"], np.repeat(pts, S))
    np.testing.assert_array_equal(r["samples_n"], hr["samples_n"])
    assert r["samples_n"][0] == S and r["samples_n"][-1] == 1
    h = br.hp(m, hr["idx"], hr["samples_n"], 0, 0, False)
    bd = br.bounds(h, br.device_chains(h["M"]))
    for k in FLOATS:
        br.check(r[k], h[k], bd[k], f"device one strand {k}")
    lz = d._err_bootstrap(0, 0, 1, False, one, True)
    br.check(lz[0], h["logz"][-1], bd["logz_last"], "device one strand ln Z")
    br.check(lz[3][0], h["mean"], bd["mean"], "device one strand mean")
    # M' >= 2^31: refused at the scan's total, the merged run and the context as they were
    big = np.zeros(S, dtype=np.int64)
    big[u] = 2 ** 31 - 1
    before = d.logz_realizations(2, 5, means=True)
    P = _lib._ptr
    out, npts = np.empty(1), np.zeros(1, dtype=np.int64)
    b32 = big.astype(np.int32)
    assert c.lib.dh_merged_bootstrap(c.handle, 0, 0, 1, 0, P(b32), 0, P(out), None, None, None, P(npts)) == _lib.ERR_ARG
    assert c.lib.dh_merged_bootstrap_run(c.handle, 0, 0, 0, P(b32), 16, 0, 0, None, P(npts)) == _lib.ERR_ARG
    with pytest.raises(ValueError, match="points"):
        d.resample_run(mult=big)
    zero = np.zeros(S, dtype=np.int32)
    assert c.lib.dh_merged_bootstrap(c.handle, 0, 0, 1, 0, P(zero), 0, P(out), None, None, None, None) == _lib.ERR_ARG
    after = d.logz_realizations(2, 5, means=True)
    for k in before:
        np.testing.assert_array_equal(before[k], after[k])


def test_argument_rules(fix):
    from dynesty_amd import _lib
    c = _lib.Context(0)
    P = _lib._ptr
    lz, mean, npts = np.empty(4), np.empty((4, 3)), np.zeros(4, dtype=np.int64)
    boot = lambda *a: c.lib.dh_merged_bootstrap(c.handle, *a)  # noqa: E731
    run = lambda *a: c.lib.dh_merged_bootstrap_run(c.handle, *a)  # noqa: E731
    assert boot(0, 0, 1, 0, None, 0, P(lz), None, None, None, None) == _lib.ERR_ARG  # no merged run
    assert run(0, 0, 0, None, 16, 0, 0, None, P(npts)) == _lib.ERR_ARG
    a = dict(bc.cases()["d_single"])
    bare = c.merge_runs(problem_for(3), **{k: v for k, v in a.items() if k not in ("dead_id", "dead_it", "dead_nc", "live_it")})
    assert boot(0, 0, 1, 0, None, 0, P(lz), None, None, None, None) == _lib.ERR_ARG  # a merge without id / it / nc
    with pytest.raises(ValueError, match="id / it / nc"):
        bare.bootstrap_realizations(1)
    with pytest.raises(ValueError, match="id / it / nc"):
        bare.resample_run()
    d = merge_case(c, "golden", fix)
    S = 180
    ones, neg = np.ones(S, dtype=np.int32), np.ones(S, dtype=np.int32)
    neg[7] = -1
    assert boot(0, 0, 1, 0, None, 0, P(lz), None, None, None, P(npts)) == 0 and npts[0] > 0
    for args in ((0, 0, 0, 0, None, 0, P(lz), None, None, None, None), (0, 0, 65537, 0, None, 0, P(lz), None, None, None, None),
                 (0, -1, 1, 0, None, 0, P(lz), None, None, None, None), (0, 0, 1, 2, None, 0, P(lz), None, None, None, None),
                 (0, 0, 2, 0, P(ones), 0, P(lz), None, None, None, None), (0, 0, 1, 0, P(neg), 0, P(lz), None, None, None, None),
                 (0, 0, 1, 0, None, 1, P(lz), None, None, None, None), (0, 0, 1, 0, None, 0, P(lz), None, None, P(mean), None),
                 (0, 0, 1, 0, None, 0, None, None, None, None, None)):
        assert boot(*args) == _lib.ERR_ARG, args
    Mx = int(npts[0])
    assert run(0, 0, 0, None, 16, 0, 0, None, P(npts)) == 0 and npts[0] == Mx
    for args in ((0, -1, 0, None, 16, 0, 0, None, None), (0, 0, 2, None, 16, 0, 0, None, None), (0, 0, 0, None, 0, 0, 0, None, None),
                 (0, 0, 0, None, 12, 0, 0, None, None), (0, 0, 0, None, 3, -1, 1, P(lz), None), (0, 0, 0, None, 3, Mx - 1, 2, P(lz), None),
                 (0, 0, 0, None, 3, Mx + 1, 0, P(lz), None), (0, 0, 0, None, 3, 0, 1, None, None), (0, 0, 0, P(neg), 3, 0, 1, P(lz), None)):
        assert run(*args) == _lib.ERR_ARG, args
    assert run(0, 0, 0, None, 3, Mx, 0, None, None) == 0
    assert run(0, 0, 0, None, 3, Mx - 1, 1, P(lz), None) == 0
    assert lz[0] == d.resample_run()["logz"][-1]
    for bad in (dict(nboot=0), dict(nboot=65537), dict(nboot=1, first=-1), dict(nboot=1, seed=2 ** 64)):
        with pytest.raises(ValueError):
            d.bootstrap_realizations(**bad)
    for mult in (ones[:-1], neg, ones.astype(np.float64)):
        with pytest.raises(ValueError):
            d.resample_run(mult=mult)
    with pytest.raises(ValueError):
        d._err_bootstrap(0, 0, 2, False, ones, False)
    assert d.field("logl").shape == (d.niter,)  # still there
    d.release()
    with pytest.raises(ValueError):
        d.bootstrap_realizations(1)


def test_realizations_unchanged_by_bootstrap_calls(ctx, fix):
    """dh_merged_realize and dh_merged_realization before and after bootstrap calls on the same context: the merged run
    is untouched and the unmapped integrals are what they were."""
    d = merge_case(ctx, "e_large", fix)
    before = d.logz_realizations(5, 31, 2, means=True)
    fields = {k: d.realization(k, 31, 3) for k in FLOATS}
    logl, n = d.field("logl"), d.field("samples_n")
    d.bootstrap_realizations(3, 31, 2, jitter=True, means=True)
    d.resample_run(31, 4)
    after = d.logz_realizations(5, 31, 2, means=True)
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    for k in FLOATS:
        np.testing.assert_array_equal(fields[k], d.realization(k, 31, 3), err_msg=k)
    np.testing.assert_array_equal(logl, d.field("logl"))
    np.testing.assert_array_equal(n, d.field("samples_n"))


def test_reference_gates_on_device_output(ctx, fix):
    d = merge_case(ctx, "golden", fix)
    res = d.bootstrap_realizations(2000, seed=1234)["logz"]
    br.gates(res, fix[0]["golden/resample/logz"], "device resample_run")
    sim = d.bootstrap_realizations(2000, seed=1234, jitter=True)["logz"]
    br.gates(sim, fix[0]["golden/simulate/logz"], "device simulate_run")
    mean, sd = d.logz_error_sampling(2000, seed=1234)
    assert mean == res.mean() and sd == res.std(ddof=1)
    ts = d.logz_error_total(2000, seed=1234)
    print(f"[merge bootstrap] device golden: ln Z = {mean:.4f} +- {sd:.4f} (sampling), +- {ts[1]:.4f} (total), "
          f"+- {d.logz_error(2000, seed=1234)[1]:.4f} (jitter alone); the summary's logzerr {d.summary['logzerr']:.4f}")
