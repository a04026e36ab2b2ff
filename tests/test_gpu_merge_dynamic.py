"""Run-level analysis of the merged run on the device (csrc/merge_errors.hip: dh_merged_kld, the KLD field of
dh_merged_realization / dh_merged_bootstrap_run, dh_merged_weight_function, dh_merged_weights):
the device against the long-double restatement (tests/merge_dynamic_ref.py), the host form and the reference's records
(tests/golden/merge_dynamic.npz); a divergence bit-identical alone and in any batch; the existing calls unchanged.
Every test prints its worst error / bound; the table is in DESIGN.md section 3.8.4."""
import os

import numpy as np
import pytest

import bootstrap_cases as bc
import inputs
import merge_cases
import merge_dynamic_ref as dr
from test_gpu_merge import problem_for
from test_merge_dynamic_cpu import (MODES, check_argument_rules, check_modes, check_resample_against_reference,
                                    check_stopping, check_weight_grid, check_weights, degenerate_args, distribution_gates)

pytestmark = pytest.mark.gpu

INDICES = (0, 1, 2 ** 32 + 5)
CASES = ("golden", "b_plateau", "c_ragged", "d_single", "e_large", "g_span", "h_bigplateau", "i_endties")


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def fix():
    return (np.load(os.path.join(bc.GOLD, "merge_dynamic.npz")), np.load(os.path.join(bc.GOLD, "merge_bootstrap.npz")),
            np.load(os.path.join(bc.GOLD, "merge.npz")))


def merge_case(ctx, name, fix):
    if name == "golden":
        return ctx.merge_runs(inputs.problem("C1"), **bc.golden_args(fix[2]))
    args = bc.cases()[name]
    return ctx.merge_runs(problem_for(args["live_u"].shape[2]), **args)


@pytest.mark.parametrize("name", CASES)
def test_batch_and_cumulative_against_restatement(ctx, fix, name):
    d = merge_case(ctx, name, fix)
    m = d.to_merged_run()
    worst = check_modes(d, m, name, dr.device_chains, INDICES, f"device {name}")
    print(f"[merge dynamic device {name}] worst error / bound: batch {worst['batch']:.3g}, cumulative {worst['cum']:.3g}")


@pytest.mark.parametrize("name", ["golden", "e_large", "h_bigplateau"])
def test_device_against_host_form(ctx, fix, name):
    """Both are float64 evaluations of one exact value: they differ by at most the sum of their bounds."""
    d = merge_case(ctx, name, fix)
    m = d.to_merged_run()
    worst = 0.0
    for mode in MODES:
        for index in INDICES[::2]:
            idx, n = dr.sequence(m, mode, 77, index)
            h = dr.kld_hp(m, idx, n, 77, index, mode != "resample")
            bd, bh = dr.kld_bounds(h, dr.device_chains(h["M"])), dr.kld_bounds(h, dr.host_chains(h["M"]))
            lab = f"device {name} {mode} {index} vs host"
            worst = max(worst, dr.check(d.kld_error(77, index, mode), m.kld_error(77, index, mode), bd["cum"] + bh["cum"], lab))
            dev, host = d.kld_realizations(1, 77, index, mode), m.kld_realizations(1, 77, index, mode)
            worst = max(worst, dr.check(dev["kld"], host["kld"], bd["batch"] + bh["batch"], lab + " batch"))
    print(f"[merge dynamic device {name}] worst error / bound against the host form {worst:.3g}")


@pytest.mark.parametrize("name", ["e_large"])
def test_batch_equals_single_bit_for_bit(ctx, fix, name):
    d = merge_case(ctx, name, fix)
    for mode in MODES:
        nmax = 130 if mode == "jitter" else 65
        single = [d.kld_realizations(1, 9, 7 + i, mode) for i in range(nmax)]
        for n in (1, 3, 64, 65, 130):
            if n > nmax:
                continue
            a = d.kld_realizations(n, 9, 7, mode)
            for k in a:
                np.testing.assert_array_equal(a[k], np.concatenate([s[k] for s in single[:n]]), err_msg=f"{mode} {k} n={n}")
        off = d.kld_realizations(3, 9, 7 + 5, mode)  # at another position of a batch
        for k in off:
            np.testing.assert_array_equal(off[k], np.concatenate([s[k] for s in single[5:8]]), err_msg=f"{mode} {k}")


def test_existing_calls_are_unchanged(ctx, fix):
    """logz_realizations and bootstrap_realizations before and after the new entry points."""
    d = merge_case(ctx, "e_large", fix)
    before = (d.logz_realizations(66, 3, 5, means=True), d.bootstrap_realizations(5, 3, 5, means=True),
              d.bootstrap_realizations(3, 3, 2, jitter=True))
    for mode in MODES:
        d.kld_realizations(5, 3, 5, mode)
        d.kld_error(3, 5, mode, first=10, count=4)
    d.weight_function()
    d.weights(0.8, "weight", 0, 10)
    after = (d.logz_realizations(66, 3, 5, means=True), d.bootstrap_realizations(5, 3, 5, means=True),
             d.bootstrap_realizations(3, 3, 2, jitter=True))
    for a, b in zip(before, after):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    lz = d.kld_realizations(66, 3, 5)["logz"]
    np.testing.assert_array_equal(lz, before[0]["logz"])  # (the divergence's ln Z is the realizations' own, bit for bit)
    np.testing.assert_array_equal(d.kld_realizations(5, 3, 5, "resample")["logz"], before[1]["logz"])


def test_cumulative_field_across_carry_blocks(ctx):
    """More than 256 chunks: the carry stage of the divergence's scan loops."""
    args = merge_cases.make(np.random.default_rng(21), [140000] * 4, 100, 2)
    d = ctx.merge_runs(problem_for(2), **args)
    M = d.niter
    nblk = -(-M // 2048)
    assert nblk > 256
    edges = [c * 256 * 2048 for c in range(1, -(-nblk // 256))]
    ks = sorted(set([0, 1, 2047, 2048, M - 2, M - 1] + [e + o for e in edges for o in (-2049, -2048, -1, 0, 1, 2047, 2048)]))
    ks += [int(k) for k in np.linspace(3, M - 3, 64 - len(ks)).astype(int)]
    ks = np.array(sorted(set(ks)))
    assert len(ks) >= 60 and all(e - 1 in ks and e in ks for e in edges)
    m = dict(logl=d.field("logl"), samples_n=d.field("samples_n"), logwt=d.field("logwt"), logz=d.field("logz"))
    h = dr.kld_hp(m, np.arange(M), m["samples_n"], 5, 1, True)
    b = dr.kld_bounds(h, dr.device_chains(M))
    got = d.kld_error(5, 1)
    worst = dr.check(got[ks], h["kld_cum"][ks], b["cum"][ks], "device carry cumulative")
    one = d.kld_realizations(1, 5, 1)
    worst = max(worst, dr.check(one["kld"], h["kld"], b["batch"], "device carry batch"))
    dr.check(got[-1], one["kld"][0], b["cum"][-1] + b["batch"], "device carry cumulative against batch")
    print(f"[merge dynamic device carry] worst error / bound {worst:.3g}")


@pytest.mark.parametrize("name", bc.NAMES)
def test_resample_divergence_with_the_references_draws(ctx, fix, name):
    d = merge_case(ctx, name, fix)
    worst = check_resample_against_reference(d, d.to_merged_run(), fix, name, dr.device_chains, f"device {name}")
    print(f"[merge dynamic device {name}] worst error / bound with the reference's draws {worst:.3g}")


def test_distributions_against_reference(ctx, fix):
    distribution_gates(merge_case(ctx, "golden", fix), fix, "device")


@pytest.mark.parametrize("name", bc.NAMES)
def test_weight_function_against_reference(ctx, fix, name):
    d = merge_case(ctx, name, fix)
    m = d.to_merged_run()
    chain = dr.device_chains(d.niter)["scan"]
    check_weight_grid(d, m, fix, name, chain, f"device {name}")
    worst = check_weights(d._err_weights(0.8), m, fix, name, chain, f"device {name}")
    w = d.weights(0.8, "zweight")
    np.testing.assert_array_equal(d.weights(0.8, "zweight", 7, 9), w[7:16])
    np.testing.assert_array_equal(d.weights(0.3, "pweight"), d.field("weights"))
    print(f"[merge dynamic device {name}] worst error / bound of the weights {worst:.3g}")


def test_stopping_function(ctx, fix):
    check_stopping(merge_case(ctx, "golden", fix), fix, "device")


def test_degenerate_run_has_equal_zweights(ctx):
    d = ctx.merge_runs(problem_for(2), **degenerate_args())
    assert d.field("logz", 0, 1)[0] == d.field("logz", d.niter - 1, 1)[0]
    (lo, hi), (pw, zw, w) = d.weight_function(pfrac=0.0, return_weights=True)
    np.testing.assert_array_equal(zw, np.full(d.niter, 1.0 / d.niter))
    np.testing.assert_array_equal(w, zw)
    assert (lo, hi) == (-np.inf, np.inf)


def test_argument_errors_leave_the_merged_run(fix):
    from dynesty_amd import _lib
    c = _lib.Context(0)
    P = _lib._ptr
    out, b2, i2 = np.empty(4), np.empty(2), np.empty(2, dtype=np.int64)
    assert c.lib.dh_merged_kld(c.handle, 0, 0, 1, 0, None, P(out), None, None) == _lib.ERR_ARG  # no merged run
    assert c.lib.dh_merged_weight_function(c.handle, 0.8, 0.8, 1, P(b2), P(i2)) == _lib.ERR_ARG
    assert c.lib.dh_merged_weights(c.handle, 0.8, 2, 0, 1, P(out)) == _lib.ERR_ARG
    d = merge_case(c, "golden", fix)
    before = d.kld_realizations(3, 5)
    check_argument_rules(d)
    mult = np.ones(int(d.field("samples_n", 0, 1)[0]), dtype=np.int32)
    rwt = np.zeros(d.niter)
    for rc in (c.lib.dh_merged_kld(c.handle, 0, 0, 0, 0, None, P(out), None, None),
               c.lib.dh_merged_kld(c.handle, 0, 0, 65537, 0, None, P(out), None, None),
               c.lib.dh_merged_kld(c.handle, 0, -1, 1, 0, None, P(out), None, None),
               c.lib.dh_merged_kld(c.handle, 0, 0, 1, 3, None, P(out), None, None),
               c.lib.dh_merged_kld(c.handle, 0, 0, 1, 0, None, None, None, None),
               c.lib.dh_merged_kld(c.handle, 0, 0, 1, 0, P(mult), P(out), None, None),
               c.lib.dh_merged_kld(c.handle, 0, 0, 2, 1, P(mult), P(out), None, None),
               c.lib.dh_merged_fetch(c.handle, 17, 0, 1, P(out)),
               c.lib.dh_merged_realization(c.handle, 0, 0, 1, P(rwt), 17, 0, 1, P(out)),
               c.lib.dh_merged_weight_function(c.handle, np.nan, 0.8, 1, P(b2), P(i2)),
               c.lib.dh_merged_weight_function(c.handle, 0.8, 1.5, 1, P(b2), P(i2)),
               c.lib.dh_merged_weight_function(c.handle, 0.8, 0.8, -1, P(b2), P(i2)),
               c.lib.dh_merged_weight_function(c.handle, 0.8, 0.8, 1, None, P(i2)),
               c.lib.dh_merged_weights(c.handle, 1.5, 2, 0, 1, P(out)),
               c.lib.dh_merged_weights(c.handle, 0.8, 3, 0, 1, P(out)),
               c.lib.dh_merged_weights(c.handle, 0.8, 2, d.niter, 1, P(out))):
        assert rc == _lib.ERR_ARG
    assert c.lib.dh_merged_kld(c.handle, 0, 0, 1, 1, P(mult), P(out), None, None) == 0  # (all ones: the run itself)
    assert abs(out[0]) < 1e-10
    after = d.kld_realizations(3, 5)
    for k in before:
        np.testing.assert_array_equal(before[k], after[k])
