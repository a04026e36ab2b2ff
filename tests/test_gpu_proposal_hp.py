"""The rwalk proposal kernels -- one walker per lane (csrc/walk.hip), four lanes per walker on the matrix cores
(csrc/walkq.hip), a wavefront per walker (csrc/wide.hip) and rwalk_propose -- held to the high-precision reference of
tests/proposal_hp_ref.py at its derived bounds, on the cases of tests/proposal_cases.py: every D = 2 ... 32 of the
four-lane form (its ur^(1/n) is a multiplication chain of its own per D), steps of 0.4, frames of axis ratio 1e3,
live sets of width 1e-7, periodic / reflective excursions of tens of units, step uniforms of exactly 0, 2^-53, 2^-30
and 1 - 2^-53, chains on the four fused problem kinds with the accumulated bound; and rslice / slice (slice_kernel,
wide_walk_kernel, slice_feed's directions) replayed around the high-precision F; and the draws inside ellipsoids
(unif_kernel, wide_unif_kernel, bound_draw_kernel) as one step from the centre.

No mpmath runs here: the radius over the norm of every one-step walker and the chains' end points come from
tests/golden/proposal_hp.npz (tools/make_golden.py proposal_hp); mat-vecs and sums are redone in long double.  One
step through rwalk_batch is walks = 1 with loglstar = -1e300: an in-cube proposal is what comes back, an out-of-cube one
returns u0 with reject = 1.  Every case prints error / bound; a test fails if any ratio is above 1.
tests/test_proposal_hp_cpu.py shows, without a device, that the float64 oracle passes the same checks and that a radius
wrong by 1e-13 does not.
"""
import numpy as np
import pytest

import proposal_cases as PC
import proposal_hp_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    c = _lib.Context(0)
    yield c
    c.set_rwalk_form(0)
    c.set_rwalk_items(True, 1 << 30)


@pytest.fixture(scope="module")
def fix():
    return H.load_fixture()


def _run(ctx, entry, inp):
    """The entry point / kernel form `entry` on one input set: what check_step and check_chain read."""
    if entry == "propose":
        up, inside, end = ctx.rwalk_propose(inp["u0"], inp["axes"], inp["scale"], inp["states"], axes_idx=inp["idx"],
                                            ncdim=inp["nc"], bc=inp["bc"])
        return dict(u=up, inside=inside, reject=None, end=end)
    ctx.set_rwalk_form(1 if entry == "lane" else 2)
    ctx.set_rwalk_items(entry != "quadf", 1 << 30)
    prob = PC.the_problem("prec", inp["d"]) if entry == "quadprec" else inp["problem"]
    out = ctx.rwalk_batch(prob, inp["u0"], inp["axes"], inp["scale"], inp["loglstar"], inp["walks"],
                          inp["states"], axes_idx=inp["idx"], ncdim=inp["nc"], bc=inp["bc"])
    assert np.array_equal(out["accept"] + out["reject"], np.full(inp["k"], inp["walks"]))
    assert np.all(np.isfinite(out["v"])) and np.all(np.isfinite(out["logl"]))
    out["end"] = out["rng_out"]
    if inp["walks"] == 1:
        out["inside"] = out["accept"] == 1
    return out


def _run_slice(ctx, inp):
    out = ctx.slice_batch(inp["problem"], inp["u0"], inp["axes"], inp["scale"], inp["loglstar"], inp["slices"],
                          inp["states"], principal=inp["principal"], doubling=inp["doubling"], axes_idx=inp["idx"])
    out["end"] = out["rng_out"]
    return out


def _groups(entries):
    """{(entry, d, nc, k): [keys]}: one test per entry point, form and dimension."""
    out = {}
    for entry, key in entries:
        p = key.split("/")
        out.setdefault((entry,) + ((int(p[1]), int(p[2]), int(p[3])) if p[0] == "step" else (int(p[1]),)), []).append(key)
    return out


STEP = _groups(PC.step_entries())
EDGE = _groups(PC.edge_entries())


def _finish(failures, worst, what):
    print(f"proposal_hp WORST {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not failures, f"{what}: error / bound above 1 in {len(failures)} case(s): {failures[:6]}"


def _one(ctx, fix, entry, keys, what, chain=False):
    failures, worst = [], H.Ratios()
    for key in keys:
        inp = H.inputs_of(key, fix)
        got = _run(ctx, entry, inp)
        if chain:
            r = H.check_chain(inp, fix[key], got, f"{entry} {key}")
        else:
            # the four-lane kernel's root is a Newton iteration: no pow, no exponent term in its bound
            r = H.check_step(inp, fix[key], got, f"{entry} {key}", propose=entry == "propose",
                             exponent=not entry.startswith("quad"))
        print(f"proposal_hp {entry} {key}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
        worst.merge(r)
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        if bad:
            failures.append((key, bad))
    _finish(failures, worst, what)


@pytest.mark.parametrize("case", sorted(STEP), ids=lambda c: "-".join(str(x) for x in c))
def test_one_step(ctx, fix, case):
    """u' = u + scale ur^(1/n) A z / |z|, wrapped and reflected, on the groups A (today's frames, steps of 0.4, axis
    ratio 1e3), B (width 1e-7, with axis ratio 1e3) and C (periodic / reflective excursions of tens of units), three
    frames inside every wavefront."""
    entry, d, nc, k = case
    _one(ctx, fix, entry, STEP[case], f"one step {entry} D={d} ncdim={nc} k={k}")


@pytest.mark.parametrize("case", sorted(EDGE), ids=lambda c: "-".join(str(x) for x in c))
def test_one_step_constructed_uniforms(ctx, fix, case):
    """Generator states built so that the step uniform is exactly 0 (u0 must come back bit for bit, everything finite:
    root_n passes through 0 * inf there), 2^-53, 2^-30 and 1 - 2^-53 (whose float is 1)."""
    entry, d = case
    _one(ctx, fix, entry, EDGE[case], f"constructed uniforms {entry} D={d}")


@pytest.mark.parametrize("entry,key", PC.chain_entries(), ids=lambda x: x.replace("/", "-") if isinstance(x, str) else x)
def test_chains(ctx, fix, entry, key):
    """Counts and generator end states exact, u within the accumulated bound of the accepted steps, ln L within
    hp_ref's bound at the device's own v; walkers with an undecidable decision (at most 2 % of a case) left out."""
    _one(ctx, fix, entry, [key], f"chain {entry} {key}", chain=True)


@pytest.mark.parametrize("key", PC.slice_keys(), ids=lambda x: x.replace("/", "-"))
def test_slices(ctx, fix, key):
    """rslice (random directions) and slice (principal axes) through slice_kernel, and wide_walk_kernel at D = 40:
    stepping out and doubling with the acceptance test, frames of axis ratio 1e3, directions longer than sqrt(n) / 2
    (renormalised), slices of width 1e-7.  ncalls, n_expand, n_contract, flags and generator end states exact, u
    within the bound of the accepted point, ln L within hp_ref's bound at the device's own v."""
    inp = H.inputs_of(key, fix)
    r = H.check_slice(inp, fix[key], _run_slice(ctx, inp), key)
    if key in PC.feed_keys():
        st6 = np.concatenate([inp["states"], np.zeros((inp["k"], 2), dtype=np.uint64)], axis=1)
        _, dirs, _ = ctx.slice_feed("direction", inp["d"], st6, axes=inp["axes"], axes_idx=inp["idx"], scale=inp["scale"])
        r.merge(H.check_feed(inp, fix[key], dirs, key))
    print(f"proposal_hp slice {key}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
    _finish([(key, dict(r))] if not all(v <= 1.0 for v in r.values()) else [], r, f"slice {key}")


@pytest.mark.parametrize("key", PC.draw_keys(), ids=lambda x: x.replace("/", "-"))
def test_draws_inside_ellipsoids(ctx, fix, key):
    """ctr + A (z ur^(1/n) / |z|) at the bound of one step from the centre: unif_batch (unif_kernel, wide_unif_kernel at
    D = 40) with one generator per walker, bound_draw with 83 draws off one generator, and bound_draw over three
    overlapping ellipsoids: idxs exact, q exact wherever every membership has a margin; unif_batch over the same three
    (rand_choice, the 1 / q acceptance loop): ncalls and generator end states exact, the kept point at the bound."""
    inp = H.inputs_of(key, fix)
    ones = np.ones(inp["k"], dtype=bool)
    if inp["kind"] == "unif":
        out = ctx.unif_batch(inp["problem"], inp["loglstar"], inp["states"], ctrs=inp["ctrs"], axes=inp["axes"])
        got = dict(u=out["u"], inside=out["ncalls"] == 1, end=out["rng_out"])
    elif inp["kind"] == "unifmulti":
        out = ctx.unif_batch(inp["problem"], inp["loglstar"], inp["start"], ctrs=inp["ctrs"], axes=inp["axes"],
                             ams=inp["ams"], logvol_ells=inp["logvol_ells"])
        np.testing.assert_array_equal(out["rng_out"], inp["end"])  # as many choices, draws and 1 / q uniforms as NumPy
        got = dict(u=out["u"], inside=out["ncalls"] == 1)
    else:
        multi = inp["kind"] == "multi"
        xs, idxs, qs, end = ctx.bound_draw(inp["state0"], inp["k"], inp["ctrs"], inp["axes"], inp["ams"] if multi else None,
                                           inp["logvol_ells"] if multi else None, return_q=multi)
        np.testing.assert_array_equal(idxs, inp["idx"])
        np.testing.assert_array_equal(end, H.draws(inp)[3][-1])
        if multi:
            print(f"proposal_hp {key}: decidable memberships {H.check_membership(inp, xs, qs, key):.3f}")
        got = dict(u=xs, inside=ones)
    r = H.check_step(inp, fix[key], got, key)
    print(f"proposal_hp draw {key}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
    _finish([(key, dict(r))] if not all(v <= 1.0 for v in r.values()) else [], r, f"draw {key}")
