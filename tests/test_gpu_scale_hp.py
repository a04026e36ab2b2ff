"""scale_logvol_kernel held to the reference of tests/scale_hp_ref.py at its derived bounds, through its three entry
points: dh_scale_to_logvol on every case of tests/scale_cases.py (all five outputs), and the batched launch shapes --
dh_enlarge_batch_dev and the diagnostic entry dh_enlarge_runs with the run mask and the per-run shift the resident loop
alone used to reach -- which must return, bit for bit, what dh_scale_to_logvol returns for the same ellipsoid and
target on every live slot, and everything else as it was sent.

tests/test_scale_hp_cpu.py shows without a device that the float64 oracles pass the same checks and that evaluations
with one defect each do not.  Every test prints its error / bound."""
import math

import numpy as np
import pytest

import scale_cases as C
import scale_hp_ref as H

pytestmark = pytest.mark.gpu
NAMES = ("covs", "ams", "axess", "axlenss", "logvols")


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def scale(ctx, covs, ams, axes, axlens, logvols, targets):
    """dh_scale_to_logvol on copies: the five arrays that came back."""
    arrs = [np.array(a, dtype=np.float64, order="C") for a in (covs, ams, axes, axlens, logvols)]
    ctx.scale_to_logvol(*arrs, np.asarray(targets, dtype=np.float64))
    return arrs


@pytest.mark.parametrize("family,d", C.CASES)
def test_scale_to_logvol(ctx, family, d):
    c = C.case(family, d)
    got = scale(ctx, *(c[n] for n in NAMES), c["targets"])
    worst = C.check(c, dict(zip(H.FIELDS, got)), "dh_scale_to_logvol")
    print(f"scale_hp WORST dh_scale_to_logvol {family} D={d}: " + "  ".join(f"{n} {worst[n]:.3g}" for n in H.FIELDS))
    for n in H.FIELDS:
        assert worst[n] <= 1.0, (c["name"], n, worst[n])


@pytest.mark.parametrize("name", C.CLOUDS)
def test_golden_clouds(ctx, name):
    """The inputs of test_gpu_small_kernels' anisotropic cases (flat10 among them) at the derived bounds."""
    c = C.cloud_case(name)
    got = scale(ctx, *(c[n] for n in NAMES), c["targets"])
    worst = C.check(c, dict(zip(H.FIELDS, got)), "dh_scale_to_logvol")
    print(f"scale_hp WORST dh_scale_to_logvol cloud {name}: " + "  ".join(f"{n} {worst[n]:.3g}" for n in H.FIELDS))
    for n in H.FIELDS:
        assert worst[n] <= 1.0, (c["name"], n, worst[n])


# ---- the batched launch shapes ------------------------------------------------------------------------------------------
RUNS = 5
PAD = 7.25


def pool(d):
    """The ellipsoids the slots are filled from: both branches, capped axes, axis ratios up to 1e6."""
    cs = [C.inputs(f, d) for f in ("enlarge", "capped", "kappa")]
    return [np.concatenate([c[n] for c in cs]) for n in NAMES]


def layout(d, me):
    """RUNS x me slots; run r holds nells[r] ellipsoids of the pool, every other slot the padding value."""
    nells = np.array([me, 1, 0, me, 1], dtype=np.int32)
    src = pool(d)
    arrs = [np.full((RUNS, me) + a.shape[1:], PAD) for a in src]
    which = np.full((RUNS, me), -1)
    t = 0
    for r in range(RUNS):
        for s in range(nells[r]):
            which[r, s] = t % len(src[0])
            for a, b in zip(arrs, src):
                a[r, s] = b[which[r, s]]
            t += 1
    return arrs, nells, which


def expected(ctx, arrs, nells, shift, active, run_shift):
    """What the launch must return: dh_scale_to_logvol's outputs on the live slots, targets added up as the kernel
    states them ((logvol + run_shift) + shift), everything else as sent.  Returns (arrays, live mask, targets)."""
    me = arrs[0].shape[1]
    live = np.arange(me)[None, :] < nells[:, None]
    if active is not None:
        live &= np.asarray(active, dtype=bool)[:, None]
    if run_shift is not None and shift == 0.0:
        live &= (np.asarray(run_shift) != 0.0)[:, None]
    rs = np.zeros(RUNS) if run_shift is None else np.asarray(run_shift, dtype=np.float64)
    targets = (arrs[4] + rs[:, None]) + shift
    want = [a.copy() for a in arrs]
    if live.any():
        for w, o in zip(want, scale(ctx, *(a[live] for a in arrs), targets[live])):
            w[live] = o
    return want, live, targets


def same(got, want, what):
    for n, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), f"{what}: {n} differs in {int(np.sum(g != w))} element(s), first at {tuple(np.argwhere(g != w)[0])}"


@pytest.mark.parametrize("me", (1, 3, 4, 5, 9))
@pytest.mark.parametrize("d", (5, 25, 45, 65))
def test_batched_forms_equal_the_single_entry(ctx, d, me):
    """G = min(max_ells, 4) workgroups per run, each striding the slots: every live slot bit for bit what
    dh_scale_to_logvol gives, and every slot past nells, every inactive run and every zero-shift run as sent (padding
    included)."""
    arrs, nells, _ = layout(d, me)
    ln125 = math.log(1.25)
    rs = np.array([d * math.log(1.5), d * math.log(1.05), d * math.log(1.5), 0.0, d * math.log(1.05)])
    # dh_enlarge_batch_dev on device arrays
    d_n = ctx.to_device(nells)
    dev = [ctx.to_device(a) for a in arrs]
    ctx._check(ctx.lib.dh_enlarge_batch_dev(ctx.handle, RUNS, me, d_n, d, *dev, ln125))
    ctx.sync()
    got = [ctx.from_device(p, a.shape, np.float64) for p, a in zip(dev, arrs)]
    for p in dev + [d_n]:
        ctx.free(p)
    want, live, _ = expected(ctx, arrs, nells, ln125, None, None)
    assert live.sum() == nells.sum()
    same(got, want, f"dh_enlarge_batch_dev d={d} max_ells={me}")
    # dh_enlarge_runs: (log_enlarge, active, run_shift)
    forms = (("plain", ln125, None, None), ("active", ln125, [1, 1, 1, 0, 1], None), ("run_shift", 0.0, None, rs),
             ("both shifts", ln125, None, rs), ("active + run_shift", 0.0, [1, 0, 1, 1, 1], rs),
             ("nothing to do", 0.0, None, np.zeros(RUNS)))
    for what, shift, active, run_shift in forms:
        got = [a.copy() for a in arrs]
        ctx.enlarge_runs(*got, nells, shift, active=active, run_shift=run_shift)
        want, live, targets = expected(ctx, arrs, nells, shift, active, run_shift)
        same(got, want, f"dh_enlarge_runs [{what}] d={d} max_ells={me}")
        if what == "run_shift":
            assert not live[3].any() and live[0].all()  # the zero-shift run holds max_ells live ellipsoids and is left alone
        if what == "nothing to do":
            assert not live.any()
        if what == "both shifts" and me == 9:
            # one function, two launch shapes: the live slots lie inside the reference's bounds too
            worst = dict.fromkeys(H.FIELDS, 0.0)
            for r, s in np.argwhere(live):
                val, bnd, sc = H.reference(*(a[r, s] for a in arrs), targets[r, s])
                assert sc["decided"]
                ratio = H.ratios({n: g[r, s] for n, g in zip(H.FIELDS, got)}, val, bnd)
                for n in H.FIELDS:
                    worst[n] = max(worst[n], ratio[n])
            print(f"scale_hp WORST dh_enlarge_runs [{what}] D={d} max_ells={me}: " +
                  "  ".join(f"{n} {worst[n]:.3g}" for n in H.FIELDS))
            for n in H.FIELDS:
                assert worst[n] <= 1.0, (d, me, n, worst[n])
    print(f"scale_hp batched d={d} max_ells={me}: dh_enlarge_batch_dev and {len(forms)} forms of dh_enlarge_runs equal "
          f"dh_scale_to_logvol bit for bit on the live slots and return everything else as sent")


def test_refuses_bad_arguments(ctx):
    """DH_ERR_ARG for a null required pointer, runs / max_ells / d < 1, d above the wide limit and an nells beyond
    max_ells; dh_scale_to_logvol refuses d > 512 too; the context serves a correct call afterwards."""
    from dynesty_amd import _lib
    d, me = 5, 3
    arrs, nells, _ = layout(d, me)
    keys = ("covs", "ams", "axes", "axlens", "logvols")

    def call(runs=RUNS, max_ells=me, d=d, nells=nells, **null):
        p = {k: (None if null.get(k) else _lib._ptr(a)) for k, a in zip(keys, arrs)}
        n = None if null.get("nells") else _lib._ptr(np.ascontiguousarray(nells, dtype=np.int32))
        return ctx.lib.dh_enlarge_runs(ctx.handle, runs, max_ells, n, d, p["covs"], p["ams"], p["axes"], p["axlens"],
                                       p["logvols"], 0.1, None, None)
    before = [a.copy() for a in arrs]
    for kw in ([{k: True} for k in keys + ("nells",)] +
               [dict(runs=0), dict(max_ells=0), dict(d=0), dict(d=513), dict(nells=[me + 1, 1, 0, me, 1]), dict(nells=[-1, 1, 0, me, 1])]):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert "enlarge_runs" in ctx.lib.dh_last_error(ctx.handle).decode()
    same(arrs, before, "a refused call")
    z = np.zeros(1)
    assert ctx.lib.dh_scale_to_logvol(ctx.handle, 1, 513, *(_lib._ptr(z),) * 6) == _lib.ERR_ARG
    assert "scale_to_logvol" in ctx.lib.dh_last_error(ctx.handle).decode()
    got = [a.copy() for a in arrs]
    ctx.enlarge_runs(*got, nells, 0.1)
    same(got, expected(ctx, arrs, nells, 0.1, None, None)[0], "the call after the refusals")
