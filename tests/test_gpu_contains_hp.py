"""The five ellipsoid membership kernels -- contains_kernel<N> and wide_contains_kernel behind dh_contains, and
contains_runs_kernel<N>, contains_runs_lds_kernel<N> and contains_runs_wide_kernel behind the diagnostic entry
dh_contains_runs -- held to the long-double reference of tests/contains_hp_ref.py at its derived bound, on the seeded
cases of tests/contains_cases.py: points in shells 64, 8 and 1/8 bounds either side of a boundary, ill-conditioned and
late-run precision matrices, every instantiation at its own d and one below the next, points with q == 1 exactly, a NaN
point, and whole run-wise launches with mixed nells, unused slots that contain everything, masked runs and preset words.

Every decidable pair is compared with the reference; the pairs of the +-B/8 shell are held to the quad bound and to the
kernels' self-consistency.  tests/test_contains_hp_cpu.py shows without a device that the float64 oracle passes the same
checks and that kernels with one defect each do not.  Every test prints its worst error / bound.
"""
import os

import numpy as np
import pytest

import contains_cases as C
import contains_hp_ref as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def hold_contains(ctx, x, ctrs, ams, q, bound, what):
    """dh_contains on (x, ctrs, ams) in both modes against q / bound: returns (worst quad error / bound, how near the
    boundary a verdict was compared)."""
    k = x.shape[0]
    worst = near = 0.0
    for mode in (0, 1):
        count, mask, quad = ctx.contains(x, ctrs, ams, mode=mode, want_mask=True, want_quad=True)
        worst = max(worst, H.check_quad(quad, q, bound))
        inside, beyond = H.unpack(mask, k)
        # every decidable pair: the reference's verdict, in the mask and (through the popcount below) in count
        near = max(near, H.check_verdicts(inside, q, bound, mode))
        # every pair, the undecidable ones included: the verdict is the one the device's own quad gives
        with np.errstate(invalid="ignore"):
            if mode == 0:
                assert same(inside, quad < 1), f"{what}: mask differs from quad < 1"
            else:  # (1, 1 + 4 * 2^-53]: a correctly rounded square root of such a quad may still be 1
                band = (quad > 1) & (quad <= 1 + 4 * H.U)
                assert same(inside[~band], (quad <= 1)[~band]), f"{what}: mask differs from quad <= 1"
        assert same(count, inside.sum(axis=1)), f"{what}: count is not the popcount of the mask rows"
        assert not beyond.any(), f"{what}: mask bits beyond k are set"
        for want_mask, want_quad in ((False, False), (True, False), (False, True)):
            count2, mask2, quad2 = ctx.contains(x, ctrs, ams, mode=mode, want_mask=want_mask, want_quad=want_quad)
            assert same(count2, count), f"{what}: count changes with want_mask={want_mask} want_quad={want_quad}"
            assert mask2 is None or same(mask2, mask), f"{what}: mask changes with want_quad={want_quad}"
            assert quad2 is None or same(quad2, quad), f"{what}: quad changes with want_mask={want_mask}"
    return worst, near


# ---- dh_contains ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,d", C.CONTAINS_NARROW)
def test_contains_narrow(ctx, family, d):
    """contains_kernel<N> at every N of DH_DIM_LIST and at the first d padded into the next."""
    c = C.case(family, d)
    worst, near = hold_contains(ctx, c["x"], c["ctrs"], c["ams"], c["q"], c["bound"], c["name"])
    print(f"contains_hp contains_kernel {c['name']}: quad error / bound {worst:.3g}  nearest verdict at bound / |q - 1| {near:.3g}")


@pytest.mark.parametrize("family,d", C.CONTAINS_WIDE)
def test_contains_wide(ctx, family, d):
    """wide_contains_kernel: a thread's rows, the tree; k is no multiple of 64, so the mask goes through the memset and
    the atomic or."""
    c = C.case(family, d)
    assert c["x"].shape[0] < 80 and c["x"].shape[0] % 64
    worst, near = hold_contains(ctx, c["x"], c["ctrs"], c["ams"], c["q"], c["bound"], c["name"])
    print(f"contains_hp wide_contains_kernel {c['name']}: quad error / bound {worst:.3g}  nearest verdict at bound / |q - 1| {near:.3g}")


@pytest.mark.parametrize("family,d", (("multi3", 5), ("multi3", 33)))
@pytest.mark.parametrize("k", (1, 63, 64, 65))
def test_contains_partial_mask_word(ctx, family, d, k):
    c = C.case(family, d)
    worst, near = hold_contains(ctx, c["x"][:k], c["ctrs"], c["ams"], c["q"][:k], c["bound"][:k], f"{c['name']} k={k}")
    print(f"contains_hp partial word {c['name']} k={k}: quad error / bound {worst:.3g}  nearest verdict {near:.3g}")


@pytest.mark.parametrize("d", C.NARROW_D + C.WIDE_D)
def test_contains_exact(ctx, d):
    """q == 1 exactly: the quad is 1.0, mode 0 says outside and mode 1 inside; one ulp either side falls on its side in
    both modes."""
    e = C.exact_case(d)
    worst, _ = hold_contains(ctx, e["x"], e["ctrs"], e["ams"], e["q"], e["bound"], e["name"])
    for mode, want in ((0, [0, 1, 0]), (1, [1, 1, 0])):
        count, _, quad = ctx.contains(e["x"], e["ctrs"], e["ams"], mode=mode, want_quad=True)
        assert quad[0, 0] == 1.0 and same(quad[:, 0], e["q"][:, 0].astype(np.float64))
        assert list(count) == want, (mode, list(count))
    print(f"contains_hp exact d={d}: quad error {worst:.3g} (exact)")


# ---- dh_contains_runs -------------------------------------------------------------------------------------------------
def launch(ctx, c, lds=None, with_first=True, flag=None, first=None):
    """One dh_contains_runs launch of a run-wise case; lds: the value of DH_CONTAINS_LDS for this launch."""
    old = os.environ.pop("DH_CONTAINS_LDS", None)
    if lds is not None:
        os.environ["DH_CONTAINS_LDS"] = lds
    try:
        first = (c["first"] if first is None else first) if with_first else None
        return ctx.contains_runs(c["x"], c["wpr"], c["ctrs"], c["ams"], nells=c["nells"], strict=c["strict"],
                                 run_mode=c.get("run_mode"), my_mode=0, bstatus=c.get("bstatus"),
                                 flag=c["flag"] if flag is None else flag, first=first)
    finally:
        os.environ.pop("DH_CONTAINS_LDS", None)
        if old is not None:
            os.environ["DH_CONTAINS_LDS"] = old


def hold_runs(ctx, c, lds=None):
    """flag / first of one launch against the reference's entry states: flagged exactly when a decidable entry of a served
    run is outside all of its nells ellipsoids, first = the lowest such index, preset words and upper bits kept, masked
    runs as sent, and the same flag when first is not asked for.  Returns (flag, first, share of runs determined)."""
    flag, first = launch(ctx, c, lds)
    share = H.check_runs(flag, first, c["flag"], c["first"], c["states"], c["served"])
    flag_nf, none = launch(ctx, c, lds, with_first=False)
    assert none is None and same(flag_nf, flag), f"{c['name']}: flag differs when first is null"
    return flag, first, share


def by_dh_contains(ctx, c):
    """The words that follow from dh_contains' own verdicts on the same pairs (count > 0 over the run's nells
    ellipsoids), and how many of the served runs' undecided entries it calls outside."""
    R, wpr = len(c["flag"]), c["wpr"]
    x = c["x"].reshape(R, wpr, -1)
    inside = np.empty((R, wpr), dtype=bool)
    for r in range(R):
        m = c["nells_eff"][r]
        inside[r] = ctx.contains(x[r], c["ctrs"][r, :m], c["ams"][r, :m], mode=0 if c["strict"] else 1)[0] > 0
    und = c["served"][:, None] & (c["states"] == 0)
    return H.runs_from_inside(inside, c["served"], c["flag"], c["first"]) + (f"{int((und & ~inside).sum())} of {int(und.sum())}",)


def nearest(c):
    """How near the boundary the run-wise comparison reached: the largest bound / |q - 1| over the decidable pairs of the
    served runs' ellipsoids."""
    best = 0.0
    for r in np.flatnonzero(c["served"]):
        q, b = c["q"][r][:, :c["nells_eff"][r]], c["bound"][r][:, :c["nells_eff"][r]]
        ok = H.decidable(q, b) & ~np.isnan(q) & (b > 0)
        best = max(best, float(np.max((b[ok] / np.abs(q - 1)[ok]).astype(np.float64))))
    return best


@pytest.mark.parametrize("single", (False, True), ids=("multi", "single"))
@pytest.mark.parametrize("d,wpr,lds", C.RUNS_SCALAR)
def test_runs_scalar_form(ctx, d, wpr, lds, single):
    """contains_runs_kernel<N>: against the reference, and bit for bit what dh_contains' own verdicts give on the same
    pairs -- the undecidable shell included: the same multiply-adds in the same order as contains_kernel.  Run 5 makes
    that comparison bite: its flag (with nells) and its first hang on entries of the +-B/8 shell alone."""
    c = C.runs_case(d, wpr, single, True)
    flag, first, share = hold_runs(ctx, c, lds)
    assert share == 0.8  # run 5's words are not the reference's to give: the kernel's rounding of the +-B/8 entries decides
    want_flag, want_first, und = by_dh_contains(ctx, c)
    assert same(flag, want_flag) and same(first, want_first), (c["name"], flag, want_flag, first, want_first)
    print(f"contains_hp contains_runs_kernel {c['name']}: nearest verdict at bound / |q - 1| {nearest(c):.3g}  "
          f"runs determined by the reference {share:.3g}  equal to dh_contains, which calls {und} undecided entries "
          f"outside: run 5 flag {flag[5]} first {first[5]}")


@pytest.mark.parametrize("single", (False, True), ids=("multi", "single"))
@pytest.mark.parametrize("d,wpr", C.RUNS_LDS)
def test_runs_lds_form(ctx, d, wpr, single):
    """contains_runs_lds_kernel<N>: against the reference, bit for bit the scalar form (DH_CONTAINS_LDS=0) on the same
    inputs, and bit for bit dh_contains."""
    c = C.runs_case(d, wpr, single, True)
    flag, first, share = hold_runs(ctx, c)
    assert share == 0.8  # (run 5, as above)
    flag0, first0, _ = hold_runs(ctx, c, "0")
    assert same(flag, flag0) and same(first, first0), (c["name"], flag, flag0, first, first0)
    want_flag, want_first, und = by_dh_contains(ctx, c)
    assert same(flag, want_flag) and same(first, want_first), (c["name"], flag, want_flag, first, want_first)
    print(f"contains_hp contains_runs_lds_kernel {c['name']}: nearest verdict at bound / |q - 1| {nearest(c):.3g}  "
          f"runs determined by the reference {share:.3g}  equal to the scalar form and to dh_contains, which calls {und} "
          f"undecided entries outside: run 5 flag {flag[5]} first {first[5]}")


@pytest.mark.parametrize("single", (False, True), ids=("multi", "single"))
@pytest.mark.parametrize("d,wpr", C.RUNS_WIDE)
def test_runs_wide_form(ctx, d, wpr, single):
    """contains_runs_wide_kernel: partial tiles, the chunk loop, P = 4 above 256, the early exit.  Decidable pairs only,
    and every entry of these cases is decidable: every served run's words are determined by the reference."""
    c = C.runs_case(d, wpr, single, False)
    assert not (c["states"] == 0).any()
    flag, first, share = hold_runs(ctx, c)
    assert share == 1.0
    want_flag, want_first = H.runs_from_inside(c["states"] == -1, c["served"], c["flag"], c["first"])
    assert same(flag, want_flag) and same(first, want_first), (c["name"], flag, want_flag, first, want_first)
    print(f"contains_hp contains_runs_wide_kernel {c['name']}: nearest verdict at bound / |q - 1| {nearest(c):.3g}  "
          f"runs determined by the reference {share:.3g}")


EXACT_RUNS = ([(d, 5, None) for d in C.NARROW_D] + [(d, 256, None) for d in (9, 13, 25, 32)] +
              [(13, 256, "0"), (25, 256, "0")] + [(d, 5, None) for d in C.WIDE_D])


@pytest.mark.parametrize("strict", (1, 0))
@pytest.mark.parametrize("d,wpr,lds", EXACT_RUNS)
def test_runs_exact(ctx, d, wpr, lds, strict):
    """q == 1 exactly through flag / first in all three run-wise kernels: strict (q < 1) flags the run at that entry, the
    single bound (sqrt(q) <= 1) does not; the neighbour one ulp outside flags its run in both, the one inside never."""
    c = C.exact_runs_case(d, wpr, strict)
    flag, first = launch(ctx, c, lds, flag=np.zeros(3, dtype=np.int32))
    assert same(flag, c["want_flag"]) and same(first, c["want_first"]), (c["name"], flag, first)
    print(f"contains_hp exact runs {c['name']}: flag {list(flag)} first {list(first)} (exact)")


def test_contains_runs_refuses_bad_arguments(ctx):
    """DH_ERR_ARG for a null required pointer, d / wpr / max_ells / runs < 1, d above the wide limit and an nells beyond
    max_ells; the context serves a correct call afterwards."""
    from dynesty_amd import _lib
    c = C.runs_case(5, 5, False, True)
    R, wpr, d, me = 7, 5, 5, 4
    arrs = dict(x=np.ascontiguousarray(c["x"]), ctrs=np.ascontiguousarray(c["ctrs"]), ams=np.ascontiguousarray(c["ams"]),
                nells=np.ascontiguousarray(c["nells"]), flag=np.zeros(R, dtype=np.int32), first=np.zeros(R, dtype=np.int32))

    def call(runs=R, wpr=wpr, d=d, max_ells=me, **null):
        p = {k: (None if null.get(k) else _lib._ptr(v)) for k, v in arrs.items()}
        return ctx.lib.dh_contains_runs(ctx.handle, p["x"], runs, wpr, d, p["ctrs"], p["ams"], p["nells"], max_ells, 1,
                                        None, 0, None, p["flag"], p["first"])
    for kw in (dict(x=True), dict(ctrs=True), dict(ams=True), dict(flag=True), dict(d=0), dict(wpr=0), dict(max_ells=0),
               dict(runs=0), dict(d=513), dict(max_ells=3)):
        assert call(**kw) == _lib.ERR_ARG, kw
        assert "contains_runs" in ctx.lib.dh_last_error(ctx.handle).decode()
    flag, first, share = hold_runs(ctx, c)
    assert share == 0.8 and flag[0] & 1 and first[0] == wpr - 1
