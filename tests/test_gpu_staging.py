"""The host-pointer entry points stage their arrays through one carved layout of the context's arena (ctx.h: arena_carve;
stage_plan.h).  The first call on a fresh context is sized so that its layout does not fit the arena dh_create made: that
call grows the arena.  The same inputs passed as two halves on a second fresh context fit without growth.  Walkers and
candidates are independent, and which kernel serves a call is a function of the problem alone, so the two must agree bit
for bit -- values, counts, flags and generator end states.  A small call on the grown context (one walker, then 65)
closes each case, compared the same way."""
import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

# dh_create reserves 8 MiB; arena_reserve makes that bytes + bytes / 2 + 1 MiB
ARENA0 = (8 << 20) + (8 << 20) // 2 + (1 << 20)
K, NDIM = 64 * 512, 25


def total(*sizes):
    """What a layout of arrays of these byte sizes takes: each 256-byte aligned."""
    return sum((s + 255) & ~255 for s in sizes)


def grows_then_fits(k, layout):
    """The whole call outgrows the first arena, each half fits in it."""
    assert layout(k) > ARENA0 >= layout(k // 2), (layout(k), ARENA0, layout(k // 2))


@pytest.fixture(scope="module")
def case():
    from dynesty_amd import _lib
    c = inputs.walker_case("C2", K + K // 8, 20261)
    assert c["u0"].shape[0] >= K and c["problem"].ndim == NDIM
    c["u0"] = np.ascontiguousarray(c["u0"][:K])
    c["states"] = _lib.Context(0).seed_children([5, 6, 7, 8], 0, K)
    return c


def same(a, b):
    a, b = (x if isinstance(x, dict) else dict(enumerate(x)) for x in (a, b))
    assert a.keys() == b.keys()
    for key in a:
        if a[key] is not None or b[key] is not None:
            np.testing.assert_array_equal(a[key], b[key], err_msg=str(key))


def joined(parts):
    """The results of consecutive slices of one call's walkers, put together again."""
    parts = [p if isinstance(p, dict) else dict(enumerate(p)) for p in parts]
    return {key: None if parts[0][key] is None else np.concatenate([p[key] for p in parts]) for key in parts[0]}


def check(call, k):
    """call(ctx, lo, hi): the entry point on the inputs of walkers lo .. hi."""
    from dynesty_amd import _lib
    grown, plain = _lib.Context(0), _lib.Context(0)
    same(call(grown, 0, k), joined([call(plain, 0, k // 2), call(plain, k // 2, k)]))  # the first call grows the arena
    same(call(grown, 0, 1), call(plain, 0, 1))
    same(call(grown, 0, 65), joined([call(plain, 0, 64), call(plain, 64, 65)]))


def test_rwalk_batch(case):
    d = NDIM
    grows_then_fits(K, lambda k: total(k * d * 8, d * d * 8, k * 32, k * d * 8, k * d * 8, k * 8, k * 4, k * 4, k * 32))
    check(lambda ctx, lo, hi: ctx.rwalk_batch(case["problem"], case["u0"][lo:hi], case["axes"], case["scale"],
                                              case["loglstar"], 2, case["states"][lo:hi]), K)


def test_slice_batch(case):
    d = NDIM
    grows_then_fits(K, lambda k: total(k * d * 8, d * d * 8, k * 32, k * d * 8, k * d * 8, k * 8, k * 4, k * 4, k * 4, k * 4,
                                       k * 32))
    check(lambda ctx, lo, hi: ctx.slice_batch(case["problem"], case["u0"][lo:hi], case["axes"], case["scale"],
                                              case["loglstar"], 1, case["states"][lo:hi]), K)


def test_unif_batch(case):
    d = NDIM
    grows_then_fits(K, lambda k: total(d * 8, d * d * 8, k * 32, k * d * 8, k * d * 8, k * 8, k * 4, k * 4, k * 32))
    ctr, axes = np.full(d, 0.5), 0.05 * np.eye(d)  # one ellipsoid inside the cube; every draw of it is accepted
    check(lambda ctx, lo, hi: ctx.unif_batch(case["problem"], -1e300, case["states"][lo:hi], ctrs=ctr, axes=axes), K)


def test_problem_eval(case):
    d, k = NDIM, 40000
    grows_then_fits(k, lambda k: total(k * d * 8, k * d * 8, k * 8))
    u = np.random.default_rng(11).uniform(0.02, 0.98, size=(k, d))
    check(lambda ctx, lo, hi: ctx.problem_eval(case["problem"], u[lo:hi]), k)


def test_contains():
    d, m = NDIM, 32
    grows_then_fits(K, lambda k: total(k * d * 8, m * d * 8, m * d * d * 8, k * 4, (k + 63) // 64 * m * 8, k * m * 8))
    rng = np.random.default_rng(12)
    x = rng.uniform(0, 1, size=(K, d))
    ctrs = rng.uniform(0.3, 0.7, size=(m, d))
    radii = rng.uniform(1.2, 1.6, size=m)
    ams = np.stack([np.eye(d) / r ** 2 for r in radii])
    inside = ((x[:2000, None, :] - ctrs[None]) ** 2).sum(-1) < radii ** 2
    assert 0.05 < inside.mean() < 0.95  # the candidates fall inside some ellipsoids and outside others

    def call(ctx, lo, hi):
        count, mask, quad = ctx.contains(x[lo:hi], ctrs, ams, want_mask=True, want_quad=True)
        bits = np.unpackbits(mask.view(np.uint8).reshape(m, -1), axis=1, bitorder="little")[:, :hi - lo]
        return dict(count=count, inside=bits.T, quad=quad)  # one row per candidate: the halves join along the rows
    check(call, K)
