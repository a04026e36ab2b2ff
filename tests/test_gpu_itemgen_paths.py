"""Every path of the generator pass's round (csrc/walkq.hip, `itemgen_kernel`) on the device, bit for bit.

The pass resolves a round's missed ziggurat candidates with the next position's draw, which lane l takes from lane
l + 1 by a wave-shift move (no LDS round trip), the wedge test's table pair read beside the fast-accept pair, and one
store under a scalar mask of the round's items.  A wrong shift direction, a stale pair or a wrong item mask changes a
wedge verdict or an item and with it everything behind it in the walker's stream, so the pass is held to

  * the generator inside the walk kernel (`wavegen_round`, `set_rwalk_items(False)`): every output of the walk equal;
  * numpy: the generator state left behind equals `Generator(PCG64(child))` after walks x (d normals, one uniform);

over streams that the host restatement of the round (tests/test_quad_rng_host.WaveGen) shows to reach every class of
round: wedge accepted / rejected, two or more misses in a round, a wedge uniform that takes what had been a step's
uniform slot, the `idx == 0` tail, a miss at position 62, a miss in the walker's last round, and a wedge verdict
inside the single-precision band (which sends the round to the double-precision test)."""
import collections
import functools
import math

import numpy as np
import pytest

import test_quad_rng_host as H
from test_rng_host import M128, M64, load_tables

pytestmark = pytest.mark.gpu

# (d, walks, walkers)
CASES = [(25, 8, 1024), (12, 5, 1024), (2, 20, 256)]
MIN_ROUNDS = 10  # of every class, in the d = 25 case
KEYS = ("u", "v", "logl", "accept", "reject", "rng_out")


class CountingWaveGen(H.WaveGen):
    """WaveGen that classifies every round before running it (the resolution restated once more, counting only)."""

    def __init__(self, base, inc, nc, steps, tables, counts):
        super().__init__(base, inc, nc, steps)
        self.tables, self.counts = tables, counts
        ki, wi, fi = tables
        # the pass's single-precision pair: (fi[i - 1] - fi[i], fi[i])
        self.ffx = [np.float32(fi[max(i - 1, 0)] - fi[i]) for i in range(256)]
        self.ffy = [np.float32(fi[i]) for i in range(256)]

    def round(self, ki, wi, fi):
        C, n, n1 = self.counts, self.n, self.n1
        st = [(self.S0 + H.G[l + 1] * self.D) & M128 for l in range(64)]
        r = [H.out64(s) for s in st]
        idx = [v & 0xff for v in r]
        rabs = [(v >> 9) & 0x000fffffffffffff for v in r]
        missmask = sum((0 if rabs[l] < ki[idx[l]] else 1) << l for l in range(63))
        umask = (self.U0 << (n - self.W % n1)) & M64
        m = missmask & ~umask
        C["rounds"] += 1
        if m:
            C["general"] += 1
            if not self.W < self.T - 63:
                C["last_round_with_miss"] += 1
            misses = 0
            while m:
                f = (m & -m).bit_length() - 1
                if idx[f] == 0:
                    C["tail"] += 1
                    break
                if f == 62:
                    C["miss_at_62"] += 1
                    break
                x = (-1.0 if r[f] & 0x100 else 1.0) * (rabs[f] * wi[idx[f]])
                lhs = (fi[idx[f] - 1] - fi[idx[f]]) * H.u53(r[f + 1]) + fi[idx[f]]
                acc = 1 if lhs < math.exp(-0.5 * x * x) else 0
                C["wedge_accepted" if acc else "wedge_rejected"] += 1
                # the first look in single precision, as the kernel forms it
                xf = np.float32(x)
                lhs32 = self.ffx[idx[f]] * (np.float32(r[f + 1] >> 40) * np.float32(2.0 ** -24)) + self.ffy[idx[f]]
                ef32 = np.exp(np.float32(-0.5) * xf * xf)
                if abs(lhs32 - ef32) <= np.float32(1e-5):
                    C["band"] += 1
                if (umask >> (f + 1)) & 1:
                    C["wedge_uniform_on_step_uniform_slot"] += 1
                misses += 1
                keep = f + 2
                low = umask & ((1 << keep) - 1)
                umask = (low | ((umask >> (f + acc)) << keep)) & M64
                m = missmask & ~umask & ((M64 << keep) & M64)
            if misses >= 2:
                C["two_or_more_misses"] += 1
        super().round(ki, wi, fi)


@functools.lru_cache(maxsize=None)
def round_classes(d, walks, k):
    """How often each class of round occurs over the case's streams (children 0 .. k - 1 of SeedSequence([d, 1, 2]))."""
    tables = load_tables()
    counts = collections.Counter()
    for kid in np.random.SeedSequence([d, 1, 2]).spawn(k):
        base, inc = H.np_state(np.random.PCG64(kid))
        q = CountingWaveGen(base, inc, d, walks, tables, counts)
        for s in range(walks):
            q.step_items(s, *tables)
    return dict(counts)


def assert_every_class_occurs():
    d, walks, k = CASES[0]
    C = round_classes(d, walks, k)
    print("rounds by class, d = %d: %s" % (d, C))
    for name in ("wedge_accepted", "wedge_rejected", "two_or_more_misses", "wedge_uniform_on_step_uniform_slot", "tail",
                 "miss_at_62", "last_round_with_miss"):
        assert C.get(name, 0) >= MIN_ROUNDS, (name, C)
    assert C.get("band", 0) >= 1, C


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    c = _lib.Context(0)
    yield c
    c.set_rwalk_form(0)
    c.set_rwalk_items(True, 1 << 30)


def walk_args(d, walks, k):
    from dynesty_amd import problems
    prob = problems.gauss_corr(d, 0.4, 5.0, f"corr{d}")
    rng = np.random.default_rng(70 + d)
    hw = prob.prior_par[0]
    spread = 0.5 / (2 * hw)
    u0 = np.clip(0.5 + spread * rng.standard_normal((k + 400, d)), 1e-3, 1 - 1e-3)
    logl = prob.loglikelihood_many(prob.prior_transform_many(u0))
    loglstar = float(np.quantile(logl, 0.05))
    u0 = u0[logl > loglstar][:k]  # start points inside the contour
    assert len(u0) == k
    q, _ = np.linalg.qr(rng.standard_normal((d, d)))
    axes = q * (spread * math.sqrt(d) * rng.uniform(0.8, 1.6, size=d))
    return prob, u0, axes, 0.7, loglstar, walks


def numpy_end_states(d, walks, k):
    from dynesty_amd import _lib
    out = np.empty((k, 4), dtype=np.uint64)
    for i, kid in enumerate(np.random.SeedSequence([d, 1, 2]).spawn(k)):
        bg = np.random.PCG64(kid)
        gen = np.random.Generator(bg)
        for _ in range(walks):
            gen.standard_normal(d)
            gen.random()
        out[i] = _lib.pcg_state_words(bg)
    return out


def pass_against_fused(ctx, d, walks, k, budget):
    st = ctx.seed_children([d, 1, 2], 0, k)
    args = walk_args(d, walks, k) + (st,)
    ctx.set_rwalk_form(2)
    try:
        ctx.set_rwalk_items(False)
        fused = ctx.rwalk_batch(*args)
        ctx.set_rwalk_items(True, budget)
        items = ctx.rwalk_batch(*args)
    finally:
        ctx.set_rwalk_items(True, 1 << 30)
    for key in KEYS:
        np.testing.assert_array_equal(items[key], fused[key], err_msg=key)
    np.testing.assert_array_equal(items["rng_out"], numpy_end_states(d, walks, k))
    assert fused["accept"].sum() > 0 and fused["reject"].sum() > 0


@pytest.mark.parametrize("d,walks,k", CASES)
def test_generator_pass_equals_fused_generator_and_numpy(ctx, d, walks, k):
    if (d, walks, k) == CASES[0]:
        assert_every_class_occurs()
    pass_against_fused(ctx, d, walks, k, 1 << 30)


def test_generator_pass_in_chunks_of_walkers(ctx):
    """The d = 25 case with an item buffer of 200 walkers' streams: the launch goes in chunks whose edges fall off every
    granularity of the pass (wavefront, workgroup, grid)."""
    d, walks, k = CASES[0]
    assert_every_class_occurs()
    pass_against_fused(ctx, d, walks, k, 200 * walks * (d + 1) * 8)
