"""The throughput RNG mode (hiprand Philox4x32-10) held to a stream-exact reference: tests/philox_ref.py restates the
words the kernels draw and the transforms they apply (pinned to rocrand itself by tests/test_philox_ref_cpu.py), and
its generator adapters drive the oracle's proposal functions in the kernels' order.

  a. raw stream, exact: unit-cube draws (uniform doubles) bit for bit, and with a real threshold the winning try and
     the call counts;
  b. normal words to float32 resolution: one-step rwalk / rslice proposals against the restated z / |z| and u^(1/n),
     in every form of the kernels (lane, four-lane with and without the items pass, wave-per-walker);
  c. whole chains against the oracle on the restated streams (principal-axes slice chains, uniform sampling in one or
     several ellipsoids): exact counts and u / logl to a tolerance derived from the bound of (b), for every walker
     with no decision within a stated margin of its boundary.

The device evaluates Box-Muller with __sincosf and ocml logf, so normals differ from the float64 restatement by
float32 rounding; NORMAL_BOUND below is the committed bound on a direction component (measured largest difference on
an MI355X rounded up to a power of two).  A wrong or shifted word gives differences of order one.
"""
import numpy as np
import pytest

import inputs
import philox_ref as PR

pytestmark = pytest.mark.gpu

# measured largest |direction component - restated| over (b): see test_normal_words_*; rounded up to a power of two
NORMAL_BOUND = 2.0**-18  # measured 2.15e-6 (2^-18.8) on an MI355X
# share of a batch allowed to have a decision within the margin of its boundary: one-step draws and single
# proposals; 45-step rwalk chains carry every accepted step's error on, and their worst-case margin sets aside
# 0.25-1.5 % of the walkers of these cases (printed), so they are allowed 2 %
MAX_NEAR = 0.005
MAX_NEAR_CHAIN = 0.02

SEEDS_SEQS = [(5, 0), (0xDEADBEEFDEADBEEF, 1), (0xFFFFFFFFFFFFFFFF, 2**32 - 1 - 300), (0x8000000000000001, 2**32 + 5)]
OFFSETS = [0, 1, 2, 3, 2**34 - 2, 2**34 + 1]


def _ctx(monkeypatch=None, **env):
    from dynesty_amd import _lib
    if monkeypatch is not None:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
    return _lib.Context(0)


@pytest.fixture(scope="module")
def ctx():
    return _ctx()


def gauss(ndim):
    from dynesty_amd import problems
    return problems.gauss_iid(ndim, 10.0, f"g{ndim}")


def lane_dims():
    """The dimensions with a register-resident (lane) instantiation: DH_DIM_LIST of csrc/ctx.h."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "dynesty_amd", "csrc", "ctx.h")).read()
    line = re.search(r"#define DH_DIM_LIST\(X\)(.*)", src).group(1)
    return {int(x) for x in re.findall(r"X\((\d+)\)", line)}


def slice_has_lane_kernel(ndim):
    """slice_batch_philox runs the lane kernel only for a dimension of DH_DIM_LIST (walk2.hip: pad_dim(n) != n goes to
    the wave-per-walker kernel); rwalk_batch_philox and unif_batch_philox use their lane kernels (padded) up to 32."""
    return ndim in lane_dims()


def cube_try(seed, seqs, offset, ndim, t, wide):
    """The restated unit-cube try t of the walkers `seqs`: lane / four-lane forms take try t from the 2 n words at
    offset + 2 n t; the wave-per-walker kernel (n > 32) n doubles in pairs, 4 ceil(n / 2) words a try, from the
    offset rounded up to a multiple of 4."""
    per = 4 * ((ndim + 1) // 2) if wide else 2 * ndim
    if wide:
        offset = (offset + 3) & ~3
    w = PR.words(seed, seqs, offset + per * t, 2 * ndim).astype(np.uint64)
    return 1.0 - PR.uniform_double(w[:, 0::2], w[:, 1::2])


# ---- (a) raw stream, exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [2, 3, 7, 25, 33, 64])
def test_unit_cube_first_try_is_the_keyed_stream(monkeypatch, ndim):
    prob = gauss(ndim)
    forms = ("1", "2") if ndim <= 32 else ("0",)
    k = 1000 + 37 if ndim <= 32 else 301
    for form in forms:
        c = _ctx(monkeypatch, DH_CUBE_FORM=form)
        for seed, seq0 in SEEDS_SEQS:
            for off in OFFSETS:
                out = c.unif_batch_philox(prob, -1e300, k, seed=seed, sequence0=seq0, offset=off)
                seqs = seq0 + np.arange(k, dtype=np.uint64)
                ref = cube_try(seed, seqs, off, ndim, 0, ndim > 32)
                assert np.all(out["ncalls"] == 1)
                np.testing.assert_array_equal(out["u"], ref, err_msg=f"form {form} seed {seed:#x} seq0 {seq0} off {off}")


@pytest.mark.parametrize("ndim", [2, 3, 7, 25, 33, 64])
def test_unit_cube_winning_try_and_calls(monkeypatch, ndim):
    """A real threshold: every try of every walker is restated until it beats the threshold; the returned point is
    the first winner's, bit for bit, and the call count its index + 1.  Walkers with a try whose log-likelihood lies
    within 1e-9 of the threshold are left out and counted: the tries are exact, so only the likelihood's rounding
    (device vs NumPy, a few ulp of |logl| ~ 40 here, far below 1e-9) can part the two."""
    prob = gauss(ndim)
    rng = np.random.default_rng(ndim)
    ll0 = prob.loglikelihood_many(prob.prior_transform_many(rng.random((20000, ndim))))
    thr = float(np.quantile(ll0, 0.9))
    k = 500 + 11
    forms = ("1", "2") if ndim <= 32 else ("0",)
    for form in forms:
        c = _ctx(monkeypatch, DH_CUBE_FORM=form)
        for seed, seq0 in SEEDS_SEQS[1:3]:
            off = 2**34 - 2 + ndim % 4
            out = c.unif_batch_philox(prob, thr, k, seed=seed, sequence0=seq0, offset=off)
            seqs = seq0 + np.arange(k, dtype=np.uint64)
            win = np.full(k, -1)
            u_win = np.zeros((k, ndim))
            near = np.zeros(k, bool)
            t = 0
            while (win < 0).any():
                u = cube_try(seed, seqs, off, ndim, t, ndim > 32)
                ll = prob.loglikelihood_many(prob.prior_transform_many(u))
                open_ = win < 0
                near |= open_ & (np.abs(ll - thr) < 1e-9)
                hit = open_ & (ll > thr)
                win[hit] = t
                u_win[hit] = u[hit]
                t += 1
                assert t < 5000
            ok = ~near
            print(f"D={ndim} form {form}: {near.sum()} of {k} walkers within 1e-9 of the threshold")
            assert near.mean() <= MAX_NEAR
            np.testing.assert_array_equal(out["ncalls"][ok], win[ok] + 1)
            np.testing.assert_array_equal(out["u"][ok], u_win[ok])
            assert np.all(out["logl"] > thr)


def test_wide_offsets_round_up_to_whole_blocks(ctx):
    """The wave-per-walker entry points round the key's offset up to a multiple of 4 (WaveGen advances in whole
    blocks): offsets 1, 2, 3 and 4 give one stream there, while the lane kernels give four.  ns.hip passes multiples of
    4 only (fill << 24, fill walks (4 ceil(D / 4) + 4)), so the resident loop never meets the aliasing."""
    wide, lane = gauss(40), gauss(7)
    a = [ctx.unif_batch_philox(wide, -1e300, 64, seed=3, sequence0=9, offset=o)["u"] for o in (1, 2, 3, 4, 5)]
    for x in a[1:4]:
        np.testing.assert_array_equal(x, a[0])
    assert (a[4] != a[0]).all()
    b = [ctx.unif_batch_philox(lane, -1e300, 64, seed=3, sequence0=9, offset=o)["u"] for o in (1, 2, 3, 4)]
    for i in range(4):
        for j in range(i):
            assert (b[i] != b[j]).all()


# ---- (b) normal words, to float32 resolution ---------------------------------------------------------------------
def lane_rwalk_step(seed, seqs, off, n):
    """LaneGen one-step rwalk draws: ceil(n / 4) hiprand_normal4, then hiprand_uniform_double (in (0, 1], unflipped)."""
    nb = (n + 3) // 4
    w = PR.words(seed, seqs, off, 4 * nb + 2)
    z = PR.normal4(w[:, :4 * nb].reshape(len(seqs), nb, 4)).reshape(len(seqs), -1)[:, :n].astype(np.float64)
    ur = PR.uniform_double(w[:, 4 * nb], w[:, 4 * nb + 1])
    return z, ur


def wave_rwalk_step(seed, seqs, off, n):
    """WaveGen one-step rwalk draws (n = ncdim): normals(n) in 4 ceil(n / 4) words, then a scalar uniform (a whole
    block, 1 - hiprand's)."""
    nb = (n + 3) // 4
    w = PR.words(seed, seqs, off, 4 * nb + 4)
    z = PR.normal4(w[:, :4 * nb].reshape(len(seqs), nb, 4)).reshape(len(seqs), -1)[:, :n].astype(np.float64)
    ur = 1.0 - PR.uniform_double(w[:, 4 * nb], w[:, 4 * nb + 1])
    return z, ur


def frame(ndim, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((ndim, ndim)))
    return q * rng.uniform(0.5, 2.0, size=ndim) * 1e-3


def check_direction_radius(dr, z, ur, n, what):
    """dr (frame coordinates) against the restated direction z / |z| and radius ur^(1/n): the radius comes from the
    uniform words and the norm of the widened float32 normals, so it is held to 1e-9 whatever the normals' rounding;
    the direction to NORMAL_BOUND.  Returns the largest direction difference."""
    r = np.linalg.norm(dr, axis=1)
    np.testing.assert_allclose(r, ur**(1.0 / n), rtol=1e-9, atol=1e-12, err_msg=what)
    d = dr / r[:, None] - z / np.linalg.norm(z, axis=1)[:, None]
    worst = float(np.abs(d).max())
    print(f"{what}: largest direction difference {worst:.3e} ({np.log2(max(worst, 1e-30)):.1f} as a power of two)")
    assert worst <= NORMAL_BOUND, (what, worst)
    return worst


RWALK_FORMS = [("lane", dict(form=1)), ("four-lane, items pass", dict(form=2, items=True)),
               ("four-lane, fused generator", dict(form=2, items=False))]


@pytest.mark.parametrize("ndim", [2, 5, 8, 13, 25, 32])
def test_normal_words_one_step_rwalk(ndim):
    from dynesty_amd import _lib, problems
    prob = problems.gauss_corr(ndim, 0.3, 50.0, "wide-prior")
    axes = frame(ndim, ndim)
    k = 4096 + 5
    u0 = np.full((k, ndim), 0.5)
    for name, f in RWALK_FORMS:
        c = _lib.Context(0)
        c.set_rwalk_form(f["form"])
        if "items" in f:
            c.set_rwalk_items(f["items"])
        for seed, seq0 in SEEDS_SEQS[:3]:
            for off in (0, 3, 2**34 + 1):
                out = c.rwalk_batch_philox(prob, u0, axes, 1.0, -1e300, 1, seed=seed, sequence0=seq0, offset=off)
                assert np.all(out["accept"] == 1)
                seqs = seq0 + np.arange(k, dtype=np.uint64)
                z, ur = lane_rwalk_step(seed, seqs, off, ndim)
                dr = np.linalg.solve(axes, (out["u"] - u0).T).T
                check_direction_radius(dr, z, ur, ndim, f"rwalk D={ndim} {name} off {off}")
        c.close()


@pytest.mark.parametrize("ndim", [40, 64])
def test_normal_words_one_step_wide(ctx, ndim):
    """The wave-per-walker kernels (n > 32): WaveGen normals in fours at pos + i -- one-step rwalk (direction and
    radius) and one-step rslice (the slice direction z / |z|, recovered from the move along it)."""
    from dynesty_amd import problems
    prob = problems.gauss_corr(ndim, 0.3, 50.0, "wide-prior")
    axes = frame(ndim, ndim)
    ball = gauss(ndim)
    ball_lstar = float(ball.like_par[0] - 0.5 * 4.0)  # |v| < 2: |u - 0.5| < 0.1
    k = 257
    u0 = np.full((k, ndim), 0.5)
    for seed, seq0 in SEEDS_SEQS[1:]:
        for off in (1, 2**34 - 2):
            seqs = seq0 + np.arange(k, dtype=np.uint64)
            out = ctx.rwalk_batch_philox(prob, u0, axes, 1.0, -1e300, 1, seed=seed, sequence0=seq0, offset=off)
            assert np.all(out["accept"] == 1)
            off4 = (off + 3) & ~3  # (the wide entry points round the offset up to whole blocks)
            z, ur = wave_rwalk_step(seed, seqs, off4, ndim)
            dr = np.linalg.solve(axes, (out["u"] - u0).T).T
            check_direction_radius(dr, z, ur, ndim, f"wide rwalk D={ndim} off {off}")
            # rslice on a ball contour (so that the bracket closes): the first draws of a slice are the direction's
            # normals (ceil(n / 4) blocks)
            sl = ctx.slice_batch_philox(ball, u0, axes * 50.0, 1.0, ball_lstar, 1, seed=seed, sequence0=seq0,
                                        offset=off)
            assert np.all(sl["logl"] > ball_lstar)
            nb = (ndim + 3) // 4
            w = PR.words(seed, seqs, off4, 4 * nb)
            zs = PR.normal4(w.reshape(k, nb, 4)).reshape(k, -1)[:, :ndim].astype(np.float64)
            dd = np.linalg.solve(axes, (sl["u"] - u0).T).T
            dd /= np.linalg.norm(dd, axis=1)[:, None]
            zs /= np.linalg.norm(zs, axis=1)[:, None]
            dd *= np.sign(np.sum(dd * zs, axis=1))[:, None]
            worst = float(np.abs(dd - zs).max())
            print(f"wide rslice D={ndim} off {off}: largest direction difference {worst:.3e}")
            assert worst <= NORMAL_BOUND


# ---- (c) whole chains against the oracle on the restated streams -------------------------------------------------
class Margin:
    """Wraps a problem for the oracle and records, for every decision the oracle takes, whether it lies within the
    margin of its boundary.  The oracle's point is within du of the kernel's, du = acc + du_step: du_step is what one
    proposal's draws can move it, and with accumulate=True every accepted proposal (logl > loglstar) adds du_step to
    acc, the error carried by the current point.  A likelihood comparison is near when |logl - loglstar| is below the
    change of logl over a ball of radius du around the point (first order: the coordinate differences at +-du, in
    quadrature) plus 1e-9 (1 + |logl|) of rounding; a unit-cube check when a coordinate lies within du of 0 or 1 (or a
    non-bounded one within du of -0.5 or 1.5)."""

    def __init__(self, prob, loglstar, du_step, unitcheck, accumulate=False):
        self.prob, self.loglstar, self.du_step = prob, loglstar, du_step
        self.accumulate, self.acc = accumulate, 0.0
        self._unitcheck = unitcheck
        self.near = False
        self._u = None

    @property
    def du(self):
        return self.acc + self.du_step

    def prior_transform(self, u):
        self._u = np.array(u, dtype=float)
        return self.prob.prior_transform(u)

    def loglikelihood(self, v):
        ll = float(self.prob.loglikelihood(v))
        u, n, du = self._u, len(self._u), self.du
        pert = np.concatenate([u + du * np.eye(n), u - du * np.eye(n)])
        lp = self.prob.loglikelihood_many(self.prob.prior_transform_many(np.clip(pert, 0.0, 1.0)))
        ch = np.maximum(np.abs(lp[:n] - ll), np.abs(lp[n:] - ll))
        if abs(ll - self.loglstar) <= np.sqrt(np.sum(ch**2)) + 1e-9 * (1.0 + abs(ll)):
            self.near = True
        if self.accumulate and ll > self.loglstar:
            self.acc += self.du_step
        return ll

    def unitcheck(self, u, nonbounded=None):
        u = np.asarray(u)
        nb = np.zeros(len(u), bool) if nonbounded is None else np.asarray(nonbounded)
        if np.min(np.minimum(np.abs(u), np.abs(1.0 - u))) < self.du:  # (a wrapped coordinate: near its wrap)
            self.near = True
        if nb.any() and np.min(np.minimum(np.abs(u[nb] + 0.5), np.abs(1.5 - u[nb]))) < self.du:
            self.near = True
        return self._unitcheck(u, nonbounded)


@pytest.fixture
def traced(monkeypatch):
    """Routes the oracle's unit-cube checks through the current Margin: traced(prob, loglstar, du_step, ...) makes
    one and installs it."""
    from oracle import proposals_ref as P
    orig = P.unitcheck
    cur = {}
    monkeypatch.setattr(P, "unitcheck", lambda u, nonbounded=None: cur["m"].unitcheck(u, nonbounded))

    def make(prob, loglstar, du_step, accumulate=False):
        cur["m"] = Margin(prob, loglstar, du_step, orig, accumulate)
        return cur["m"]
    make.current = cur
    return make


def compare_walkers(out, refs, nears, keys, du, dll, what, max_near=MAX_NEAR):
    """Exact counts and u / logl within (du, dll) for every walker without a near decision; at most max_near near."""
    k = len(refs)
    near = np.array(nears)
    print(f"{what}: {near.sum()} of {k} walkers with a decision within the margin (du = {du:.2e})")
    assert near.mean() <= max_near, (what, near.sum(), k)
    bad = []
    for i in np.flatnonzero(~near):
        r = refs[i]
        if any(out[kk][i] != r[rk] for kk, rk in keys):
            bad.append((i, [(kk, out[kk][i], r[rk]) for kk, rk in keys]))
            continue
        if np.abs(out["u"][i] - r["u"]).max() > du or abs(out["logl"][i] - r["logl"]) > dll * (1 + abs(r["logl"])):
            bad.append((i, "u / logl", np.abs(out["u"][i] - r["u"]).max(), out["logl"][i], r["logl"]))
    assert not bad, (what, len(bad), bad[:5])


RWALK_CASES = [("C2", {}), ("G5", {}), ("G5", {"frames": 3}), ("G5", {"bc": True}), ("G5", {"ncdim": 3})]


def rwalk_case(pname, opt, k=400):
    from dynesty_amd import _lib
    case = inputs.walker_case(pname, 800, 31)
    prob = case["problem"]
    ndim = prob.ndim
    u0 = case["u0"][:k]
    nc = opt.get("ncdim", ndim)
    nf = opt.get("frames", 1)
    frames = np.stack([case["axes"][:nc, :nc] * (1.0 + 0.3 * f) for f in range(nf)])
    idx = np.random.default_rng(5).integers(nf, size=k).astype(np.int32) if nf > 1 else None
    bc = periodic = reflective = nonbounded = None
    if opt.get("bc"):
        bc = np.array([_lib.BC_PERIODIC, _lib.BC_REFLECT] + [_lib.BC_HARD] * (ndim - 2), dtype=np.int8)
        periodic, reflective = np.array([0]), np.array([1])
        nonbounded = np.zeros(ndim, bool)
        nonbounded[:2] = True
    return dict(prob=prob, u0=u0, loglstar=case["loglstar"], scale=case["scale"], nc=nc, frames=frames, idx=idx,
                bc=bc, periodic=periodic, reflective=reflective, nonbounded=nonbounded)


def rwalk_oracle(c, traced, seed, seq0, off, walks):
    """proposals_ref.rwalk per walker on LaneStream(flip=False): the rwalk lane kernel's order (the non-clustered
    coordinates' uniforms, ceil(nc / 4) hiprand_normal4, the radius uniform unflipped).  Margin: a proposal's draws move
    the point by at most du_step = scale |axes|_2 sqrt(nc) NORMAL_BOUND (the direction's components within
    NORMAL_BOUND, the radius exact), and each accepted step carries its error on."""
    from oracle import proposals_ref as P
    refs, nears, du_max = [], [], 0.0
    for i in range(len(c["u0"])):
        ax = c["frames"][c["idx"][i] if c["idx"] is not None else 0]
        m = traced(c["prob"], c["loglstar"], c["scale"] * np.linalg.norm(ax, 2) * np.sqrt(c["nc"]) * NORMAL_BOUND,
                   accumulate=True)
        st = PR.LaneStream(seed, seq0 + i, off, flip=False, normal_mode="normal4")
        r = P.rwalk(c["u0"][i].copy(), c["loglstar"], ax, c["scale"], m.prior_transform, m.loglikelihood, st, walks,
                    periodic=c["periodic"], reflective=c["reflective"], nonbounded=c["nonbounded"])
        refs.append(r)
        nears.append(m.near)
        du_max = max(du_max, m.du)
    return refs, nears, du_max


@pytest.mark.parametrize("pname,opt", RWALK_CASES, ids=["C2", "G5", "G5-frames", "G5-bc", "G5-ncdim"])
def test_rwalk_chains_against_the_oracle(traced, pname, opt):
    """45-step rwalk_batch_philox (lane form; the four-lane forms are held to it bit for bit by test_gpu_rwalkq.py)
    against proposals_ref.rwalk on the restated streams: several frames by axes_idx, periodic and reflective
    coordinates, ncdim < ndim.  Accept and reject counts exact, u within the accumulated margin, for every walker
    without a near decision."""
    from dynesty_amd import _lib
    c = rwalk_case(pname, opt)
    seed, seq0, off, walks = 0xDEADBEEFDEADBEEF, 2**32 - 100, 2**34 + 1, 45
    ctx = _lib.Context(0)
    ctx.set_rwalk_form(1)
    out = ctx.rwalk_batch_philox(c["prob"], c["u0"], c["frames"] if c["idx"] is not None else c["frames"][0],
                                 c["scale"], c["loglstar"], walks, seed=seed, sequence0=seq0, offset=off,
                                 axes_idx=c["idx"], ncdim=c["nc"] if c["nc"] < c["prob"].ndim else None, bc=c["bc"])
    refs, nears, du = rwalk_oracle(c, traced, seed, seq0, off, walks)
    compare_walkers(out, refs, nears, [("accept", "accept"), ("reject", "reject")], du, 1e-6, f"rwalk {pname} {opt}",
                    max_near=MAX_NEAR_CHAIN)


SLICE_CASES = [(5, True, False), (7, True, False), (9, True, False), (40, True, False)]


@pytest.mark.parametrize("ndim,principal,doubling", SLICE_CASES)
def test_slice_chains_against_the_oracle(traced, ndim, principal, doubling):
    """Principal-axes slice chains (slice_batch_philox, principal=True) against proposals_ref.pslice on the restated
    streams: LaneStream (uniforms 1 - hiprand's, the shuffle's masked-rejection intervals) where the slice entry point
    has a lane kernel for the dimension, WaveStream where it sends the call to the wave-per-walker kernel (n = 7 and 9
    have no lane instantiation; see slice_has_lane_kernel).  These chains draw no normals, so they are exact up to the likelihood's rounding: counts exact, u to
    1e-12."""
    from dynesty_amd import problems
    from oracle import proposals_ref as P
    prob = problems.gauss_iid(ndim, 10.0, f"ball{ndim}")
    loglstar = float(prob.like_par[0] - 0.5 * 4.0)
    ru = 2.0 / 20.0
    k = 300
    rng = np.random.default_rng(ndim)
    u0 = 0.5 + rng.uniform(-0.3, 0.3, size=(k, ndim)) * ru / np.sqrt(ndim)
    q, _ = np.linalg.qr(rng.standard_normal((ndim, ndim)))
    axes = q * ru * rng.uniform(0.3, 0.8, size=ndim)
    slices = 4 if ndim <= 32 else 2
    seed, seq0, off = 0x0123456789ABCDEF, 2**32 - 7, (3 << 24) + 1
    out = _ctx().slice_batch_philox(prob, u0, axes, 1.0, loglstar, slices, seed=seed, sequence0=seq0, offset=off,
                                    principal=principal, doubling=doubling)
    ax2 = np.linalg.norm(axes, 2)
    du = 1e-12 if principal else slices * 64 * ax2 * np.sqrt(ndim) * NORMAL_BOUND
    fn = P.pslice if principal else P.rslice
    refs, nears = [], []
    for i in range(k):
        m = traced(prob, loglstar, du)
        st = (PR.LaneStream(seed, seq0 + i, off, flip=True, normal_mode="cached") if slice_has_lane_kernel(ndim)
              else PR.WaveStream(seed, seq0 + i, off))
        r = fn(u0[i].copy(), loglstar, axes, 1.0, m.prior_transform, m.loglikelihood, st, slices, doubling=doubling)
        assert st.consumed < 1 << 24  # the resident loop's budget per walker and fill
        refs.append(r)
        nears.append(m.near)
    keys = [("ncalls", "ncalls"), ("n_expand", "n_expand"), ("n_contract", "n_contract")]
    compare_walkers(out, refs, nears, keys, max(du, 1e-12), 1e-9 if principal else 1e-6,
                    f"{'slice' if principal else 'rslice'} D={ndim} doubling={doubling}")


@pytest.mark.parametrize("ndim,nells", [(3, 1), (5, 1), (3, 3), (6, 2), (40, 1), (40, 2)])
def test_unif_bound_against_the_oracle(traced, monkeypatch, ndim, nells):
    """unif_batch_philox inside one or several ellipsoids against proposals_ref.unif_bound (bounding_ref sampling)
    on the restated streams: the ellipsoid pick and the 1 / q acceptance are uniforms, the point a ball draw
    (normals then the radius uniform).  Margin: a point moves by |axes|_2 sqrt(n) NORMAL_BOUND with the normals."""
    from dynesty_amd import _lib
    from oracle import bounding_ref as B
    from oracle import proposals_ref as P
    prob = gauss(ndim)
    rng = np.random.default_rng(100 + ndim + nells)
    ctrs = 0.5 + rng.uniform(-0.02, 0.02, size=(nells, ndim))
    ells = []
    for e in range(nells):
        a = rng.standard_normal((ndim, ndim))
        cov = (a @ a.T / ndim + np.eye(ndim)) * 0.03**2
        ells.append(B.make_ell(ctrs[e], cov))
    mell = B.stack_ells(ells) if nells > 1 else None
    axes = np.stack([e.axes for e in ells])
    ams = np.stack([e.am for e in ells])
    lv = np.array([e.logvol for e in ells])
    ll0 = prob.loglikelihood_many(prob.prior_transform_many(ctrs[:1] + 0.03 * rng.standard_normal((4000, ndim))))
    thr = float(np.quantile(ll0, 0.6))
    k = 300
    seed, seq0, off = 0xFFFFFFFFFFFFFFFF, 1, (5 << 24) + 3
    out = _ctx().unif_batch_philox(prob, thr, k, seed=seed, sequence0=seq0, offset=off, ctrs=ctrs, axes=axes,
                                   ams=ams, logvol_ells=lv)
    du = max(np.linalg.norm(a, 2) for a in axes) * np.sqrt(ndim) * NORMAL_BOUND
    draw = P.unif_single(ells[0]) if nells == 1 else P.unif_multi(mell)
    # the 1 / q acceptance counts the ellipsoids that hold the draw: a draw within du of a surface (|quad - 1| below
    # the first-order change 2 sqrt(quad) du / shortest axis) is a near decision too
    amin = min(float(np.sqrt(np.linalg.eigvalsh(e.cov).min())) for e in ells)
    quadforms = B.multi_quadforms

    def traced_quadforms(x, c, a):
        qf = quadforms(x, c, a)
        if np.any(np.abs(qf - 1.0) <= 2.0 * np.sqrt(np.abs(qf)) * du / amin + 1e-12):
            traced.current["m"].near = True
        return qf
    monkeypatch.setattr(B, "multi_quadforms", traced_quadforms)
    refs, nears = [], []
    for i in range(k):
        m = traced(prob, thr, du)
        # (unif_batch_philox: lane kernels up to 32 dimensions, padded; the wave-per-walker kernel above)
        st = (PR.LaneStream(seed, seq0 + i, off, flip=True, normal_mode="cached") if ndim <= 32
              else PR.WaveStream(seed, seq0 + i, off))
        r = P.unif_bound(thr, draw, m.prior_transform, m.loglikelihood, st, ndim, ndim)
        refs.append(r)
        nears.append(m.near)
    compare_walkers(out, refs, nears, [("ncalls", "ncalls")], du, 1e-6, f"unif D={ndim} nells={nells}")


# ---- (e) one resident run, event for event ------------------------------------------------------------------------
def test_resident_cube_phase_equals_its_philox_mirror(ctx):
    """ns_ensemble(rng='philox') with the first bound update beyond the run, so that every proposal comes from the
    unit-cube phase, against tests/resident_mirror.py drawing the cube tries from the restated stream keyed as ns.hip
    keys it (seed from the entropy words and the cube stage's constant, subsequence = global run * K + walker, offset
    = fill << 24).  Two shardings of the same global runs (runs 0-3 in one launch; runs 2-3 alone with first_run = 2)
    must both equal the mirror: dead slots, ln L and ncall exactly, ln Z to 1e-10."""
    from resident_mirror import mirror_run
    prob = inputs.problem("C1")
    nlive, K, dlogz, ent = 40, 8, 3.0, [0x12345678ABCD, 77]
    kw = dict(walks=10, bound="multi", dlogz=dlogz, entropy=ent, rebuild_every=1, want_samples=True,
              want_dead_logl=True, max_iter=20000, rng="philox", first_update=dict(min_ncall=10**9, min_eff=0.0))
    ra = ctx.ns_ensemble(prob, 4, nlive, K, **kw)
    rb = ctx.ns_ensemble(prob, 2, nlive, K, first_run=2, **kw)
    assert (ra["status"] == 0).all() and (rb["status"] == 0).all()
    for grun, r, i in ((1, ra, 1), (2, ra, 2), (2, rb, 0), (3, rb, 1)):
        m = mirror_run(ctx, prob, nlive, K, 10, "multi", ent, grun, dlogz, rng="philox",
                       first_update=dict(min_ncall=10**9, min_eff=0.0))
        n = int(r["niter"][i])
        assert m["done"] and m["nbound"] == 0 and m["niter"] == n, (grun, m["niter"], n)
        np.testing.assert_array_equal(r["dead_id"][i, :n], np.array(m["dead_slot"]))
        np.testing.assert_array_equal(r["dead_logl"][i, :n], np.array(m["dead_logl"]))
        assert int(r["ncall"][i]) == m["ncall"]
        assert abs(r["logz"][i] - m["logz"]) < 1e-10
        print(f"global run {grun}: {n} deaths, {m['ncall']} calls, {m['nfills']} fills equal to the mirror")
