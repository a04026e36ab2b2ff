"""Seeded inputs of the proposal-geometry checks (tests/proposal_hp_ref.py, tests/test_proposal_hp_cpu.py,
tests/test_gpu_proposal_hp.py, tools/make_golden.py proposal_hp): start points, frames, boundary conditions and
generator states for one rwalk step, for rwalk chains and for rslice / slice.  Everything is regenerated from the seed, so
tests/golden/proposal_hp.npz holds the reference's outputs only (and the constructed generator states).

An INPUT SET is what one launch reads; several entry points and kernel forms run the same set (the four-lane form,
the lane form and rwalk_propose at D = 5 all read "step/5/5/83/A"), so the reference is computed once per set.

One step (`step_sets`), 83 walkers (off the 16-per-wave and 64-per-workgroup granularity; 5 and 9 at wide D, either
side of the four-walker workgroup), three frames mixed inside every wavefront by idx = 5 i mod 3; the frame of a
walker is also its family, because the start point is the walker's own:

  group A  scale 0.7  frame 0  "today"   Q diag(0.04 sqrt(n) U(0.8, 1.6)),  u0 = clip(0.5 + 0.04 N, 1e-3, 1 - 1e-3)
                      frame 1  "long"    Q diag(U(0.3, 0.4) / 0.7): steps up to 0.4, u0 = U(0.05, 0.95); some leave the cube
                      frame 2  "kappa"   Q diag(0.3 * 1e-3^(j / (n - 1)) / 0.7): axis ratio 1e3, u0 = clip(0.5 + 0.05 N)
  group B  scale 0.7  frame 0  "late"    Q diag(1e-7 sqrt(n) U(0.8, 1.6)),  u0 = 0.3 + 1e-7 N
                      frame 1  "klate"   Q diag(1e-7 sqrt(n) 1e-3^(j / (n - 1))): axis ratio 1e3 at width 1e-7
                      frame 2  "late2"   half of frame 0 with rows and columns reversed
  group C  scale 1.0  coordinates periodic, reflective, hard, periodic, ... ; frames R Q diag(s) with R = 1 on the
                      periodic / reflective rows and 4e-3 on the hard ones (those stay inside the cube):
                      frame 0  "bc"      s = U(10, 30): excursions of tens of units, both signs
                      frame 1  "bc2"     s = -U(5, 15)
                      frame 2  "bck"     s = 30 * 1e-3^(j / (n - 1))
                      u0 = U(0.2, 0.8)

Constructed uniforms (`edge_keys`): eight walkers whose step uniform is exactly 0, 2^-53, 2^-30, 1 - 2^-53 (twice
each), on one "long" frame.  Chains: see chain_inputs.  rslice / slice: see slice_inputs.
"""
import math
import zlib

import numpy as np

from dynesty_amd import problems

K = 83
QUAD_DIMS = tuple(range(2, 33))  # the four-lane form: a multiplication chain of its own at every D
QUAD_FUSED_DIM = 13  # this D once more with the generator inside the walk kernel (set_rwalk_items(False))
QUAD_PREC_DIM = 25
LANE_DIMS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 25, 31, 32)
LANE_NC = ((5, 3), (25, 7))  # ncdim < ndim: lane form only
PROPOSE_DIMS = (5, 25)
WIDE_DIMS = (33, 40, 64, 65, 128, 200, 257, 512)
WIDE_K = (5, 9)
GROUPS = ("A", "B", "C")
FAMILIES = {"A": ("today", "long", "kappa"), "B": ("late", "klate", "late2"), "C": ("bc", "bc2", "bck")}
SCALE = {"A": 0.7, "B": 0.7, "C": 1.0}
EDGE_DIMS = (2, 5, 25, 32, 40)
EDGE_TARGETS = (0, 1, 1 << 23, (1 << 53) - 1)  # the uniform's 53 random bits: ur = bits * 2^-53
EDGE_K = 8

BC_HARD, BC_PERIODIC, BC_REFLECT = 0, 1, 2  # include/dynhip.h DH_BC_*


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) + 0x5EED


def _rot(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return q


def _geo(n, ratio=1e-3):
    return ratio ** (np.arange(n) / (n - 1.0)) if n > 1 else np.ones(1)


def bc_of(d):
    return np.array([(BC_PERIODIC, BC_REFLECT, BC_HARD)[i % 3] for i in range(d)], dtype=np.int8)


def frames(group, nc, d, rng):
    """(3, nc, nc) frames of a group; see the module docstring."""
    sq = math.sqrt(nc)
    if group == "A":
        f0 = _rot(rng, nc) * (0.04 * sq * rng.uniform(0.8, 1.6, nc))
        f1 = _rot(rng, nc) * (rng.uniform(0.3, 0.4, nc) / 0.7)
        f2 = _rot(rng, nc) * (0.3 * _geo(nc) / 0.7)
    elif group == "B":
        f0 = _rot(rng, nc) * (1e-7 * sq * rng.uniform(0.8, 1.6, nc))
        f1 = _rot(rng, nc) * (1e-7 * sq * _geo(nc))
        f2 = 0.5 * f0[::-1, ::-1].copy()
    else:
        rows = np.where(bc_of(d)[:nc] == BC_HARD, 4e-3, 1.0)[:, None]
        f0 = rows * (_rot(rng, nc) * rng.uniform(10.0, 30.0, nc))
        f1 = rows * (_rot(rng, nc) * -rng.uniform(5.0, 15.0, nc))
        f2 = rows * (_rot(rng, nc) * (30.0 * _geo(nc)))
    return np.ascontiguousarray(np.stack([f0, f1, f2]))


def start_points(group, k, d, idx, rng):
    if group == "A":
        today = np.clip(0.5 + 0.04 * rng.standard_normal((k, d)), 1e-3, 1 - 1e-3)
        far = rng.uniform(0.05, 0.95, (k, d))
        kap = np.clip(0.5 + 0.05 * rng.standard_normal((k, d)), 1e-3, 1 - 1e-3)
        return np.where((idx == 0)[:, None], today, np.where((idx == 1)[:, None], far, kap))
    if group == "B":
        return 0.3 + 1e-7 * rng.standard_normal((k, d))
    return rng.uniform(0.2, 0.8, (k, d))


def child_states(entropy, k):
    """(k, 4) uint64 {state_hi, state_lo, inc_hi, inc_lo} of PCG64(SeedSequence(entropy).spawn(k)[i]): what
    Context.seed_children(entropy, 0, k) computes on the device (held bit for bit by tests/test_gpu_rng.py)."""
    out = np.empty((k, 4), dtype=np.uint64)
    for i, kid in enumerate(np.random.SeedSequence(entropy).spawn(k)):
        out[i] = state_words(np.random.PCG64(kid))
    return out


def state_words(bitgen):
    s, inc = bitgen.state["state"]["state"], bitgen.state["state"]["inc"]
    m = (1 << 64) - 1
    return np.array([s >> 64, s & m, inc >> 64, inc & m], dtype=np.uint64)


def generator_of(words):
    """A numpy Generator positioned at four state words."""
    bg = np.random.PCG64(0)
    st = bg.state
    w = [int(x) for x in words]
    st["state"]["state"] = (w[0] << 64) | w[1]
    st["state"]["inc"] = (w[2] << 64) | w[3]
    st["has_uint32"], st["uinteger"] = 0, 0
    bg.state = st
    return np.random.Generator(bg)


# ---------------------------------------------------------------------------------------------------------
# one step
# ---------------------------------------------------------------------------------------------------------
def step_sets():
    """[(key, d, nc, k, group)]: every input set of the one-step checks."""
    dims = sorted(set(QUAD_DIMS) | set(LANE_DIMS) | set(PROPOSE_DIMS))
    sets = [(d, d, K) for d in dims] + [(d, nc, K) for d, nc in LANE_NC]
    sets += [(d, d, k) for d in WIDE_DIMS for k in WIDE_K]
    out = []
    for d, nc, k in sets:
        for g in GROUPS:
            if k == WIDE_K[0] and g != "A":
                continue  # the five-walker launch once per D
            out.append((f"step/{d}/{nc}/{k}/{g}", d, nc, k, g))
    return out


def step_key(d, nc, k, group):
    return f"step/{d}/{nc}/{k}/{group}"


def step_entries():
    """[(entry, key)]: which entry point / kernel form runs which input set.
    entry: quad (four lanes per walker), quadf (the same with the generator inside the kernel), quadprec (the same
    set through the precision-matrix problem: the KIND_PREC_AFFINE, R1 instance of the benchmark), lane, propose
    (rwalk_propose: the lane kernel's propose-only path), wide."""
    out = []
    for g in GROUPS:
        out += [("quad", step_key(d, d, K, g)) for d in QUAD_DIMS]
        out.append(("quadf", step_key(QUAD_FUSED_DIM, QUAD_FUSED_DIM, K, g)))
        out.append(("quadprec", step_key(QUAD_PREC_DIM, QUAD_PREC_DIM, K, g)))
        out += [("lane", step_key(d, d, K, g)) for d in LANE_DIMS]
        out += [("lane", step_key(d, nc, K, g)) for d, nc in LANE_NC]
        out += [("propose", step_key(d, d, K, g)) for d in PROPOSE_DIMS]
        out += [("wide", step_key(d, d, WIDE_K[1], g)) for d in WIDE_DIMS]
    out += [("wide", step_key(d, d, WIDE_K[0], "A")) for d in WIDE_DIMS]
    return out


_cache = {}


def step_inputs(key):
    if key in _cache:
        return _cache[key]
    _, d, nc, k, group = key.split("/")
    d, nc, k = int(d), int(nc), int(k)
    rng = np.random.default_rng(_seed(key))
    idx = (np.arange(k) * 5 % 3).astype(np.int32)
    inp = dict(key=key, d=d, nc=nc, k=k, group=group, idx=idx, axes=frames(group, nc, d, rng),
               u0=np.ascontiguousarray(start_points(group, k, d, idx, rng)), scale=SCALE[group],
               bc=bc_of(d) if group == "C" else None, walks=1, loglstar=-1e300,
               states=child_states([d, nc, k, GROUPS.index(group), 20241], k),
               problem=problems.gauss_iid(d, 6.0, f"iid{d}"))
    _cache[key] = inp
    return inp


# ---------------------------------------------------------------------------------------------------------
# constructed uniforms
# ---------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1
_M128 = (1 << 128) - 1


def _rotl(x, r):
    r &= 63
    return ((x << r) | (x >> (64 - r))) & _M64 if r else x


def construct_state(d, bits, rng):
    """Four state words from which standard_normal(d) and then random() return bits * 2^-53 exactly.

    PCG64's output is rotr(hi ^ lo, hi >> 58) of the state AFTER the step, so a state with a chosen output `out` is
    any hi with lo = hi ^ rotl(out, hi >> 58).  That state is written into a generator and taken back d + 1 steps;
    if every normal of the d takes one draw (the ziggurat's common case, 98.9 % each) the uniform lands on it.
    Otherwise another hi is drawn.  Returns (words, tries)."""
    out = (bits << 11) | 0x2A5  # random() drops the low 11 bits
    for tries in range(1, 200):
        hi = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        lo = hi ^ _rotl(out, hi >> 58)
        bg = np.random.PCG64(int(rng.integers(0, 1 << 62)))
        st = bg.state
        st["state"]["state"] = (hi << 64) | lo
        st["has_uint32"], st["uinteger"] = 0, 0
        bg.state = st
        bg.advance((-(d + 1)) & _M128)
        words = state_words(bg)
        g = np.random.Generator(bg)
        g.standard_normal(d)
        if g.random() == bits * 2.0**-53:
            return words, tries
    raise RuntimeError("no state found")


def edge_keys():
    return [f"edge/{d}" for d in EDGE_DIMS]


def edge_entries():
    out = []
    for d in EDGE_DIMS:
        out += [("wide", f"edge/{d}")] if d > 32 else [("quad", f"edge/{d}"), ("lane", f"edge/{d}")]
    return out


def edge_targets():
    return np.array([EDGE_TARGETS[i % 4] for i in range(EDGE_K)], dtype=np.uint64)


def edge_inputs(key, states=None):
    """states: the fixture's (EDGE_K, 4) words; None constructs them (the generator, and the CPU test that holds the
    fixture to the construction)."""
    d = int(key.split("/")[1])
    rng = np.random.default_rng(_seed(key))
    f1 = _rot(rng, d) * (rng.uniform(0.3, 0.4, d) / 0.7)
    u0 = rng.uniform(0.3, 0.7, (EDGE_K, d))
    tries = None
    if states is None:
        got = [construct_state(d, int(b), rng) for b in edge_targets()]
        states = np.array([w for w, _ in got], dtype=np.uint64)
        tries = max(t for _, t in got)
    return dict(key=key, d=d, nc=d, k=EDGE_K, group="edge", idx=np.zeros(EDGE_K, dtype=np.int32),
                axes=np.ascontiguousarray(f1[None]), u0=np.ascontiguousarray(u0), scale=0.7, bc=None, walks=1,
                loglstar=-1e300, states=np.ascontiguousarray(states, dtype=np.uint64), tries=tries,
                problem=problems.gauss_iid(d, 6.0, f"iid{d}"))


# ---------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------
# (D, problem kind, steps): D = 25 with 45 steps is the R1 instance of the four-lane kernel (the benchmark's)
CHAIN_PROBLEMS = ((25, "prec", 45), (2, "egg", 18), (7, "iid", 18), (12, "normal", 18), (32, "prec", 18))
CHAIN_WIDE = (40, "normal", 10)
CHAIN_BC = (8, "prec", 20)
CAP = 0.02  # at most this share of a case's walkers may have an undecidable decision


def the_problem(kind, d):
    if kind == "prec":
        return problems.gauss_corr(d, 0.4, 5.0, f"corr{d}")
    if kind == "iid":
        return problems.gauss_iid(d, 6.0, f"iid{d}")
    if kind == "normal":
        return problems.gauss_normal_prior(d, f"nprior{d}")
    return problems.eggbox(d, name=f"egg{d}")


def chain_keys():
    out = []
    for d, kind, walks in CHAIN_PROBLEMS + (CHAIN_WIDE,):
        out += [f"chain/{d}/{kind}/{walks}/{fam}" for fam in ("T", "E")]
    d, kind, walks = CHAIN_BC
    out.append(f"chain/{d}/{kind}/{walks}/BC")
    return out


def chain_entries():
    out = []
    for key in chain_keys():
        d = int(key.split("/")[1])
        if d > 32:
            out.append(("wide", key))
        else:
            out += [("quad", key), ("lane", key)]
    return out


def chain_inputs(key):
    """T: the frames of tests/test_gpu_rwalkq.py (start points of width `spread` about 0.5, an orthogonal frame times
    0.8 ... 1.6), with an axis-ratio-1e3 frame and the transpose mixed in.  E: a cloud of width 1e-7 about 0.3 with
    frames of that width (one of axis ratio 1e3).  BC: the T cloud with a frame twice as long and periodic /
    reflective / hard coordinates.  loglstar is the 5 % quantile of the cloud's own ln L, and the walkers are the
    first 83 (9 at wide D) above it."""
    if key in _cache:
        return _cache[key]
    _, d, kind, walks, fam = key.split("/")
    d, walks = int(d), int(walks)
    prob = the_problem(kind, d)
    rng = np.random.default_rng(_seed(key))
    k = WIDE_K[1] if d > 32 else K
    n0 = k + 40
    if kind == "normal":
        spread = 0.08
    elif kind == "egg":
        spread = 0.004
    else:
        spread = 0.5 / (2 * prob.prior_par[0])
    sq = math.sqrt(d)
    if fam == "E":
        u0 = 0.3 + 1e-7 * rng.standard_normal((n0, d))
        f0 = _rot(rng, d) * (1e-7 * sq * rng.uniform(0.8, 1.6, d))
        axes = np.stack([f0, _rot(rng, d) * (1e-7 * sq * 1.6 * _geo(d)), 0.5 * f0[::-1, ::-1].copy()])
    else:
        u0 = np.clip(0.5 + spread * rng.standard_normal((n0, d)), 1e-3, 1 - 1e-3)
        f0 = _rot(rng, d) * (spread * sq * rng.uniform(0.8, 1.6, d))
        axes = np.stack([f0, _rot(rng, d) * (spread * sq * 1.6 * _geo(d)), 0.8 * f0.T.copy()])
        if fam == "BC":
            axes = 2.0 * axes
    logl = prob.loglikelihood_many(prob.prior_transform_many(u0))
    loglstar = float(np.quantile(logl, 0.05))
    u0 = np.ascontiguousarray(u0[logl > loglstar][:k])
    assert len(u0) == k
    inp = dict(key=key, d=d, nc=d, k=k, group=fam, idx=(np.arange(k) * 5 % 3).astype(np.int32),
               axes=np.ascontiguousarray(axes), u0=u0, scale=0.7, bc=bc_of(d) if fam == "BC" else None, walks=walks,
               loglstar=loglstar, states=child_states([d, walks, ("T", "E", "BC").index(fam), 20242], k), problem=prob)
    _cache[key] = inp
    return inp


# ---------------------------------------------------------------------------------------------------------
# rslice / slice
# ---------------------------------------------------------------------------------------------------------
# (form, D, problem kind, slices): r = rslice (random directions), p = slice (principal axes in shuffled order)
SLICE_PROBLEMS = (("r", 5, "prec", 3), ("r", 9, "iid", 3), ("p", 5, "prec", 3), ("p", 7, "egg", 3))
SLICE_WIDE = ("r", 40, "normal", 2)
SLICE_LATE = (("r", 5, "iid", 3), ("p", 5, "iid", 3))
LATE_HALFWIDTH = 1e7  # a unit Gaussian in v under a prior of this half-width is 5e-8 wide in u


def slice_keys():
    out = []
    for form, d, kind, slices in SLICE_PROBLEMS:
        out += [f"slice/{form}/{d}/{kind}/{slices}/{dbl}/T" for dbl in (0, 1)]
    form, d, kind, slices = SLICE_WIDE
    out.append(f"slice/{form}/{d}/{kind}/{slices}/0/T")
    out += [f"slice/{form}/{d}/{kind}/{slices}/0/E" for form, d, kind, slices in SLICE_LATE]
    return out


def feed_keys():
    """slice_feed's directions on the frames and streams of these slice cases."""
    return ["slice/r/5/prec/3/0/T", "slice/r/9/iid/3/0/T", "slice/r/40/normal/2/0/T", "slice/r/5/iid/3/0/E"]


def slice_inputs(key):
    """T: the cloud and frame of chain_inputs' T, with an axis-ratio-1e3 frame and a frame of length 30 mixed in --
    its directions are longer than sqrt(n) / 2 and are renormalised (internal_samplers.py:1098-1101).
    E: a unit Gaussian under a prior of half-width 1e7: cloud, frames and slices of width 1e-7 about 0.5 (a slice
    needs a likelihood contour of that width to stop at; the rwalk chains' 1e-7 cloud about 0.3 sees a half-space)."""
    if key in _cache:
        return _cache[key]
    _, form, d, kind, slices, dbl, fam = key.split("/")
    d, slices = int(d), int(slices)
    rng = np.random.default_rng(_seed(key))
    k = WIDE_K[1] if d > 32 else K
    n0 = k + 40
    if fam == "E":
        prob = problems.gauss_iid(d, LATE_HALFWIDTH, f"iid{d}late")
        spread = 0.5 / (2 * LATE_HALFWIDTH)
    else:
        prob = the_problem(kind, d)
        spread = 0.08 if kind == "normal" else 0.004 if kind == "egg" else 0.5 / (2 * prob.prior_par[0])
    sq = math.sqrt(d)
    u0 = np.clip(0.5 + spread * rng.standard_normal((n0, d)), 1e-3, 1 - 1e-3)
    f0 = _rot(rng, d) * (spread * sq * rng.uniform(0.8, 1.6, d))
    # stepping out along a principal axis 1e3 times shorter than the contour takes a thousand expansions and sets the
    # expansion warning: that form gets an axis ratio of 30, the doubling one and the random directions 1e3
    ratio = 1.0 / 30.0 if form == "p" and dbl == "0" else 1e-3
    axes = np.stack([f0, _rot(rng, d) * (spread * sq * 1.6 * _geo(d, ratio)), _rot(rng, d) * 30.0])
    logl = prob.loglikelihood_many(prob.prior_transform_many(u0))
    loglstar = float(np.quantile(logl, 0.05))
    u0 = np.ascontiguousarray(u0[logl > loglstar][:k])
    assert len(u0) == k
    inp = dict(key=key, d=d, nc=d, k=k, group=fam, idx=(np.arange(k) * 5 % 3).astype(np.int32),
               axes=np.ascontiguousarray(axes), u0=u0, scale=0.7, bc=None, slices=slices, loglstar=loglstar,
               principal=form == "p", doubling=dbl == "1",
               states=child_states([d, slices, int(dbl), ("T", "E").index(fam), int(form == "p"), 20243], k), problem=prob)
    _cache[key] = inp
    return inp


# ---------------------------------------------------------------------------------------------------------
# draws inside ellipsoids
# ---------------------------------------------------------------------------------------------------------
DRAW_N = 83


def draw_keys():
    """unif: unif_batch, one walker per generator (unif_kernel; wide_unif_kernel at D = 40); bound: bound_draw, 83
    draws off one generator; multi: bound_draw over three overlapping ellipsoids with the membership counts;
    unifmulti: unif_batch over the same three ellipsoids (choice, draw, acceptance with probability 1 / q).
    The ellipsoids depend on the dimension and their number alone: unif and bound share theirs, and so do multi and
    unifmulti."""
    return ["draw/unif/3", "draw/unif/25", "draw/unif/40", "draw/bound/3", "draw/bound/25", "draw/multi/5",
            "draw/unifmulti/5"]


def draw_inputs(key):
    """ctr + A (z ur^(1/n) / |z|) is one rwalk step from the centre with scale 1, so a draw is stated as a walker of
    a one-step input set: u0 the centre of its ellipsoid, idx the ellipsoid, `states` the generator in front of its
    normals.  Every ellipsoid lies inside the cube (centres within 0.06 of 1/2, axes up to 0.3).  For bound_draw the
    states are the successive states of ONE generator (state0), walked here with NumPy: a draw from three
    ellipsoids first takes the uniform that chooses one (rand_choice, bounding.py:1300-1308)."""
    if key in _cache:
        return _cache[key]
    from scipy.special import logsumexp
    _, kind, d = key.split("/")
    d = int(d)
    m = 3 if kind in ("multi", "unifmulti") else 1
    rng = np.random.default_rng(_seed("draw", "ellipsoids", d, m))
    k = WIDE_K[1] if d > 32 else DRAW_N
    ctrs = np.clip(0.5 + 0.02 * rng.standard_normal((m, d)), 0.44, 0.56)
    lens = rng.uniform(0.05, 0.3, (m, d)) if m == 1 else rng.uniform(0.1, 0.25, (m, d))
    rots = [_rot(rng, d) for _ in range(m)]
    axes = np.ascontiguousarray(np.stack([rots[j] * lens[j] for j in range(m)]))
    ams = np.stack([(rots[j] / lens[j]**2) @ rots[j].T for j in range(m)])
    ams = np.ascontiguousarray(0.5 * (ams + ams.transpose(0, 2, 1)))
    lv = np.log(lens).sum(axis=1)
    cumprob = np.cumsum(np.exp(lv - logsumexp(lv)))
    idx = np.zeros(k, dtype=np.int32)
    state0 = start = end = None
    if kind == "unif":
        states = child_states([d, 77, 20244], k)
    elif kind == "unifmulti":
        # UniformBoundSampler.sample over MultiEllipsoid.sample (bounding.py:525-590) walked with NumPy per walker:
        # choose, draw, count the ellipsoids that hold the point, keep it with probability 1 / q.  The walker of the
        # one-step set is the draw that was kept; `start` is where its generator begins and `end` where it stops.
        # Every membership of every draw, kept or not, is 1e-9 or more from the boundary: q is no matter of rounding.
        start = child_states([d, 78, 20244], k)
        states, end = np.empty((k, 4), dtype=np.uint64), np.empty((k, 4), dtype=np.uint64)
        redrawn = shared = 0
        for i in range(k):
            g = generator_of(start[i])
            while True:
                c = g.random()
                assert np.min(np.abs(cumprob - c)) > 1e-12
                j = min(np.searchsorted(cumprob, c), m - 1)
                st = state_words(g.bit_generator)
                z = g.standard_normal(d)
                x = ctrs[j] + axes[j] @ (z * (g.random()**(1.0 / d) / np.linalg.norm(z)))
                quad = np.einsum('ai,aij,aj->a', x - ctrs, ams, x - ctrs)
                assert np.min(np.abs(quad - 1.0)) > 1e-9
                q = int((quad < 1).sum())
                assert q >= 1
                if q == 1 or g.random() < 1.0 / q:
                    break
                redrawn += 1
            shared += q > 1
            idx[i], states[i], end[i] = j, st, state_words(g.bit_generator)
        assert redrawn >= 5 and shared >= 5  # the 1 / q loop both rejects and accepts
    else:
        bg = np.random.PCG64(_seed(key, "stream"))
        g = np.random.Generator(bg)
        state0 = state_words(bg)
        states = np.empty((k, 4), dtype=np.uint64)
        for i in range(k):
            if m > 1:
                c = g.random()
                assert np.min(np.abs(cumprob - c)) > 1e-12  # the choice is not a matter of rounding
                idx[i] = min(np.searchsorted(cumprob, c), m - 1)
            states[i] = state_words(bg)
            g.standard_normal(d)
            g.random()
    inp = dict(key=key, d=d, nc=d, k=k, group="draw", idx=idx, axes=axes, u0=np.ascontiguousarray(ctrs[idx]),
               scale=1.0, bc=None, walks=1, loglstar=-1e300, states=states, state0=state0, start=start, end=end, ctrs=ctrs, ams=ams,
               logvol_ells=lv, kind=kind, problem=problems.gauss_iid(d, 6.0, f"iid{d}"))
    _cache[key] = inp
    return inp
