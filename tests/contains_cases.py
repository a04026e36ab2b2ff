"""Seeded inputs for the membership kernels' high-precision tests (tests/contains_hp_ref.py): ellipsoids, points placed in
shells next to their boundaries, exactly representable cases, a NaN point, and whole run-wise launches.  Everything is
regenerated from a seed; nothing is read from a file.

Families of ellipsoids (centres within 0.06 of 1/2 unless stated):
  round    a random rotation times lengths U(0.05, 0.3)
  kappa    axis ratio 1e3: the precision matrix has condition 1e6 and S is about 2e5 on the surface
  late     a cloud of width 1e-7 about 0.3: entries of A about 1e14, x - c exact
  multi3   three overlapping `round` ellipsoids about a common point (cluster), with a ladder of points that are
           in exactly 3, 2, 1 and 0 of them
  multi17  seventeen of them (mask rows)

Shells.  B_e is the largest bound over 64 points of ellipsoid e's surface.  Points x = c + axes z with |z|^2 = 1 + delta
for delta = +-1e-3, +-64 B_e, +-8 B_e (decidable) and +-B_e / 8 (undecidable on purpose), plus bulk points well inside
and well outside.  The float64 grid is coarse next to B_e in low dimensions (one ulp of a coordinate moves q by
2 |(A dl)_j| ulp), so each point is the best of a few candidates jittered by some ulp per coordinate: the one nearest
its target that is on the right side and decidable (the +-B_e / 8 shell: within its bound).  Where no candidate of the
+-B_e / 8 shell comes that near -- the `late` family, whose grid moves q by 1e-9 a step, and the one axis of 3e-4 of
`kappa` at d = 1 -- the point is left out.

Exact cases: dyadic centre, offsets and diagonal A, every operation exact in any order and q == 1; neighbours one ulp of
the last offset coordinate inside and outside.  The neighbours' q is NOT exact (at d = 1, (1 - 2^-52)^2 needs 104 bits):
their one inexact term is a single product, and adding the other, dyadic terms to it before or after its rounding gives
the same float64, so every evaluation rounds identically (tests/test_contains_hp_cpu.py runs three orders) and they are
held to that value as well.  The centre is 2 (d >= 2) so that this ulp moves q by 2^-51 or more: one ulp at a centre of
1/2 would give q = 1 + 2^-52, whose correctly rounded square root is 1, which mode 1 calls inside."""
import functools
import zlib

import numpy as np

import contains_hp_ref as H

LD = np.longdouble
NARROW_D = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21, 25, 26, 32)
WIDE_D = (33, 64, 65, 200, 257, 512)
DECIDABLE_SHELLS = ("+1e-3", "-1e-3", "+64B", "-64B", "+8B", "-8B")
UNDECIDABLE_SHELLS = ("+B/8", "-B/8")
BULK = ("in", "out")


def _seed(*key):
    return zlib.crc32(repr(key).encode())


# ---- ellipsoids -----------------------------------------------------------------------------------------------------
def ellipsoid(kind, d, rng):
    """(centre, axes, A): the columns of `axes` are the semi-axes, A the float64 precision matrix (symmetric), an exact
    datum from there on."""
    rot = np.linalg.qr(rng.standard_normal((d, d)))[0]
    if kind == "round":
        ctr, lens = 0.5 + rng.uniform(-0.06, 0.06, d), rng.uniform(0.05, 0.3, d)
    elif kind == "kappa":
        ctr, lens = 0.5 + rng.uniform(-0.06, 0.06, d), 0.3 * np.logspace(-3, 0, d)  # (d = 1: one axis of 3e-4)
    elif kind == "late":
        ctr, lens = 0.3 + rng.uniform(-1e-7, 1e-7, d), rng.uniform(0.5e-7, 1e-7, d)
    else:
        raise ValueError(kind)
    am = (rot / lens**2) @ rot.T
    return ctr, rot * lens, 0.5 * (am + am.T)


def _place(ctr, axes, am, z, rng, ncand):
    """Candidates next to c + axes z: the point itself and ncand - 1 neighbours a few ulp away per coordinate."""
    base = ctr + axes @ z
    cand = np.repeat(base[None], ncand, axis=0)
    if ncand > 1:
        cand[1:] += np.spacing(base) * rng.integers(-4, 5, size=(ncand - 1, len(base)))
    q, s = H.quad_hp(cand, ctr[None], am[None])
    return cand, q[:, 0], H.quad_bound(len(base), s[:, 0])


def surface_bound(ctr, axes, am, rng):
    """B_e: the largest bound over 64 points of the surface."""
    d = len(ctr)
    z = rng.standard_normal((64, d))
    z /= np.linalg.norm(z, axis=1)[:, None]
    dl = np.abs(z @ axes.T)  # (a placement scale, not a test's bound: float64 serves)
    return float(H.coeff(d)) * float(np.max(np.sum(dl * (dl @ np.abs(am)), axis=1)))


def cluster(kinds, d, rng):
    """Overlapping ellipsoids: each holds one common point (within 0.06 of 1/2) 0.3 of the way out from its centre, so
    that they overlap at every d (independent centres lie far outside one another at wide d)."""
    ells = [ellipsoid(kind, d, rng) for kind in kinds]
    if len(ells) == 1:
        return ells, ells[0][0]
    common = 0.5 + rng.uniform(-0.06, 0.06, d)
    out = []
    for _, axes, am in ells:
        z = rng.standard_normal(d)
        out.append((common + axes @ (0.3 * z / np.linalg.norm(z)), axes, am))
    return out, common


def ladder(ells, common, rng):
    """Points along a ray from the common point, one between every two consecutive exits: counts m, m - 1, .., 0."""
    d = len(common)
    u = rng.standard_normal(d)
    u *= 0.01 / np.linalg.norm(u)
    exits = []
    for ctr, _, am in ells:  # q(common + t u) = 1, the positive root
        p = common - ctr
        a, b, c = u @ am @ u, 2 * (u @ am @ p), p @ am @ p - 1
        exits.append((-b + np.sqrt(b * b - 4 * a * c)) / (2 * a))
    t = np.sort(exits)
    mids = np.concatenate([[t[0] / 2], (t[1:] + t[:-1]) / 2, [2 * t[-1]]])
    return [common + ti * u for ti in mids]


def shell_point(ctr, axes, am, be, shell, rng):
    """One point of a shell of ellipsoid (ctr, axes, am), or None where the float64 grid has none (see above)."""
    d = len(ctr)
    ncand = 128 if d <= 8 else (32 if d <= 32 else 3)
    z = rng.standard_normal(d)
    z /= np.linalg.norm(z)
    if shell == "in":
        return ctr + axes @ (z * np.sqrt(rng.uniform(0.0, 0.6)))
    if shell == "out":
        return ctr + axes @ (z * np.sqrt(rng.uniform(1.5, 9.0)))
    sign = 1.0 if shell[0] == "+" else -1.0
    delta = sign * {"1e-3": 1e-3, "64B": 64 * be, "8B": 8 * be, "B/8": be / 8}[shell[1:]]
    # the float64 A is not the inverse of axes axes^T to the last bit: rescale the ray so that q_hp hits the target
    _, q0, _ = _place(ctr, axes, am, z, rng, 1)
    z = z * float(np.sqrt((1 + LD(delta)) / q0[0]))
    cand, q, b = _place(ctr, axes, am, z, rng, ncand)
    off = (q - 1).astype(np.float64)
    if shell in UNDECIDABLE_SHELLS:
        ok = np.abs(q - 1) <= b
    else:
        ok = (np.sign(off) == sign) & (np.abs(q - 1) > 2 * b)
    if not ok.any():
        if shell in UNDECIDABLE_SHELLS:
            return None
        raise RuntimeError(f"no float64 point in shell {shell} at d = {d}")
    pick = np.flatnonzero(ok)[np.argmin(np.abs(off[ok] - delta))]
    return cand[pick]


# ---- dh_contains cases ----------------------------------------------------------------------------------------------
FAMILIES = {"round": ("round",), "kappa": ("kappa",), "late": ("late",), "multi3": ("round",) * 3, "multi17": ("round",) * 17}


@functools.lru_cache(maxsize=None)
def case(family, d, nan=True):
    """dict(x (k, d), ctrs (m, d), ams (m, d, d), shell (k,) names, own (k,) the ellipsoid a point was placed at,
    q, bound (k, m) long double).  The last point has a NaN coordinate (shell "nan", own -1)."""
    rng = np.random.default_rng(_seed("contains", family, d))
    ells, common = cluster(FAMILIES[family], d, rng)
    m = len(ells)
    per = 1 if m == 17 else (3 if d <= 32 else (5 if m == 1 else 2))
    xs, shells, own = [], [], []
    for e, (ctr, axes, am) in enumerate(ells):
        be = surface_bound(ctr, axes, am, rng)
        for shell in DECIDABLE_SHELLS + UNDECIDABLE_SHELLS + BULK:
            for _ in range(per if shell not in BULK else max(per, 2)):
                p = shell_point(ctr, axes, am, be, shell, rng)
                if p is not None:
                    xs.append(p), shells.append(shell), own.append(e)
    if m > 1:
        for p in ladder(ells, common, rng):
            xs.append(p), shells.append("ladder"), own.append(-1)
    if nan:
        p = np.array(xs[0])
        p[d // 2] = np.nan
        xs.append(p), shells.append("nan"), own.append(-1)
    order = rng.permutation(len(xs) - 1) if nan else rng.permutation(len(xs))  # shells mixed within a wavefront
    if nan:
        order = np.append(order, len(xs) - 1)
    x = np.array(xs)[order]
    ctrs, ams = np.array([e[0] for e in ells]), np.array([e[2] for e in ells])
    q, bound = H.reference(x, ctrs, ams)
    for a in (x, ctrs, ams, q, bound):
        a.setflags(write=False)
    return dict(name=f"{family}/d{d}", x=x, ctrs=ctrs, ams=ams, shell=np.array(shells)[order], own=np.array(own)[order],
                q=q, bound=bound)


def own_pairs(c, shells):
    """(rows, columns) of the pairs (point, the ellipsoid it was placed at) of the given shells."""
    rows = np.flatnonzero(np.isin(c["shell"], shells) & (c["own"] >= 0))
    return rows, c["own"][rows]


def exact_case(d):
    """The exactly representable case of dimension d: x (3, d) -- q == 1, one ulp inside, one ulp outside --, ctrs
    (1, d), ams (1, d, d), q (3, 1) long double, bound 0: q[0] is exact; the neighbours' q rounds to the same float64 in
    every order of evaluation (module docstring), and the long double's value is that float64."""
    if d == 1:
        ctr, am, off = np.array([0.5]), np.eye(1), {0: 1.0}
    elif d == 2:
        ctr, am, off = np.full(2, 2.0), 2 * np.eye(2), {0: 0.5, 1: 0.5}
    elif d == 3:
        ctr, am, off = np.full(3, 2.0), np.diag([1.0, 1.0, 2.0]), {0: 0.5, 1: 0.5, 2: 0.5}
    else:
        ctr, am, off = np.full(d, 2.0), np.eye(d), {0: 0.5, 1: 0.5, d - 2: 0.5, d - 1: 0.5}
    on = ctr.copy()
    for i, o in off.items():
        on[i] += o
    inside, outside = on.copy(), on.copy()
    inside[d - 1] = np.nextafter(on[d - 1], ctr[d - 1])
    outside[d - 1] = np.nextafter(on[d - 1], np.inf)
    x = np.array([on, inside, outside])
    q, bound = H.reference(x, ctr[None], am[None], exact=np.ones(3, dtype=bool))
    return dict(name=f"exact/d{d}", x=x, ctrs=ctr[None], ams=am[None], q=q, bound=bound)


# ---- run-wise launches ----------------------------------------------------------------------------------------------
MAX_ELLS = 4
NELLS = (1, 2, 3, 4, 2, 4, 3)
RUN_MODE = (0, 0, 0, 1, 0, 0, 0)  # my_mode = 0: run 3 is masked by its mode
BSTATUS = (0, 0, 0, 0, 5, 0, 0)   # run 4 is masked by its bound's status
FLAG_IN = (0, 4, 2, 6, 9, 0, 8)   # upper bits that must survive; the masked runs' words come back as they are
FIRST_BIG = 1 << 20


def _outside_all(p, ells, strict):
    q, b = H.reference(p[None], np.array([e[0] for e in ells]), np.array([e[2] for e in ells]))
    return bool(np.all(H.decidable(q, b) & ~H.hp_inside(q, 0 if strict else 1)))


@functools.lru_cache(maxsize=None)
def runs_case(d, wpr, single=False, undecidable=True):
    """One run-wise launch: 7 runs of wpr entries against max_ells = 4 slots.
      run 0  kappa, its only outside entry is the LAST one (+8B shell)
      run 1  outside: entry 0 (+64B) and one three quarters down the queue (far out); undecidable entries after entry 0
      run 2  every entry inside (-8B and -64B shells among them)
      run 3  masked by run_mode, run 4 masked by bstatus; both have entries outside
      run 5  entries that only the run's LAST ellipsoid holds.  Without undecidable entries: one entry outside (+8B) in
             mid-queue.  With them: entries of the +-B/8 shell, decidably outside the run's other ellipsoids, spread
             over the queue from entry 0 on -- with nells they are all that may be outside, so the kernel's own
             rounding decides flag and first; with the single bound the +8B entry stays in mid-queue and the
             undecided entries ahead of it decide first
      run 6  a NaN point in mid-queue, all else inside
    single: nells is None (every run has the one bound of slot 0), strict = 0.  The slots from nells[run] on hold an
    ellipsoid that contains everything (A = 0).  Returns dict(x, ctrs, ams, nells, strict, run_mode, bstatus, flag,
    first, q, bound (runs, wpr, 4), states (runs, wpr), served)."""
    rng = np.random.default_rng(_seed("runs", d, wpr, single, undecidable))
    R = len(NELLS)
    strict = 0 if single else 1
    ctrs, ams = np.full((R, MAX_ELLS, d), 0.5), np.zeros((R, MAX_ELLS, d, d))
    x = np.empty((R, wpr, d))
    nells = [1] * R if single else list(NELLS)
    for r in range(R):
        ells, _ = cluster(["kappa" if r == 0 else "round"] * nells[r], d, rng)
        bes = [surface_bound(*e, rng) for e in ells]
        for a, e in enumerate(ells):
            ctrs[r, a], ams[r, a] = e[0], e[2]

        def pt(shell, a=None):
            for _ in range(200):  # an outside entry has to be outside ALL of the run's ellipsoids
                e = int(rng.integers(len(ells))) if a is None else a
                p = shell_point(*ells[e], bes[e], shell, rng)
                if p is not None and (shell[0] != "+" and shell != "out" or _outside_all(p, ells, strict)):
                    return p
            raise RuntimeError(f"no {shell} entry for run {r} at d = {d}")
        near = max(3, wpr // 16)  # every near-th entry sits next to a boundary, on the inside
        for j in range(wpr):
            x[r, j] = pt(("-1e-3", "-64B", "-8B")[(j // near) % 3] if j % near == 0 else "in")
        last = len(ells) - 1
        if r == 0:
            x[r, wpr - 1] = pt("+8B")
        elif r in (1, 3, 4):
            x[r, 0] = pt("+64B")
            x[r, (3 * wpr) // 4 if wpr > 1 else 0] = pt("out")
            if undecidable and r == 1 and wpr > 2:
                for j, shell in zip(range(1, wpr, max(1, wpr // 3)), UNDECIDABLE_SHELLS * 2):
                    if j != (3 * wpr) // 4:
                        p = shell_point(*ells[0], bes[0], shell, rng)
                        x[r, j] = x[r, j] if p is None else p
        elif r == 5:
            mid = wpr // 2
            for j in range(0, wpr, max(2, wpr // 8)):  # inside the last ellipsoid only, where there is such a point
                for _ in range(20):
                    p = shell_point(*ells[last], bes[last], ("-8B", "in")[j % 4 == 0], rng)
                    if len(ells) == 1 or _outside_all(p, ells[:last], strict):
                        x[r, j] = p
                        break
            if not undecidable or single:
                x[r, mid] = pt("+8B")
            if undecidable:
                # entries of the +-B/8 shell of one ellipsoid that are decidably outside the run's others: the kernel's
                # own rounding decides them, and the run's words with them -- the flag where they are all that may be
                # outside (multi), first where they come ahead of the +8B entry (single)
                def undecided(shell):
                    for _ in range(400):
                        e = int(rng.integers(len(ells)))
                        p = shell_point(*ells[e], bes[e], shell, rng)
                        if p is not None and (len(ells) == 1 or _outside_all(p, ells[:e] + ells[e + 1:], strict)):
                            return p
                    raise RuntimeError(f"no {shell} entry outside the other ellipsoids of run {r} at d = {d}")
                for j, shell in zip(range(0, wpr, max(1, wpr // 6)), UNDECIDABLE_SHELLS * 4):
                    if j != mid:
                        x[r, j] = undecided(shell)
        elif r == 6:
            x[r, wpr // 3, d - 1] = np.nan
    q, bound = np.empty((R, wpr, MAX_ELLS), dtype=LD), np.empty((R, wpr, MAX_ELLS), dtype=LD)
    states = np.empty((R, wpr), dtype=np.int8)
    for r in range(R):
        q[r], bound[r] = H.reference(x[r], ctrs[r], ams[r])
        states[r] = H.entry_states(q[r], bound[r], nells[r], strict)
    first = np.array([FIRST_BIG, wpr, FIRST_BIG, 12345, -7, FIRST_BIG, FIRST_BIG], dtype=np.int32)
    out = dict(name=f"runs/d{d}/wpr{wpr}/{'single' if single else 'multi'}", d=d, wpr=wpr, x=x.reshape(R * wpr, d),
               ctrs=ctrs, ams=ams, nells=None if single else np.array(nells, dtype=np.int32), max_ells=MAX_ELLS,
               strict=strict, run_mode=np.array(RUN_MODE, dtype=np.int32), my_mode=0,
               bstatus=np.array(BSTATUS, dtype=np.int32), flag=np.array(FLAG_IN, dtype=np.int32), first=first, q=q,
               bound=bound, states=states, nells_eff=np.array(nells),
               served=H.served_runs(R, RUN_MODE, 0, BSTATUS))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def exact_runs_case(d, wpr, strict):
    """Run-wise form of the exact cases: run 0 holds the q == 1 point at its last entry and the inside neighbour
    elsewhere; run 1 the outside neighbour at entry wpr // 2; run 2 the inside neighbour throughout.  One ellipsoid in
    slot 0; with strict the other slots are unused (nells = 1)."""
    e = exact_case(d)
    R = 3
    ctrs, ams = np.empty((R, MAX_ELLS, d)), np.zeros((R, MAX_ELLS, d, d))
    ctrs[:] = e["ctrs"][0]
    ams[:, 0] = e["ams"][0]
    x = np.empty((R, wpr, d))
    x[:] = e["x"][1]
    x[0, wpr - 1] = e["x"][0]
    x[1, wpr // 2] = e["x"][2]
    first = np.full(R, FIRST_BIG, dtype=np.int32)
    # q == 1: strict (q < 1) says outside, sqrt(q) <= 1 says inside
    want_flag = np.array([1 if strict else 0, 1, 0], dtype=np.int32)
    want_first = np.array([wpr - 1 if strict else FIRST_BIG, wpr // 2, FIRST_BIG], dtype=np.int32)
    return dict(name=f"exact_runs/d{d}/wpr{wpr}/strict{strict}", d=d, wpr=wpr, x=x.reshape(R * wpr, d), ctrs=ctrs, ams=ams,
                nells=np.ones(R, dtype=np.int32) if strict else None, strict=strict, first=first, want_flag=want_flag,
                want_first=want_first)


# ---- the shapes of the tests ----------------------------------------------------------------------------------------
CONTAINS_NARROW = [(f, d) for d in NARROW_D for f in ("round", "kappa", "late", "multi3")] + [("multi17", 5), ("multi17", 25)]
CONTAINS_WIDE = [(f, d) for d in WIDE_D for f in ("round", "kappa", "multi3")]
# (d, wpr, DH_CONTAINS_LDS): the scalar form -- several runs per wavefront (5), whole wavefronts (64), runs that straddle
# them (83), queues of a multiple of 256 below the LDS form's d >= 9 and with the LDS form switched off
RUNS_SCALAR = ([(d, wpr, None) for d in (1, 5, 8, 13, 25, 32) for wpr in (5, 64, 83)] + [(8, 256, None)] +
               [(13, 256, "0"), (25, 256, "0")])
RUNS_LDS = [(d, wpr) for d in (9, 13, 25, 32) for wpr in (256, 512)]
# np < P throughout; tiles of 8 then 3; two chunks; P = 4 and five chunks (wavefront 0 takes two); the widest
RUNS_WIDE = [(33, 5), (64, 11), (65, 8), (257, 6), (512, 4)]
