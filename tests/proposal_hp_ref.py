"""High-precision reference of the proposal geometry -- one rwalk step, rwalk chains, rslice / slice, the draws inside
ellipsoids -- and forward error bounds for an fp64 evaluation of it.
Plain Python: no device code, nothing in the operation order of dynesty_amd/csrc/walk.hip, walk2.hip, walkq.hip or wide.hip.

  u'_i = u_i + scale * ur^(1/n) * (A z)_i / |z|      then periodic wrap / reflection and unitcheck

z (n standard normals) and ur (one uniform) are NumPy's own Generator(PCG64) draws -- the device's streams are held
to them bit for bit by tests/test_gpu_rng.py -- so they enter as exact fp64 numbers and only the geometry is held.

  g = ur^(1/n) / |z|   mpmath, 50 digits (radius, the sum of squares, the root, the quotient)
  A z, the products with scale and g, the sum with u   np.longdouble (eps <= 2^-60 asserted by tests/hp_ref.py)

THE BOUND of one step, per coordinate i, eps = 2^-53, S_i = sum_j |A_ij| |z_j|, fac = scale g (step_coeff, step_hp):

  eps |u'_i|                      the final rounding (one fused multiply-add, or the rounding of the sum), taken
                                  before the wrap
  |fac| S_i times the sum of
    n eps                         the mat-vec row: n products and n - 1 additions in any order, fused or not
    (n + 1) / 2 eps               the norm: the sum of n squares is a sum of positive terms (n roundings at most, one
                                  granted on top), and the root halves a relative error
    G_RSQ = 4e-16                 GRANTED: 1 / sqrt of the sum (dynesty_amd/csrc/walkq.hip: v_rsq_f64 and two Newton steps, stated
                                  "two Newton steps"; sqrt and a quotient, two roundings = 2.2e-16, are inside it)
    G_ROOT = 4e-16                GRANTED: ur^(1/n), twice the 2e-16 dynesty_amd/csrc/walkq.hip states for root_n (twice, as TAU in
                                  tests/hp_ref.py: the project's figure comes from reading, not from a proof)
    eps |ln ur| / n               (pow evaluators only: step_coeff's `exponent`)  pow(ur, fl(1 / n)) moves the result by |ln ur| |fl(1/n) - 1/n| relative,
                                  and |fl(1/n) - 1/n| <= eps / n.  (What the float64 oracle and the lane kernel do; a
                                  Newton iteration on y^n = ur has no such term.)  2e-15 at ur = 2^-53, n = 2.
    2 eps                         two products: the radius with 1 / |z| (or z with g), and the scale
  all of it times 1 + 1e-9        second-order terms: the largest relative error above is 800 eps = 1e-13

  wrap / reflection               np.mod(x, 1), x - floor(x), np.mod(x, 2) and 1 - m are exact except where a result
                                  in (1/2, 1) comes from an x of smaller magnitude (x = -1e-20 -> 1): half an ulp of
                                  the result, granted as eps |w_i| on every wrapped / reflected coordinate.

Nothing is fitted to device output.  The float64 oracle (oracle.proposals_ref.propose_ball) stays within the bound on
every case (tests/test_proposal_hp_cpu.py); `u` is the whole error against the whole bound, `step` is the error
less eps |u'_i| against the bound less eps |u'_i| -- where the final rounding dominates (small steps, the late-run
family) `u` says nothing about the step, and `step` does.

Chains: the map is affine in u with a fixed frame, so the bounds of the accepted steps add (chain_record).  A
decision is decidable when the proposal is further from a face than its accumulated bound and |ln L_hp - loglstar|
exceeds hp_ref.loglike_bound + sum_i |d ln L / d v_i| (prior_bound_i + |dv_i / du_i| (accumulated bound_i + eps |u_i|)).
Slices: generic_slice_step replayed around the high-precision F (slice_walker, with the abscissa grant derived there).
Draws inside an ellipsoid are one step from its centre with scale 1 (proposal_cases.draw_inputs, check_membership).
"""
import math
import os

import mpmath as mp
import numpy as np

import hp_ref as HP
import proposal_cases as PC
from dynesty_amd import problems as PR
from ell_hp_ref import Ratios

LD = np.longdouble
EPS = 2.0**-53
DPS = 50
G_ROOT = 2 * 2e-16
G_RSQ = 4e-16
SECOND = 1.0 + 1e-9


def ld(a):
    return np.asarray(a).astype(LD)


def _hilo(x):
    hi = float(x)
    return hi, float(x - mp.mpf(hi))


def radius_over_norm(z, ur, n):
    """g = ur^(1/n) / |z| as (hi, lo) fp64 with hi + lo good to 1e-32 relative; z, ur exact fp64."""
    with mp.workdps(DPS):
        if ur == 0.0:
            return 0.0, 0.0
        ss = mp.fsum(mp.mpf(float(x))**2 for x in z)
        return _hilo(mp.root(mp.mpf(float(ur)), n) / mp.sqrt(ss))


def draws(inp, steps=1):
    """What every walker of an input set consumes, as NumPy draws it (internal_samplers.py:989-1035, bounding.py:
    1288-1297: the non-cluster uniforms, n normals, one uniform, per step):
    z (k, steps, nc), ur (k, steps), extra (k, steps, d - nc), end states (k, 4)."""
    k, d, nc = inp["k"], inp["d"], inp["nc"]
    z, ur, extra = np.empty((k, steps, nc)), np.empty((k, steps)), np.empty((k, steps, d - nc))
    end = np.empty((k, 4), dtype=np.uint64)
    for i in range(k):
        g = PC.generator_of(inp["states"][i])
        for t in range(steps):
            extra[i, t] = g.random(d - nc)
            z[i, t] = g.standard_normal(nc)
            ur[i, t] = g.random()
        end[i] = PC.state_words(g.bit_generator)
    return z, ur, extra, end


def step_coeff(n, ur, exponent=True):
    """The factor of |fac| S_i in the bound: see the module docstring.  exponent: the evaluator computes the root as
    pow(ur, fl(1 / n)) -- the oracle, the lane kernel, rwalk_propose, the wide kernel, unif_kernel, bound_draw; False
    for the four-lane kernel, whose root_n is a Newton iteration on y^n = ur and is held to G_ROOT alone."""
    ur = np.asarray(ur, dtype=np.float64)
    with np.errstate(divide="ignore"):
        lnu = np.where(ur > 0, np.abs(np.log(np.where(ur > 0, ur, 1.0))), 0.0)
    return (n + (n + 1) / 2.0 + 2.0) * EPS + G_RSQ + G_ROOT + (EPS * lnu / n if exponent else 0.0)


def step_hp(u, a_ld, a_abs, z, ur, g, scale, exponent=True):
    """One proposal before the wrap.  u (nc,) longdouble, z (nc,) fp64, g longdouble.
    Returns (u' longdouble, bound fp64, final-rounding part of the bound fp64)."""
    n = len(z)
    fac = LD(scale) * g
    up = u + fac * (a_ld @ ld(z))
    s = a_abs @ np.abs(z)
    fin = EPS * np.abs(up).astype(np.float64)
    stepb = abs(float(fac)) * s * float(step_coeff(n, ur, exponent))
    return up, (fin + stepb) * SECOND, fin


def wrap_hp(up, bc):
    """Periodic wrap and reflection (utils.py:1053-1078) of a longdouble vector.
    Returns (w, wrap bound, distance of the wrapped / reflected coordinates to the nearest integer)."""
    w = up.copy()
    wb = np.zeros(len(up))
    near = np.full(len(up), np.inf)
    if bc is None:
        return w, wb, near
    for i, b in enumerate(bc[:len(up)]):
        if b == PC.BC_HARD:
            continue
        x = up[i]
        fl = np.floor(x)
        m1 = x - fl
        if b == PC.BC_REFLECT and int(fl) % 2 != 0:
            m1 = LD(1) - m1
        w[i] = m1
        wb[i] = EPS * float(m1)
        near[i] = float(min(x - fl, fl + LD(1) - x))
    return w, wb, near


def face_margin(w, bound, near, bc):
    """min over coordinates of (distance to what would change the outcome) / bound: the cube's faces for a hard
    coordinate, the nearest integer for a wrapped or reflected one.  Above 1: decidable.  And `inside`."""
    hard = np.ones(len(w), dtype=bool) if bc is None else np.asarray(bc[:len(w)]) == PC.BC_HARD
    dist = np.where(hard, np.minimum(np.abs(w), np.abs(LD(1) - w)).astype(np.float64), near)
    inside = bool(np.all((w[hard] > 0) & (w[hard] < 1)))
    return float(np.min(dist / bound)), inside


# ---------------------------------------------------------------------------------------------------------
# one step
# ---------------------------------------------------------------------------------------------------------
def step_g(inp, z=None, ur=None):
    """(g_hi, g_lo) of every walker: the fixture's content."""
    if z is None:
        z, ur, _, _ = draws(inp)
    hl = [radius_over_norm(z[i, 0], ur[i, 0], inp["nc"]) for i in range(inp["k"])]
    return np.array([h for h, _ in hl]), np.array([l for _, l in hl])


def step_reference(inp, g_hi, g_lo, exponent=True):
    """The reference's outcome of one step for every walker of an input set, from the stored g.
    Returns dict(up (k, d) longdouble: the proposal after wrap / reflection; bound, fin (k, d); inside (k,);
    margin (k,); end (k, 4); ur (k,))."""
    k, d, nc, bc = inp["k"], inp["d"], inp["nc"], inp["bc"]
    z, ur, extra, end = draws(inp)
    up = np.empty((k, d), dtype=LD)
    bound, fin = np.zeros((k, d)), np.zeros((k, d))
    inside, margin = np.empty(k, dtype=bool), np.empty(k)
    a_ld, a_abs = ld(inp["axes"]), np.abs(inp["axes"])
    for i in range(k):
        f = inp["idx"][i]
        g = LD(g_hi[i]) + LD(g_lo[i])
        p, b, fi = step_hp(ld(inp["u0"][i, :nc]), a_ld[f], a_abs[f], z[i, 0], ur[i, 0], g, inp["scale"], exponent)
        full = np.concatenate([p, ld(extra[i, 0])])
        w, wb, near = wrap_hp(full, bc)
        up[i] = w
        bound[i, :nc], fin[i, :nc] = b, fi
        bound[i] += wb
        tiny = np.where(bound[i] > 0, bound[i], 1e-300)  # the redrawn coordinates are exact: their margin is huge
        margin[i], inside[i] = face_margin(w, tiny, near, bc)
    return dict(up=up, bound=bound, fin=fin, inside=inside, margin=margin, end=end, ur=ur[:, 0])


def step_record(key, states=None):
    inp = PC.edge_inputs(key, states) if key.startswith("edge/") else PC.draw_inputs(key) \
        if key.startswith("draw/") else PC.step_inputs(key)
    g_hi, g_lo = step_g(inp)
    ref = step_reference(inp, g_hi, g_lo)
    rec = dict(g_hi=g_hi, g_lo=g_lo.astype(np.float32), inside=ref["inside"].astype(np.int8),
               margin=np.float64(ref["margin"].min()), undecidable=np.int32((ref["margin"] <= 1.0).sum()))
    if key.startswith("edge/"):
        rec["states"] = inp["states"]
        rec["tries"] = inp["tries"]
    return rec


def check_step(inp, rec, got, what, propose=False, exponent=True):
    """One step of an evaluator against the reference.  got: u (k, d); inside (k,) bool -- for a walk of one step,
    accept == 1; reject (k,) or None; end (k, 4) or None.  A walk returns u0 where the proposal left the cube
    (exactly); rwalk_propose returns the proposal itself.  Exact parts are asserted here; returns Ratios."""
    ref = step_reference(inp, rec["g_hi"], rec["g_lo"], exponent)
    assert np.array_equal(ref["inside"], rec["inside"] != 0), f"{what}: the fixture does not belong to these inputs"
    assert np.all(ref["margin"] > 1.0), f"{what}: an undecidable walker in a one-step case"
    u = np.asarray(got["u"])
    ins = ref["inside"]
    np.testing.assert_array_equal(np.asarray(got["inside"]).astype(bool), ins, err_msg=f"{what}: inside the cube")
    if got.get("reject") is not None:
        np.testing.assert_array_equal(np.asarray(got["reject"]), (~ins).astype(np.int32), err_msg=f"{what}: rejects")
    if got.get("end") is not None:
        np.testing.assert_array_equal(np.asarray(got["end"]), ref["end"], err_msg=f"{what}: generator end states")
    assert np.all(np.isfinite(u)), f"{what}: a non-finite coordinate"
    rows = np.ones(len(ins), dtype=bool) if propose else ins
    if not propose:
        np.testing.assert_array_equal(u[~ins], inp["u0"][~ins], err_msg=f"{what}: a rejected walker moved")
    zero = ref["ur"] == 0.0
    np.testing.assert_array_equal(u[zero & rows], inp["u0"][zero & rows], err_msg=f"{what}: ur == 0 must not move")
    r = Ratios()
    err = np.abs(ld(u) - ref["up"]).astype(np.float64)[rows]
    b, fin = ref["bound"][rows], ref["fin"][rows]
    r.add("u", HP.worst_ratio(err, b), 1.0)
    r.add("step", HP.worst_ratio(np.maximum(err - fin, 0.0), b - fin), 1.0)
    return r


# ---------------------------------------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------------------------------------
def prior_slope(prob, v64):
    """|dv_i / du_i| at v."""
    if prob.prior_id == PR.PRIOR_IDENTITY:
        return np.ones_like(v64)
    if prob.prior_id == PR.PRIOR_AFFINE:
        return np.full_like(v64, 2.0 * abs(prob.prior_par[0]))
    mu, sg = prob.prior_par
    zz = (v64 - mu) / sg
    return abs(sg) * math.sqrt(2.0 * math.pi) * np.exp(0.5 * zz * zz)


def like_margin(prob, w, acc, loglstar):
    """(ln L_hp(w) > loglstar, |ln L_hp - loglstar| / uncertainty) for a longdouble point w whose fp64 counterpart is
    within acc of it."""
    u64 = w.astype(np.float64)
    v = HP.prior_hp(prob, u64[None])
    v64 = v.astype(np.float64)
    ll = HP.loglike_hp(prob, v)[0]
    du = acc + EPS * np.abs(u64)
    thr = HP.loglike_bound(prob, v64)[0] + float(np.sum(
        HP.loglike_grad_abs(prob, v64)[0] * (HP.prior_bound(prob, u64[None])[0] + prior_slope(prob, v64[0]) * du)))
    return bool(ll > LD(loglstar)), float(abs(ll - LD(loglstar))) / thr


def chain_walker(inp, i):
    """The chain of walker i replayed in high precision: dict(u (d,) longdouble, acc (d,) accumulated bound, accept,
    reject, undecidable, margin: the smallest margin of its decisions, end)."""
    d, bc, prob, walks = inp["d"], inp["bc"], inp["problem"], inp["walks"]
    f = inp["idx"][i]
    a_ld, a_abs = ld(inp["axes"][f]), np.abs(inp["axes"][f])
    g = PC.generator_of(inp["states"][i])
    u, acc = ld(inp["u0"][i]), np.zeros(d)
    nacc = nrej = 0
    und, mmin = False, math.inf
    for _ in range(walks):
        z = g.standard_normal(d)
        ur = g.random()
        if und:
            continue  # the stream is consumed to its end whatever was decided
        hi, lo = radius_over_norm(z, ur, d)
        up, b, _ = step_hp(u, a_ld, a_abs, z, ur, LD(hi) + LD(lo), inp["scale"])
        w, wb, near = wrap_hp(up, bc)
        accn = (acc + b) * SECOND + wb
        m, inside = face_margin(w, accn, near, bc)
        mmin = min(mmin, m)
        if m <= 1.0:
            und = True
            continue
        if not inside:
            nrej += 1
            continue
        above, m = like_margin(prob, w, accn, inp["loglstar"])
        mmin = min(mmin, m)
        if m <= 1.0:
            und = True
            continue
        if above:
            u, acc = w, accn
            nacc += 1
        else:
            nrej += 1
    return dict(u=u, acc=acc, accept=nacc, reject=nrej, undecidable=und, margin=mmin,
                end=PC.state_words(g.bit_generator))


def chain_record(key):
    inp = PC.chain_inputs(key)
    ws = [chain_walker(inp, i) for i in range(inp["k"])]
    u = np.array([w["u"] for w in ws], dtype=LD)
    hi = u.astype(np.float64)
    # the accumulated bound is stored in float32, rounded up
    acc = np.array([w["acc"] for w in ws])
    acc32 = acc.astype(np.float32)
    acc32 = np.where(acc32.astype(np.float64) < acc, np.nextafter(acc32, np.float32(np.inf)), acc32)
    return dict(u_hi=hi, u_lo=(u - ld(hi)).astype(np.float32), acc=acc32.astype(np.float32),
                accept=np.array([w["accept"] for w in ws], dtype=np.int16),
                reject=np.array([w["reject"] for w in ws], dtype=np.int16),
                undecidable=np.array([w["undecidable"] for w in ws], dtype=np.int8),
                margin=np.float64(min(w["margin"] for w in ws)))


def check_caps(rec, what):
    und = rec["undecidable"] != 0
    assert und.mean() <= PC.CAP, f"{what}: {und.sum()} of {len(und)} walkers undecidable"
    assert rec["accept"][~und].sum() > 0 and rec["reject"][~und].sum() > 0, f"{what}: one outcome only"


def check_chain(inp, rec, got, what):
    """A chain of an evaluator against the replay.  got: u, v, logl, accept, reject, end (or None).  Counts and end
    states exact, u within the accumulated bound (plus the rounding of the reference's own storage), ln L within
    hp_ref's bounds at the evaluator's own u and v.  Walkers with an undecidable decision are left out."""
    keep = rec["undecidable"] == 0
    np.testing.assert_array_equal(np.asarray(got["accept"])[keep], rec["accept"][keep], err_msg=f"{what}: accepts")
    np.testing.assert_array_equal(np.asarray(got["reject"])[keep], rec["reject"][keep], err_msg=f"{what}: rejects")
    if got.get("end") is not None:
        _, _, _, end = draws(inp, inp["walks"])
        np.testing.assert_array_equal(np.asarray(got["end"]), end, err_msg=f"{what}: generator end states")
    uref = ld(rec["u_hi"]) + ld(rec["u_lo"])
    moved = rec["accept"] > 0
    u = np.asarray(got["u"])
    np.testing.assert_array_equal(u[keep & ~moved], inp["u0"][keep & ~moved], err_msg=f"{what}: moved without an accept")
    err = np.abs(ld(u) - uref).astype(np.float64)
    # u_lo in float32: 2^-24 of eps |u| / 2; a walker that never moved has bound 0 and error 0
    bound = rec["acc"].astype(np.float64) + 2.0**-24 * EPS * np.abs(rec["u_hi"])
    r = Ratios()
    sel = keep & moved
    r.add("u", HP.worst_ratio(err[sel], bound[sel]) if sel.any() else 0.0, 1.0)
    prob = inp["problem"]
    ev = np.abs(ld(got["v"]) - HP.prior_hp(prob, u)).astype(np.float64)
    el = np.abs(ld(got["logl"]) - HP.loglike_hp(prob, got["v"])).astype(np.float64)
    r.add("v", HP.worst_ratio(ev, HP.prior_bound(prob, u)), 1.0)
    r.add("logl", HP.worst_ratio(el, HP.loglike_bound(prob, got["v"])), 1.0)
    return r


# ---------------------------------------------------------------------------------------------------------
# rslice / slice
# ---------------------------------------------------------------------------------------------------------
def direction_coeff(n):
    """The factor of |scale / |z|| S_i in the bound of an rslice direction scale A z / |z|: the terms of step_bound
    without the root (mat-vec, norm, 1 / sqrt granted, two products)."""
    return ((n + (n + 1) / 2.0 + 2.0) * EPS + G_RSQ) * SECOND


def direction_hp(a, z, scale, g):
    """(direction longdouble, bound) of scale A z / |z| from g = 1 / |z|."""
    fac = LD(scale) * g
    return fac * (ld(a) @ ld(z)), abs(float(fac)) * (np.abs(a) @ np.abs(z)) * direction_coeff(len(z))


def inv_norm(z):
    with mp.workdps(DPS):
        return _hilo(1 / mp.sqrt(mp.fsum(mp.mpf(float(x))**2 for x in z)))


class _Undecidable(Exception):
    pass


def slice_walker(inp, i):
    """generic_slice_step (internal_samplers.py:1075-1206) with stepping out or doubling and the acceptance test of
    Neal's algorithm 6, replayed around the high-precision F(x) = ln L(prior(u + x direction)).

    The abscissae -- left, right, the midpoints, left + random() * width -- are the algorithm's own fp64 numbers and
    stay fp64 here.  x = left + r * width may be contracted into a fused multiply-add by an evaluator.  That removes
    the rounding of the product r * width, half an ulp of a number as large as the window -- after doubling to a
    window of 2^11 and cancellation to x = 0.01 that is many ulps of x, so the grant is in ulps of the largest
    abscissa in play, M = max(|left|, |right|): the product rounded or not (ulp(r * width) / 2 <= ulp(M)), the sum
    rounded from another value (<= ulp(M)), and width = right - left rounded from end points that differ
    (<= ulp(M)): 3 ulp(M).  A contraction point becomes an end point and the next x is a convex combination of the end
    points, so it inherits the larger of their errors on top of its own 3 ulp(M); end points set by stepping out or
    doubling are sums and differences without a product, the same in every evaluator, and carry none.
    The point F looks at is u + x direction: its bound is the accumulated bound of u, |x| times the direction's,
    |direction_i| times the abscissa's, and two roundings eps (|x direction_i| + |u_i + x direction_i|).
    A direction longer than maxlen = sqrt(n) / 2 is divided by dirlen / maxlen: the decision has the margin
    |dirlen - maxlen| over the norm's error; the quotient adds ((n + 1) / 2 + 4) eps relative (sum of squares and
    root, the root of n, two quotients) and the direction's own error carried through the norm."""
    d, prob, loglstar = inp["d"], inp["problem"], inp["loglstar"]
    a = inp["axes"][inp["idx"][i]]
    g = PC.generator_of(inp["states"][i])
    st = dict(u=ld(inp["u0"][i]), acc=np.zeros(d), nc=0, ne=0, nt=0, margin=math.inf)
    doubling = inp["doubling"]

    def note(m):
        st["margin"] = min(st["margin"], m)
        if m <= 1.0:
            raise _Undecidable()

    def one_step(dr, db):
        rand0 = g.random()
        dirlen = np.sqrt(np.sum(dr * dr))
        maxlen = np.sqrt(LD(d)) / LD(2)
        carried = float(np.sum(np.abs(dr).astype(np.float64) * db) / dirlen)
        note(float(abs(dirlen - maxlen)) / (carried + ((d + 1) / 2.0 + 1.0) * EPS * float(dirlen) + EPS * float(maxlen)))
        if dirlen > maxlen:
            q = maxlen / dirlen
            db = db * float(q) + np.abs(dr * q).astype(np.float64) * (((d + 1) / 2.0 + 4.0) * EPS + carried / float(dirlen))
            dr = dr * q
        dabs = np.abs(dr).astype(np.float64)

        def F(x, xerr=0.0):
            st["nc"] += 1
            unew = st["u"] + LD(x) * dr
            b = (st["acc"] + abs(x) * db + xerr * dabs
                 + EPS * (abs(x) * dabs + np.abs(unew).astype(np.float64))) * SECOND
            m, inside = face_margin(unew, b, None, None)
            note(m)
            if not inside:
                return False, unew, b
            above, m = like_margin(prob, unew, b, loglstar)
            note(m)
            return above, unew, b

        left, right = -rand0, 1 - rand0
        el = er = 0.0  # what the end points may differ by between evaluators
        fl, fr = F(left)[0], F(right)[0]
        nexp = 0
        if not doubling:
            while fl:
                left -= 1
                fl = F(left)[0]
                nexp += 1
            while fr:
                right += 1
                fr = F(right)[0]
                nexp += 1
            assert nexp <= 1000, "the expansion warning is not part of these cases"
        else:
            kk = 1
            while fl or fr:
                if g.random() < 0.5:
                    left -= (right - left)
                    fl = F(left)[0]
                else:
                    right += (right - left)
                    fr = F(right)[0]
                nexp += kk
                kk *= 2
            big_l, big_r, f_l, f_r = left, right, fl, fr
        st["ne"] += nexp
        while True:
            x = left + g.random() * (right - left)
            xerr = max(el, er) + 3.0 * np.spacing(max(abs(left), abs(right)))
            above, unew, b = F(x, xerr)
            st["nt"] += 1
            if above and doubling:
                # _doubling_accept: the points it looks at are midpoints of exact end points
                lh, rh, flh, frh, dd = big_l, big_r, f_l, f_r, False
                while rh - lh > 1.1:
                    mid = (lh + rh) / 2.
                    if (0 < mid <= x) or (x < mid <= 0):
                        dd = True
                    if x < mid:
                        rh = mid
                        frh = F(rh)[0]
                    else:
                        lh = mid
                        flh = F(lh)[0]
                    if dd and not flh and not frh:
                        above = False
                        break
            if above:
                break
            if x < 0:
                left, el = x, xerr
            elif x > 0:
                right, er = x, xerr
            else:
                raise RuntimeError("Slice sampler has failed to find a valid point")
        st["u"], st["acc"] = unew, b

    und = False
    try:
        for _ in range(inp["slices"]):
            if inp["principal"]:
                order = np.arange(d)
                g.shuffle(order)
                for j in order:
                    dr = LD(inp["scale"]) * ld(a[:, j])  # scale * axes.T[j]: one rounding
                    one_step(dr, EPS * np.abs(dr).astype(np.float64))
            else:
                z = g.standard_normal(d)
                hi, lo = inv_norm(z)
                one_step(*direction_hp(a, z, inp["scale"], LD(hi) + LD(lo)))
    except _Undecidable:
        und = True
    return dict(u=st["u"], acc=st["acc"], ncalls=st["nc"], n_expand=st["ne"], n_contract=st["nt"], undecidable=und,
                margin=st["margin"], end=None if und else PC.state_words(g.bit_generator))


def slice_record(key):
    inp = PC.slice_inputs(key)
    ws = [slice_walker(inp, i) for i in range(inp["k"])]
    u = np.array([w["u"] for w in ws], dtype=LD)
    hi = u.astype(np.float64)
    acc = np.array([w["acc"] for w in ws])
    acc32 = acc.astype(np.float32)
    acc32 = np.where(acc32.astype(np.float64) < acc, np.nextafter(acc32, np.float32(np.inf)), acc32)
    rec = dict(u_hi=hi, u_lo=(u - ld(hi)).astype(np.float32), acc=acc32.astype(np.float32),
               undecidable=np.array([w["undecidable"] for w in ws], dtype=np.int8),
               margin=np.float64(min(w["margin"] for w in ws)),
               end=np.array([w["end"] if w["end"] is not None else np.zeros(4, dtype=np.uint64) for w in ws],
                            dtype=np.uint64))
    for name in ("ncalls", "n_expand", "n_contract"):
        rec[name] = np.array([w[name] for w in ws], dtype=np.int32)
    if key in PC.feed_keys():
        z = np.array([PC.generator_of(inp["states"][i]).standard_normal(inp["d"]) for i in range(inp["k"])])
        hl = [inv_norm(z[i]) for i in range(inp["k"])]
        rec["feed_hi"], rec["feed_lo"] = np.array([h for h, _ in hl]), np.array([l for _, l in hl], dtype=np.float32)
    return rec


def check_slice_caps(rec, what):
    und = rec["undecidable"] != 0
    assert und.mean() <= PC.CAP, f"{what}: {und.sum()} of {len(und)} walkers undecidable"


def check_slice(inp, rec, got, what):
    """got: u, v, logl, ncalls, n_expand, n_contract, expansion_warning_set, end.  Counts, flags and generator end
    states exact, u within the bound of the point the last slice accepted, ln L within hp_ref's bounds at the
    evaluator's own u and v.  Walkers with an undecidable decision are left out."""
    keep = rec["undecidable"] == 0
    for name in ("ncalls", "n_expand", "n_contract"):
        np.testing.assert_array_equal(np.asarray(got[name])[keep], rec[name][keep], err_msg=f"{what}: {name}")
    assert not np.any(np.asarray(got["expansion_warning_set"])[keep]), f"{what}: expansion warning"
    np.testing.assert_array_equal(np.asarray(got["end"])[keep], rec["end"][keep], err_msg=f"{what}: generator end states")
    u = np.asarray(got["u"])
    err = np.abs(ld(u) - (ld(rec["u_hi"]) + ld(rec["u_lo"]))).astype(np.float64)
    bound = rec["acc"].astype(np.float64) + 2.0**-24 * EPS * np.abs(rec["u_hi"])
    r = Ratios()
    r.add("u", HP.worst_ratio(err[keep], bound[keep]), 1.0)
    prob = inp["problem"]
    ev = np.abs(ld(got["v"]) - HP.prior_hp(prob, u)).astype(np.float64)
    el = np.abs(ld(got["logl"]) - HP.loglike_hp(prob, got["v"])).astype(np.float64)
    r.add("v", HP.worst_ratio(ev, HP.prior_bound(prob, u)), 1.0)
    r.add("logl", HP.worst_ratio(el, HP.loglike_bound(prob, got["v"])), 1.0)
    return r


def check_feed(inp, rec, dirs, what):
    """slice_feed's directions scale A z / |z| of the walkers' first n normals, at the direction's bound."""
    r = Ratios()
    worst = 0.0
    for i in range(inp["k"]):
        z = PC.generator_of(inp["states"][i]).standard_normal(inp["d"])
        dr, db = direction_hp(inp["axes"][inp["idx"][i]], z, inp["scale"], LD(rec["feed_hi"][i]) + LD(rec["feed_lo"][i]))
        # the stored direction is rounded once more
        worst = max(worst, HP.worst_ratio(np.abs(ld(dirs[i]) - dr).astype(np.float64),
                                          db + EPS * np.abs(dr).astype(np.float64)))
    r.add("direction", worst, 1.0)
    return r


# ---------------------------------------------------------------------------------------------------------
# draws inside ellipsoids
# ---------------------------------------------------------------------------------------------------------
def check_membership(inp, xs, qs, what):
    """MultiEllipsoid.samples' q (bounding.py:525-590): the number of ellipsoids with (x - c)^T A (x - c) < 1, at the
    evaluator's own x; exact wherever every one of the quadratic forms is further from 1 than
    ell_hp_ref.quadform_bound.  Returns the share of draws that were decidable."""
    import ell_hp_ref as EH
    xs = np.asarray(xs)
    q = np.stack([EH.quadforms_ld(xs, inp["ctrs"][e], inp["ams"][e])[0] for e in range(len(inp["ctrs"]))], axis=1)
    b = np.stack([EH.quadform_bound(inp["d"], EH.quadforms_ld(xs, inp["ctrs"][e], inp["ams"][e])[1])
                  for e in range(len(inp["ctrs"]))], axis=1)
    clear = np.all(np.abs(q - LD(1)).astype(np.float64) > b, axis=1)
    want = (q < 1).sum(axis=1)
    assert np.all(want[clear] >= 1), f"{what}: a draw outside every ellipsoid"
    np.testing.assert_array_equal(np.asarray(qs)[clear], want[clear], err_msg=f"{what}: membership counts")
    assert (want[clear] >= 2).sum() >= 5, f"{what}: the ellipsoids hardly overlap"
    return float(clear.mean())


# ---------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------
def all_keys():
    """One-step sets, constructed-uniform sets, and the walks that are replayed (rwalk chains, then slices)."""
    return [s[0] for s in PC.step_sets()] + PC.draw_keys(), PC.edge_keys(), PC.chain_keys() + PC.slice_keys()


_SLICE_COUNTS = ("ncalls", "n_expand", "n_contract")


def pack_fixture(records):
    """{key: record} -> the arrays of tests/golden/proposal_hp.npz, walkers end to end in the order of all_keys()
    (the keys themselves are regenerated, not stored)."""
    skeys, ekeys, ckeys = all_keys()
    assert sorted(skeys + ekeys + ckeys) == sorted(records)
    one = skeys + ekeys
    g = {"step_k": np.array([len(records[k]["g_hi"]) for k in one], dtype=np.int32)}
    for name in ("g_hi", "g_lo", "inside"):
        g["step_" + name] = np.concatenate([records[k][name] for k in one])
    g["step_margin"] = np.array([records[k]["margin"] for k in one])
    g["step_undecidable"] = np.array([records[k]["undecidable"] for k in one], dtype=np.int32)
    g["edge_states"] = np.array([records[k]["states"] for k in ekeys], dtype=np.uint64)
    g["chain_k"] = np.array([len(records[k]["undecidable"]) for k in ckeys], dtype=np.int32)
    g["chain_d"] = np.array([records[k]["u_hi"].shape[1] for k in ckeys], dtype=np.int32)
    for name in ("u_hi", "u_lo", "acc"):
        g["chain_" + name] = np.concatenate([records[k][name].ravel() for k in ckeys])
    g["chain_undecidable"] = np.concatenate([records[k]["undecidable"] for k in ckeys])
    for name in ("accept", "reject"):
        g["chain_" + name] = np.concatenate([records[k][name] for k in ckeys if name in records[k]])
    g["chain_margin"] = np.array([records[k]["margin"] for k in ckeys])
    sk = PC.slice_keys()
    for name in _SLICE_COUNTS + ("end",):
        g["slice_" + name] = np.concatenate([records[k][name] for k in sk])
    for name in ("feed_hi", "feed_lo"):
        g["slice_" + name] = np.concatenate([records[k][name] for k in PC.feed_keys()])
    return g


def load_fixture(path=None):
    """{key: record} from tests/golden/proposal_hp.npz (see pack_fixture)."""
    g = np.load(path or os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "proposal_hp.npz"))
    skeys, ekeys, ckeys = all_keys()
    one = skeys + ekeys
    assert len(g["step_k"]) == len(one) and len(g["chain_k"]) == len(ckeys), \
        "tests/golden/proposal_hp.npz does not belong to this list of cases: regenerate it"
    out = {}
    at = np.concatenate([[0], np.cumsum(g["step_k"])])
    for i, key in enumerate(one):
        s = slice(at[i], at[i + 1])
        out[key] = dict(g_hi=g["step_g_hi"][s], g_lo=g["step_g_lo"][s], inside=g["step_inside"][s],
                        margin=g["step_margin"][i], undecidable=g["step_undecidable"][i])
    for i, key in enumerate(ekeys):
        out[key]["states"] = g["edge_states"][i]
    at = np.concatenate([[0], np.cumsum(g["chain_k"])])
    at2 = np.concatenate([[0], np.cumsum(g["chain_k"] * g["chain_d"])])
    nrw = sum(int(g["chain_k"][i]) for i, key in enumerate(ckeys) if key.startswith("chain/"))
    feed_at = 0
    for i, key in enumerate(ckeys):
        s, s2 = slice(at[i], at[i + 1]), slice(at2[i], at2[i + 1])
        shape = (int(g["chain_k"][i]), int(g["chain_d"][i]))
        out[key] = dict(u_hi=g["chain_u_hi"][s2].reshape(shape), u_lo=g["chain_u_lo"][s2].reshape(shape),
                        acc=g["chain_acc"][s2].reshape(shape), undecidable=g["chain_undecidable"][s],
                        margin=g["chain_margin"][i])
        if key.startswith("chain/"):  # the rwalk chains come first
            out[key].update(accept=g["chain_accept"][s], reject=g["chain_reject"][s])
        else:
            t = slice(at[i] - nrw, at[i + 1] - nrw)
            out[key].update({name: g["slice_" + name][t] for name in _SLICE_COUNTS + ("end",)})
            if key in PC.feed_keys():
                out[key].update(feed_hi=g["slice_feed_hi"][feed_at:feed_at + shape[0]],
                                feed_lo=g["slice_feed_lo"][feed_at:feed_at + shape[0]])
                feed_at += shape[0]
    return out


def inputs_of(key, fix=None):
    if key.startswith("edge/"):
        return PC.edge_inputs(key, fix[key]["states"])
    if key.startswith("chain/"):
        return PC.chain_inputs(key)
    if key.startswith("slice/"):
        return PC.slice_inputs(key)
    if key.startswith("draw/"):
        return PC.draw_inputs(key)
    return PC.step_inputs(key)
