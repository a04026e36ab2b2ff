"""Ellipsoid membership restated in np.longdouble (64-bit mantissa on x86), the reference the five membership kernels
(contains_kernel, wide_contains_kernel, contains_runs_kernel, contains_runs_lds_kernel, contains_runs_wide_kernel) are
held to, and the bound an fp64 evaluation of it has to keep.  Plain Python: no device code.

The quantity is q = (x - c)^T A (x - c) per (point, ellipsoid), from the float64 inputs; S = |x - c|^T |A| |x - c| is the
sum of the absolute values of its d^2 terms.

The bound.  Write u = 2^-53.  Every kernel forms dl_i = fl(x_i - c_i) = (x_i - c_i)(1 + e_i), |e_i| <= u (one rounding;
none where x_i and c_i lie within a factor two of each other), then r_i = sum_j A_ij dl_j and q = sum_i dl_i r_i.
  * The narrow forms (contains_kernel, contains_runs_kernel, contains_runs_lds_kernel) run both sums as chains of d
    fused multiply-adds: one rounding per step, so a term of r_i passes through at most d roundings and a term of q
    through at most d more.  With the two roundings of dl_i and dl_j a term dl_i A_ij dl_j of q carries a factor
    (1 + e)^(2d + 2), and |q_fp64 - q| <= ((1 + u)^(2d + 2) - 1) S <= (2d + 4) u S: the second-order remainder,
    (2d + 2)^2 u^2 / 2, stays below the 2 u left over for every d < 10^7.
  * wide_contains_kernel has the same row chain (d) and folds the rows a thread owns (ceil(d / 256) steps) and then a
    tree of 8 additions: shorter than d for d > 32.  contains_runs_wide_kernel has the row chain (d), a lane's fold over
    ceil(d / 64) chunks and 6 levels across the lanes: shorter too.  Both are held to the same (2d + 4) u S; the
    sequential narrow form is the longest chain.
  * The reference itself: the differences are exact or rounded once to 64 bits, the rows and the fold are sums of d
    products, so a term passes through at most 2d + 2 roundings of 2^-64 each.  That is below (d^2 + 2d) 2^-64 S from
    d = 2 on; at d = 1 it is 4 against 3, and the missing 2^-64 S lies far inside the 2 u S of slack above.
Together:  bound = (2d + 4) 2^-53 S + (d^2 + 2d) 2^-64 S.

A pair is DECIDABLE when |q_hp - 1| > bound: every fp64 evaluation within the bound then gives the same verdict as the
reference (q < 1 in mode 0 / strict, sqrt(q) <= 1 in mode 1 / single).  A pair whose evaluation gives the same float64
in every order (the dyadic cases of tests/contains_cases.py: exact at q == 1, rounding identically one ulp either side)
has bound 0 and is decidable at q == 1 too: mode 0 says outside, mode 1 inside.  A point with a NaN coordinate is inside
nothing, decidably.

check_quad, check_verdicts and check_runs raise AssertionError where a kernel's output breaks this, and return the worst
ratio they saw so that it can be recorded."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
U_LD = 2.0 ** -64


def ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def quad_hp(x, ctrs, ams):
    """q and S, (k, m) long double each, for x (k, d) against ctrs (m, d), ams (m, d, d)."""
    x, ctrs, ams = ld(x), ld(ctrs), ld(ams)
    k, m = x.shape[0], ctrs.shape[0]
    q, s = np.empty((k, m), dtype=LD), np.empty((k, m), dtype=LD)
    for a in range(m):
        dl = x - ctrs[a]
        q[:, a] = np.sum(dl * (dl @ ams[a].T), axis=1)
        dl = np.abs(dl)
        s[:, a] = np.sum(dl * (dl @ np.abs(ams[a]).T), axis=1)
    return q, s


def coeff(d):
    return LD(2 * d + 4) * LD(U) + LD(d * d + 2 * d) * LD(U_LD)


def quad_bound(d, s):
    """The bound of the module docstring for S = s (NaN where s is NaN)."""
    return coeff(d) * s


def reference(x, ctrs, ams, exact=None):
    """(q, bound) of every pair; `exact` (k,) marks points whose evaluation gives the same float64 in every order
    (exact, or rounding identically): bound 0."""
    q, s = quad_hp(x, ctrs, ams)
    b = quad_bound(np.shape(x)[1], s)
    if exact is not None:
        b[np.asarray(exact, dtype=bool)] = 0
    return q, b


def hp_inside(q, mode):
    """The reference's verdict: mode 0 q < 1, mode 1 q <= 1 (sqrt(q) <= 1 exactly where q <= 1); NaN: outside."""
    with np.errstate(invalid="ignore"):
        return (q < 1) if mode == 0 else (q <= 1)


def decidable(q, bound):
    """|q - 1| > bound, or an exact pair (bound 0), or a NaN point (inside nothing)."""
    with np.errstate(invalid="ignore"):
        return (np.abs(q - 1) > bound) | (bound == 0) | np.isnan(q)


def unpack(mask, k):
    """dh_contains' mask (m, ceil(k / 64)) uint64 -> (k, m) bool, and the bits of the last words beyond k."""
    m = mask.shape[0]
    bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(m, -1), axis=1, bitorder="little")
    return bits[:, :k].astype(bool).T, bits[:, k:]


def check_quad(quad, q, bound):
    """|quad - q| <= bound for every pair; NaN exactly where the reference is NaN.  Returns the worst error / bound
    (an exact pair counts 0 when it is met exactly)."""
    quad = np.asarray(quad, dtype=np.float64)
    nan = np.isnan(q)
    assert np.array_equal(np.isnan(quad), nan), "NaN pairs differ from the reference's"
    err = np.abs(quad.astype(LD) - q)
    ok = ~nan
    zero = ok & (bound == 0)
    assert np.all(err[zero] == 0), f"an exact pair is off by {float(np.max(err[zero]))}"
    rest = ok & ~zero
    if not rest.any():
        return 0.0
    ratio = (err[rest] / bound[rest]).astype(np.float64)
    worst = float(np.max(ratio))
    assert worst <= 1.0, f"quad: error / bound = {worst:.3g}"
    return worst


def check_verdicts(inside, q, bound, mode):
    """inside (k, m) bool against the reference's verdict on every decidable pair.  Returns how near the boundary the
    comparison reached: the largest bound / |q - 1| over the compared pairs that are not exact (below 1)."""
    inside = np.asarray(inside, dtype=bool)
    dec = decidable(q, bound)
    want = hp_inside(q, mode)
    bad = dec & (inside != want)
    assert not bad.any(), (f"mode {mode}: {int(bad.sum())} decidable verdict(s) differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"q - 1 = {float((q - 1)[bad][0]):.3g}, bound {float(bound[bad][0]):.3g}")
    near = dec & (bound > 0) & ~np.isnan(q)
    return float(np.max((bound[near] / np.abs(q - 1)[near]).astype(np.float64))) if near.any() else 0.0


def entry_states(q, bound, nells, strict):
    """Per queue entry of one run, from q / bound (wpr, max_ells): +1 decidably outside all of the first nells
    ellipsoids, -1 decidably inside one of them, 0 neither."""
    mode = 0 if strict else 1
    q, bound = q[:, :nells], bound[:, :nells]
    dec, ins = decidable(q, bound), hp_inside(q, mode)
    state = np.zeros(q.shape[0], dtype=np.int8)
    state[np.all(dec & ~ins, axis=1)] = 1
    state[np.any(dec & ins, axis=1)] = -1
    return state


def served_runs(runs, run_mode, my_mode, bstatus):
    s = np.ones(runs, dtype=bool)
    if run_mode is not None:
        s &= np.asarray(run_mode) == my_mode
    if bstatus is not None:
        s &= np.asarray(bstatus) == 0
    return s


def runs_from_inside(inside_any, served, flag_in, first_in):
    """What the run-wise kernels must return when entry j of run r is inside its bound exactly where inside_any[r, j]:
    flag |= 1 and first = min(first, lowest outside index) for a served run with an entry outside; all else as sent."""
    flag = np.array(flag_in, dtype=np.int32)
    first = None if first_in is None else np.array(first_in, dtype=np.int32)
    for r in range(len(flag)):
        out = np.flatnonzero(~np.asarray(inside_any[r], dtype=bool))
        if served[r] and len(out):
            flag[r] |= 1
            if first is not None:
                first[r] = min(first[r], out[0])
    return flag, first


def check_runs(flag, first, flag_in, first_in, states, served):
    """flag / first (runs,) as returned against the entry states (runs, wpr) of the reference.  A served run: bit 0 set
    if an entry is decidably outside, clear if all are decidably inside (and it was sent clear); first = the lowest
    outside index -- the lowest decidably outside one, or an undecided one below it -- or the value sent where nothing
    is outside; the upper bits of flag as sent.  A run that is not served: both words as sent.  Returns the share of
    served runs whose flag and first were both fully determined by the reference."""
    flag, flag_in = np.asarray(flag), np.asarray(flag_in)
    runs = len(flag_in)
    determined = 0
    for r in range(runs):
        if not served[r]:
            assert flag[r] == flag_in[r], f"run {r} is masked: flag {flag_in[r]} came back {flag[r]}"
            if first is not None:
                assert first[r] == first_in[r], f"run {r} is masked: first {first_in[r]} came back {first[r]}"
            continue
        assert (flag[r] & ~1) == (flag_in[r] & ~1), f"run {r}: upper bits of flag {flag_in[r]} came back {flag[r]}"
        out = np.flatnonzero(states[r] == 1)
        maybe = np.flatnonzero(states[r] == 0)
        if len(out):
            assert flag[r] & 1, f"run {r}: entry {out[0]} is outside and the run is not flagged"
        elif not len(maybe):
            assert (flag[r] & 1) == (flag_in[r] & 1), f"run {r}: every entry is inside and the run is flagged"
        if first is not None:
            j0 = out[0] if len(out) else np.iinfo(np.int32).max
            allowed = {min(int(first_in[r]), int(j)) for j in maybe[maybe < j0]}
            allowed.add(min(int(first_in[r]), int(j0)))
            assert int(first[r]) in allowed, f"run {r}: first {first[r]}, the reference allows {sorted(allowed)}"
            if len(allowed) == 1 and (len(out) or not len(maybe)):
                determined += 1
        elif len(out) or not len(maybe):
            determined += 1
    n = int(np.sum(served))
    return determined / n if n else 1.0
