"""Seeded cases for tests/scale_hp_ref.py: ellipsoids and targets at which scale_to_logvol can go wrong.

An ellipsoid is axes = Q diag(axlens) with Q orthogonal (QR of a seeded normal matrix; a signed permutation in the
dyadic case), rounded once; cov = axes axes^T and am = axes diag(axlens^-4) axes^T are formed from the rounded axes in
long double and rounded once.  At D = 512 that holds for the `edge` family, whose undecided pair's bound uses it; the
other families' cov and am are formed in float64 there (two long-double products of that size cost 1.4 s per ellipsoid,
and outside the undecided pair neither branch asks more of cov and am than to be the stored numbers).  A case is one
call: up to 6 ellipsoids of one dimension.  c = sqrt(D) / 2 is the cap.

  enlarge  largest axis at 0.3 c and 0.9 c; logf = ln 1.25, D ln 1.05, D ln 1.5 (the enlarge factor and the bootstrap's)
  edge     the isotropic decision at +-64, +-8 and +-1/8 of its bound (the last undecided on purpose); logvol = 0 and a
           largest axis at c (1 - 2^-7), so that the target resolves the margin to 1e-19
  capped   one axis reaches the cap; half of them; all of them (volume unspent); an axis already over the cap with a
           growing target; the same with a shrinking one (delta = 0 everywhere: axes and axlens come back bit for bit)
  ties     all axlens equal (both branches); two equal leading axes, both capped; dyadic axlens on a signed permutation
  kappa    axis ratios 1e3 and 1e6 on both branches
  shrink   logf = -D ln 2 (isotropic), and target = logvol (f = 1: everything bit for bit)
  tiny     axlens of 1e-7; logf = -300 D; logf = +300 D on axlens of 1e-140 (everything stays inside fp64)

Every family runs at every dimension.  At D = 512 cov', am' and axes' are compared on 48 rows (the first and last four
and 40 seeded ones, every column; axlens' and logvol' in full): the launch takes no other route there than at 65 and
128, which are compared in full.

tests/golden/scale_hp.npz pins the reference's per-axis delta (as two doubles), its verdicts and the targets; run this
file to write it again.
"""
import functools
import math
import os

import numpy as np

import scale_hp_ref as H

DIMS = (1, 2, 3, 5, 15, 16, 17, 25, 32, 33, 44, 45, 64, 65, 128, 512)
FAMILIES = ("enlarge", "edge", "capped", "ties", "kappa", "shrink", "tiny")
CASES = [(f, d) for d in DIMS for f in FAMILIES]
EDGE_K = (64.0, 8.0, 0.125, -0.125, -8.0, -64.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scale_hp.npz")


def prefactor(D):
    """ln of the unit D-ball's volume."""
    return 0.5 * D * math.log(math.pi) - math.lgamma(0.5 * D + 1.0)


def spread(rng, D, ratio, top):
    """D distinct axis lengths from top down to top / ratio, geometric, in seeded order."""
    a = top * ratio ** (-np.arange(D) / max(D - 1, 1))
    return rng.permutation(a)


def gram_ld(Y, Z):
    """Y Z^T in long double for Z = Y diag(w): symmetric, so only the blocks on and above the diagonal are formed."""
    D, blk = Y.shape[0], 64
    out = np.empty((D, D), dtype=H.LD)
    for i in range(0, D, blk):
        out[i:i + blk, i:] = Y[i:i + blk] @ Z[i:].T
        out[i:, i:i + blk] = out[i:i + blk, i:].T
    return out


def ellipsoid(rng, axlens, perm=False, exact=True):
    axlens = np.asarray(axlens, dtype=np.float64)
    D = len(axlens)
    if perm:
        Q = np.eye(D)[rng.permutation(D)] * rng.choice([-1.0, 1.0], D)
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    X = (H.ld(Q) * H.ld(axlens)).astype(np.float64)
    if not exact:
        Y = X / axlens ** 2  # (Q / axlens: axlens^-4 itself would leave fp64 at axlens of 1e-140)
        cov, am = X @ X.T, Y @ Y.T
    elif D >= 512:
        Xl, a = H.ld(X), H.ld(axlens)
        cov, am = gram_ld(Xl, Xl).astype(np.float64), gram_ld(Xl, Xl / (a * a * a * a)).astype(np.float64)
    else:
        Xl, a = H.ld(X), H.ld(axlens)
        cov, am = (Xl @ Xl.T).astype(np.float64), ((Xl / (a * a * a * a)) @ Xl.T).astype(np.float64)
    logvol = float(prefactor(D) + np.sum(np.log(axlens)))
    return dict(cov=cov, am=am, axes=X, axlens=axlens, logvol=logvol)


def specs(family, D, rng):
    """[(label, axlens, logf or None, perm)]; logf None: the edge family's own targets."""
    c = math.sqrt(D) / 2
    h = D // 2
    if family == "enlarge":
        tops = (0.3, 0.9)
        logfs = (("ln1.25", math.log(1.25)), ("Dln1.05", D * math.log(1.05)), ("Dln1.5", D * math.log(1.5)))
        return [(f"top{t}/{n}", spread(rng, D, 10.0, t * c), lf, False) for t in tops for n, lf in logfs]
    if family == "edge":
        return [(f"k={k:+g}", spread(rng, D, 10.0, c * (1 - 2.0 ** -7)), None, False) for k in EDGE_K]
    if family == "capped":
        lo = spread(rng, D, 3.0, 0.3 * c)
        one = lo.copy()
        one[rng.integers(D)] = 0.9 * c
        half = np.concatenate([spread(rng, D - h, 1.2, 0.95 * c), spread(rng, h, 3.0, 0.2 * c)])
        over = spread(rng, D, 2.0, 0.6 * c)
        over_g, over_s = over.copy(), over.copy()
        over_g[rng.integers(D)] = 1.2 * c
        over_s[rng.integers(D)] = 1.5 * c
        return [("half", rng.permutation(half), D * 0.5, False), ("one", one, D * math.log(1.3), False),
                ("all", spread(rng, D, 1.8, 0.9 * c), D * 2.0, False), ("over_grow", over_g, D * 0.3, False),
                ("over_shrink", over_s, -D * 0.2, False)]
    if family == "ties":
        two = spread(rng, D, 3.0, 0.5 * c)
        two[:min(2, D)] = 0.9 * c
        dy = 2.0 ** -(1.0 + np.arange(D) % 4)
        return [("equal_iso", np.full(D, 0.3 * c), math.log(1.25), False),
                ("equal_capped", np.full(D, 0.9 * c), D * math.log(1.5), False),
                ("two_lead", rng.permutation(two), D * 0.2, False),
                ("dyadic", rng.permutation(dy), D * math.log(1.5), True),
                ("dyadic_capped", rng.permutation(dy) * 2.0 ** math.floor(math.log2(c) + 1), D * 0.4, True)]
    if family == "kappa":
        return [(f"{r:g}/{n}", spread(rng, D, r, t * c), lf, False) for r in (1e3, 1e6)
                for n, t, lf in (("iso", 0.3, math.log(1.25)), ("greedy", 0.9, D * math.log(1.5)))]
    if family == "shrink":
        return [("half_volume", spread(rng, D, 10.0, 0.9 * c), -D * math.log(2.0), False),
                ("f=1", spread(rng, D, 10.0, 0.9 * c), 0.0, False)]
    if family == "tiny":
        return [("axlens1e-7", spread(rng, D, 10.0, 1e-7), math.log(1.25), False),
                ("logf-300D", spread(rng, D, 10.0, 0.5 * c), -300.0 * D, False),
                ("logf+300D", spread(rng, D, 10.0, 1e-140), 300.0 * D, False)]
    raise KeyError(family)


def edge_target(axlens, k):
    """logvol = 0 and the target whose margin is k decision bounds (k > 0: isotropic)."""
    import mpmath as mp
    D = len(axlens)
    with mp.workdps(H.DPS):
        cap = mp.log(mp.sqrt(D) / 2)
        mx = max(mp.log(mp.mpf(float(a))) for a in axlens)
        B = H.scalars(axlens, 0.0, float(D * (cap - mx)))["dec_bound"]
        return float(D * (cap - mx - k * mp.mpf(B)))


def rows_of(D):
    if D < 512:
        return None
    rng = np.random.default_rng(512)
    return np.unique(np.concatenate([np.arange(4), np.arange(D - 4, D), rng.choice(np.arange(4, D - 4), 40, replace=False)]))


@functools.lru_cache(maxsize=None)
def inputs(family, D):
    """The float64 arrays of one call: covs, ams, axes (m, D, D), axlens (m, D), logvols, targets (m,), labels."""
    rng = np.random.default_rng([FAMILIES.index(family), D, 20250])
    ells, targets, labels = [], [], []
    for label, axlens, logf, perm in specs(family, D, rng):
        e = ellipsoid(rng, axlens, perm, exact=D < 512 or family == "edge")
        if logf is None:
            e["logvol"] = 0.0
            targets.append(edge_target(e["axlens"], float(label[2:])))
        else:
            targets.append(e["logvol"] + logf)
        ells.append(e)
        labels.append(label)
    c = {n + "s": np.ascontiguousarray(np.stack([e[n] for e in ells])) for n in ("cov", "am", "axes", "axlens", "logvol")}
    c.update(targets=np.array(targets), labels=labels, name=f"{family} D={D}", family=family, D=D, rows=rows_of(D))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(family, D):
    """inputs(family, D) with the reference: ref[e] = (values, bounds, scalars) per ellipsoid."""
    c = dict(inputs(family, D))
    c["ref"] = [H.reference(c["covs"][e], c["ams"][e], c["axess"][e], c["axlenss"][e], c["logvols"][e], c["targets"][e],
                            rows=c["rows"]) for e in range(len(c["targets"]))]
    return c


CLOUDS = ("c2", "c3", "g3", "two5", "ring2", "flat10", "small4")


@functools.lru_cache(maxsize=None)
def cloud_case(name):
    """The reference's bounding ellipsoid of a small cloud (`be/*` of tests/golden/bounding.npz) and the anisotropic
    target tests/test_gpu_small_kernels.py scales it to: the same inputs, held to the derived bounds."""
    g = np.load(os.path.join(os.path.dirname(GOLDEN), "bounding.npz"))
    c = {n + "s": np.ascontiguousarray(g[f"{name}/be/{n}"], dtype=np.float64)[None] for n in ("cov", "am", "axes", "axlens")}
    D = c["axlenss"].shape[1]
    c.update(logvols=np.array([float(g[f"{name}/be/logvol"])]), targets=np.array([float(g[f"{name}/aniso/target"])]),
             labels=["be -> aniso"], name=f"cloud {name} D={D}", family="cloud", D=D, rows=None)
    c["ref"] = [H.reference(c["covs"][0], c["ams"][0], c["axess"][0], c["axlenss"][0], c["logvols"][0], c["targets"][0])]
    return c


def must_be_undecided(c, e):
    return c["family"] == "edge" and abs(float(c["labels"][e][2:])) < 1


def check(c, out, what=""):
    """out: dict over H.FIELDS of (m, ...) float64 arrays, one call's outputs.  Returns the worst error / bound per
    field, after printing one line per ellipsoid."""
    worst = dict.fromkeys(H.FIELDS, 0.0)
    for e, (val, bnd, sc) in enumerate(c["ref"]):
        r = H.ratios({n: out[n][e] for n in H.FIELDS}, val, bnd, c["rows"])
        branch = ("iso" if sc["iso"] else "greedy") + ("" if sc["decided"] else " (undecided)")
        print(f"scale_hp {what} {c['name']} {c['labels'][e]} [{branch}]: error / bound " +
              "  ".join(f"{n} {r[n]:.3g}" for n in H.FIELDS))
        for n in H.FIELDS:
            worst[n] = max(worst[n], r[n])
    return worst


def golden_arrays():
    names, offs, dh, dl, iso, dec, tg, mb = [], [0], [], [], [], [], [], []
    for f, d in CASES:
        c = case(f, d)
        for e, (_, _, sc) in enumerate(c["ref"]):
            own = H.own(sc)
            names.append(f"{f}/{d}/{c['labels'][e]}")
            dh.append(own["delta"][0])
            dl.append(own["delta"][1])
            offs.append(offs[-1] + d)
            iso.append(sc["iso"])
            dec.append(sc["decided"])
            tg.append(c["targets"][e])
            mb.append(sc["margin"] / sc["dec_bound"])
    return dict(names=np.array(names), offsets=np.array(offs), delta_hi=np.concatenate(dh), delta_lo=np.concatenate(dl),
                iso=np.array(iso), decided=np.array(dec), targets=np.array(tg), margin_over_bound=np.array(mb))


if __name__ == "__main__":
    np.savez_compressed(GOLDEN, **golden_arrays())
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
