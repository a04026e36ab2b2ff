"""Seeded inputs of the ellipsoid linear-algebra checks (tests/ell_hp_ref.py, tests/test_ell_hp_cpu.py,
tests/test_gpu_ell_hp.py, tools/make_golden.py ell_hp): live-point clouds and covariance matrices whose spectra
walk the condition number through the places where the rebuild kernels change route.  Everything is regenerated
from the seed, as tests/inputs.py does, so tests/golden/ell_hp.npz holds outputs only.

A cloud is  0.5 + s * Z * diag(sqrt(lam)) * Q^T :  Z an n x D standard-normal draw, Q a random rotation, s the
largest scale that keeps every point inside the cube (or 1e-7: the width of a live set towards the end of a run).
For every spectrum but the flat one Z is centred and whitened first (its sample covariance is the identity to
rounding), so that the cloud's sample spectrum IS s^2 * lam and not a Wishart draw around it -- a leading pair 1e-9
apart stays 1e-9 apart.  "flat" keeps the draw as it is (a nearly isotropic covariance with a spectrum of its own, as
a real live set has); "iso" is the whitened flat cloud: D eigenvalues equal to rounding, a covariance that is
diagonal before the solver starts.
"""
import zlib

import numpy as np

DIMS = (1, 2, 3, 9, 10, 13, 14, 16, 17, 22, 23, 28, 29, 32, 33, 43, 44)  # every route change of D <= 44
DIMS_N = (13, 14, 25, 44)  # these also get the tile-edge sizes below
SIZES_N = (255, 256, 257, 513)  # parts of one, two and three 256-point tiles
WIDE_DIMS = (45, 64, 96)
MAT_DIMS = tuple(range(1, 45))

GAPS = ("gap1e-3", "gap1e-6", "gap1e-9", "gap1e-12")
GEO = ("geo1e3", "geo1e6", "geo1e9", "geo1e11")
POSITIVE = ("flat",) + GEO + ("trlo", "trhi", "dom") + GAPS
CLOUD_KINDS = POSITIVE + ("iso", "geo1e13", "rank3", "dup6", "flat@1e-7", "geo1e6@1e-7")
WIDE_KINDS = ("flat", "geo1e6", "geo1e13", "gap1e-9")
MAT_KINDS = POSITIVE + ("neg", "negdef", "zero", "geo1e13", "eye", "diagdesc", "flat*2^400", "geo1e6*2^400",
                        "flat*2^-400", "geo1e6*2^-400")
TIGHT_FAMILIES = ("flat", "geo1e3", "geo1e6")  # where the existing suite's hand-set tolerances apply


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) + 0x5EED


def _geo(d, kappa):
    return kappa ** (-np.arange(d) / (d - 1.0))


def _tr_product_kappa(d, target):
    """kappa of the geometric spectrum whose tr(lam) * tr(1 / lam) is `target` (bisection on log kappa)."""
    lo, hi = 0.0, 30.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lam = _geo(d, 10.0**mid)
        if lam.sum() * (1.0 / lam).sum() < target:
            lo = mid
        else:
            hi = mid
    return 10.0**(0.5 * (lo + hi))


def spectrum(kind, d):
    """Population spectrum, largest first, lam_max = 1; None where D does not allow the kind."""
    kind = kind.split("@")[0].split("*")[0]
    if kind == "negdef":  # nothing positive: the identity blend runs until the top eigenvalue is
        return -np.linspace(0.2, 1.0, d)
    if kind in ("flat", "iso", "dup6", "eye"):
        return np.ones(d)
    if d < 2:
        return None
    if kind.startswith("geo"):
        return _geo(d, float(kind[3:]))
    if kind == "trlo":
        return _geo(d, _tr_product_kappa(d, 0.3e7))
    if kind == "trhi":
        return _geo(d, _tr_product_kappa(d, 3e7))
    if kind == "dom":
        return np.concatenate([[1.0], np.full(d - 1, 1e-4)])
    if kind.startswith("gap"):
        gap = float(kind[3:])
        return np.concatenate([[1.0, 1.0 - gap], np.full(d - 2, 0.1)])
    if kind == "neg":  # one negative eigenvalue under a positive top: floored, not blended
        lam = np.linspace(1.0, 0.2, d)
        lam[-1] = -0.5
        return lam
    raise KeyError(kind)


def _rotation(rng, d):
    q, r = np.linalg.qr(rng.standard_normal((d, d)))
    return q * np.sign(np.diag(r))


def _whitened(rng, n, d):
    z = rng.standard_normal((n, d))
    z -= z.mean(axis=0)
    for _ in range(2):  # the second pass removes the rounding of the first
        z = z @ np.linalg.inv(np.linalg.cholesky(np.cov(z, rowvar=False).reshape(d, d))).T
        z -= z.mean(axis=0)
    return z


def cloud_size(kind, d):
    if kind == "dup6":
        return 6 * max(d + 8, 22)  # the distinct points alone must span the space
    return max(5 * d, 130)


def cloud(kind, d, n=None):
    """(n, D) float64 points inside the unit cube, or None where D does not allow the kind."""
    if n is None:
        n = cloud_size(kind, d)
    rng = np.random.default_rng(_seed("cloud", kind, d, n))
    if kind == "rank3":
        if d < 5:
            return None
        # exactly rank 3: dyadic coordinates times a dyadic basis, so every product and sum below is exact in
        # fp64 and the points lie IN a 3-D affine subspace (the null space of the covariance is exact)
        z = np.round(np.clip(rng.standard_normal((n, 3)), -3.5, 3.5) * 2.0**12) / 2.0**12
        basis = np.round(rng.uniform(-1.0, 1.0, (3, d)) * 8.0) / 8.0
        basis[:, :3] += np.eye(3)
        return 0.5 + (z @ basis) / 64.0
    lam = spectrum(kind, d)
    if lam is None:
        return None
    if kind == "dup6":
        z = np.repeat(_whitened(rng, n // 6, d), 6, axis=0)[rng.permutation(n)]
    elif kind.split("@")[0] == "flat":
        z = rng.standard_normal((n, d))
    else:
        z = _whitened(rng, n, d)
    x = (z * np.sqrt(lam)) @ _rotation(rng, d).T
    width = 1e-7 if kind.endswith("@1e-7") else 0.45
    return 0.5 + x * (width / np.abs(x).max())


def cloud_cases():
    """[(key, kind, d, n)] of every cloud of the narrow path (D <= 44)."""
    out = []
    for d in sorted(set(DIMS) | {25}):
        for kind in CLOUD_KINDS:
            if (d < 5) if kind == "rank3" else (spectrum(kind, d) is None):
                continue
            out.append((f"cl/{d}/{kind}", kind, d, cloud_size(kind, d)))
    for d in DIMS_N:
        for n in SIZES_N:
            for kind in ("flat", "geo1e6"):
                out.append((f"cl/{d}/{kind}/n{n}", kind, d, n))
    return out


def wide_cases():
    return [(f"wd/{d}/{kind}", kind, d, 6 * d) for d in WIDE_DIMS for kind in WIDE_KINDS]


def matrix(kind, d):
    """One symmetric D x D float64 matrix, or None where D does not allow the kind."""
    rng = np.random.default_rng(_seed("mat", kind, d))
    if kind == "zero":
        return np.zeros((d, d))
    if kind == "eye":
        return np.eye(d)
    if kind == "diagdesc":
        return np.diag(0.01 * np.arange(d, 0, -1.0))
    lam = spectrum(kind, d)
    if lam is None:
        return None
    q = _rotation(rng, d)
    a = (q * (0.01 * lam)) @ q.T
    a = 0.5 * (a + a.T)
    if "*2^" in kind:
        a = np.ldexp(a, int(kind.split("*2^")[1]))
    return a


def matrix_cases(d):
    """[(key, kind)] of the stack of dimension d, in stack order."""
    return [(f"mt/{d}/{kind}", kind) for kind in MAT_KINDS if matrix(kind, d) is not None]


def is_positive_kind(kind):
    return kind.split("*")[0] in POSITIVE or kind in ("eye", "diagdesc")
