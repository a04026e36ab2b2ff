"""Clouds for the split tree's high-precision tests (tests/split_hp_ref.py, tests/test_split_hp_cpu.py,
tests/test_gpu_split_hp.py): the smallest shapes at which every path of MultiEllipsoid.update's recursion is still
taken.  Everything is regenerated from a seed; tests/golden/split_hp.npz holds results only.

A case is (key, family, d, n, k): key 'family/d/n[/k]'; k is the side blob's size (0 elsewhere).

  dimensions  2, 3, 5, 9, 13        256-point parts, the wave-level child ellipsoid
              14, 17, 25, 33, 44    128-point parts, the whole-workgroup Lloyd form either side of its 16-column blocks
              45, 64                the wide path's host recursion
  sizes       4 d - 1, 4 d, 4 d + 1 at one d per group (5, 17, 45): the split threshold from both sides, and children
              of exactly 2 d points; 513 at d <= 13 and 257, 1100 at d = 25: nodes of 2 to 9 parts; max(8 d, 300)
              elsewhere
"""
import zlib

import numpy as np

GROUPS = ((2, 3, 5, 9, 13), (14, 17, 25, 33, 44), (45, 64))
FAMILIES = ("blobs", "ring", "parabola", "aniso", "overlap", "box", "side", "narrow", "cross", "outlier")


def group_of(d):
    return next(g for g, dims in enumerate(GROUPS) if d in dims)


def part_points(d):
    """Points per part of a k-means node (csrc/rebuild.hip: 256 up to d = 13, 128 above; the wide path has no parts)."""
    return 256 if d <= 13 else 128


def _seed(family, d, n, k):
    return zlib.crc32(f"split/{family}/{d}/{n}/{k}".encode())


def cloud(family, d, n, k=0):
    if family == "blobs":
        # the family of tests/test_gpu_split_lloyd.py, seed and all
        rng = np.random.default_rng(1000 * d + n)
        x = rng.standard_normal((n, d)) * 0.02 + 0.5
        x[:n // 2, 0] -= 0.07
        x[n // 2:, 0] += 0.07
        return x
    rng = np.random.default_rng(_seed(family, d, n, k))
    if family == "ring":
        # three quarters of a ring in coordinates 0, 1
        x = rng.standard_normal((n, d)) * 0.02 + 0.5
        th = rng.uniform(0.0, 1.5 * np.pi, n)
        r = 0.3 + 0.01 * rng.standard_normal(n)
        x[:, 0] = 0.5 + r * np.cos(th)
        x[:, 1] = 0.5 + r * np.sin(th)
        return x
    if family == "parabola":
        x = rng.standard_normal((n, d)) * 0.02 + 0.5
        u = rng.uniform(-0.4, 0.4, n)
        x[:, 0] = 0.5 + u
        x[:, 1] = 0.15 + 4.0 * u * u + 0.01 * rng.standard_normal(n)
        return x
    if family == "aniso":
        # sigma 0.01; coordinate 1 uniform over +-0.4; two halves +-0.04 apart in coordinate 0: the major axis is
        # coordinate 1, the structure is in coordinate 0, and only the per-coordinate scale lets k-means see it
        x = rng.standard_normal((n, d)) * 0.01 + 0.5
        x[:, 1] = 0.5 + rng.uniform(-0.4, 0.4, n)
        x[:n // 2, 0] -= 0.04
        x[n // 2:, 0] += 0.04
        return x
    if family == "overlap":
        # two blobs 2.5 sigma apart: labels keep moving
        x = rng.standard_normal((n, d)) * 0.02 + 0.5
        x[:n // 2, 0] -= 0.025
        x[n // 2:, 0] += 0.025
        return x
    if family == "box":
        return rng.uniform(0.1, 0.9, (n, d))
    if family == "side":
        # a blob of n - k points and a tight side blob of k points 15 sigma away along a diagonal of coordinates 0, 1
        x = rng.standard_normal((n, d)) * 0.02 + 0.4
        x[n - k:] = rng.standard_normal((k, d)) * 0.005 + 0.4
        x[n - k:, 0] += 0.3
        x[n - k:, 1] += 0.2
        return x
    if family == "narrow":
        # two blobs of width 1e-7 about 0.3
        z = rng.standard_normal((n, d))
        z[:n // 2, 0] -= 3.5
        z[n // 2:, 0] += 3.5
        return 0.3 + 1e-7 * z
    if family == "cross":
        # two blobs 0.2 apart in coordinate 0, each thin (sigma 0.002) in the half of the coordinates in which the
        # other is wide (sigma 0.02): the union's ellipsoid is wide everywhere, so the split is accepted at any d
        # (two round blobs are not split above d ~ 10: dec grows like d^2 ln(n) / n, the gain only like ln(gap / sigma))
        h = d // 2
        sig = np.full((n, d), 0.002)
        sig[:n // 2, :h] = 0.02
        sig[n // 2:, h:] = 0.02
        x = rng.standard_normal((n, d)) * sig + 0.5
        x[:n // 2, 0] -= 0.1
        x[n // 2:, 0] += 0.1
        return x
    if family == "outlier":
        # one point far from a tight blob: a cluster of ONE point, the nearest a cloud comes to an empty cluster (the
        # seeds' bisector passes through the mean, so both sides hold points; afterwards each centroid is the mean of
        # its own members, one of which is then on its side: k = 2 Lloyd from these seeds never empties a cluster)
        x = rng.standard_normal((n, d)) * 0.01 + 0.3
        x[n // 3, 0] += 0.5
        x[n // 3, 1] += 0.3
        return x
    raise ValueError(family)


def _cases():
    c = []
    for d, n in ((2, 513), (5, 19), (5, 20), (5, 21), (13, 513), (17, 67), (17, 68), (17, 69), (25, 257), (25, 1100),
                 (44, 352), (45, 179), (45, 180), (45, 181), (45, 364), (64, 516)):
        c.append(("blobs", d, n, 0))
    for d, n in ((2, 513), (3, 513), (9, 513), (14, 300), (33, 300)):
        c.append(("ring", d, n, 0))
    for d, n in ((3, 513), (5, 300), (17, 300)):
        c.append(("parabola", d, n, 0))
    for d, n in ((3, 513), (13, 300), (25, 257)):
        c.append(("aniso", d, n, 0))
    for d, n in ((2, 513), (9, 300), (25, 300), (44, 352)):
        c.append(("overlap", d, n, 0))
    for d, n in ((3, 300), (25, 1100), (33, 300)):
        c.append(("box", d, n, 0))
    for d, n in ((3, 300), (9, 600), (14, 300)):
        for k in (2 * d - 1, 2 * d, 2 * d + 3):
            c.append(("side", d, n, k))
    for d, n in ((5, 300), (25, 300)):
        c.append(("narrow", d, n, 0))
    for d, n in ((14, 300), (25, 1100), (33, 300), (44, 352), (45, 364), (64, 516)):
        c.append(("cross", d, n, 0))
    for d, n in ((3, 300), (14, 300)):
        c.append(("outlier", d, n, 0))
    return [(f"{f}/{d}/{n}" + (f"/{k}" if k else ""), f, d, n, k) for f, d, n, k in c]


CASES = _cases()
KEYS = [c[0] for c in CASES]


def case(key):
    return CASES[KEYS.index(key)]


def points(key):
    _, f, d, n, k = case(key)
    x = cloud(f, d, n, k)
    x.setflags(write=False)
    return x


# ---- bootstrap expansion (dh_bootstrap_expand) ----
BOOT_B = 3
BOOT_CASES = [(f"boot/{f}/{d}/{n}/{'multi' if multi else 'single'}", f, d, n, multi)
              for f, d, n in (("ring", 2, 130), ("blobs", 5, 200), ("ring", 14, 300), ("blobs", 25, 260),
                              ("ring", 5, 150), ("blobs", 14, 180))
              for multi in (False, True)]


def boot_entropy(key):
    """The four 64-bit words a run would have drawn for this rebuild."""
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    return rng.integers(0, 2**63, size=4, dtype=np.uint64)
