"""Seeded inputs of the RadFriends / SupFriends checks (tests/friends_hp_ref.py, tests/test_friends_hp_cpu.py,
tests/test_gpu_friends_hp.py, tools/make_golden.py friends_hp).  Everything comes from numpy.random.default_rng and a
seed made of the case's name, so tests/golden/friends_hp.npz holds outputs only.

The shapes are the smallest at which an edge of friends.hip exists, not the workload's: every dimension of DIMS (1; the
resident loop's limit 32 | 33; fr_shape's LDS crossing 64 KB at 51 | 52; the three statements of the clustering limit
60, 63, 64; one coordinate per lane at 64), point counts on the 64-lane tile, the 256-thread block and the 1024-thread
stride of fr_components.  A cloud serves both kinds (balls, cubes): they differ in the norm of the radius only.

Left out on purpose: clouds that are rank deficient by rounding (a `flat10`-like cloud of more dimensions than
points spans, whose smallest eigenvalue lands inside the cutoff band d eps lam_max): there either answer is defensible.
The failing cases here have a coordinate that is constant, hence an exactly zero row, column and eigenvalue.
"""
import zlib

import numpy as np

from ell_cases import _geo, _rotation, _whitened

DIMS = (1, 2, 3, 8, 25, 31, 32, 33, 51, 52, 60, 63, 64)
N_EDGES = (63, 64, 65, 255, 256, 257, 1025)
CLUSTER_DMAX = 63  # fr_adjacency's LDS (d^2 + 4 * 65 d) * 8 bytes fits the 160 KB of a CU up to here
KINDS = ("balls", "cubes")


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) + 0xF51E


def cloud(name, d, n):
    """(n, d) float64 points of the family `name`."""
    rng = np.random.default_rng(_seed("cloud", name, d, n))
    if name == "iso":
        return 0.5 + 0.1 * rng.standard_normal((n, d))
    if name == "tail":  # the isotropic cloud, ordered so that the radius hangs on the LAST point
        # the loneliest point (largest nearest-neighbour distance of the whitened cloud) goes first and its nearest
        # neighbour last: a candidate loop that loses its last partial tile returns another radius
        x = 0.5 + 0.1 * rng.standard_normal((n, d))
        lam, vec = np.linalg.eigh(np.atleast_2d(np.cov(x, rowvar=False)))
        y = x @ (vec / np.sqrt(lam)) @ vec.T
        dist = np.sqrt(((y[:, None, :] - y[None, :, :])**2).sum(-1))
        np.fill_diagonal(dist, np.inf)
        i = int(np.argmax(dist.min(axis=1)))
        j = int(np.argmin(dist[i]))
        rest = [k for k in range(n) if k not in (i, j)]
        return x[[i] + rest + [j]]
    if name == "late":  # a live set towards the end of a run: width 1e-7 around 0.5
        return 0.5 + 1e-7 * rng.standard_normal((n, d))
    if name.startswith("corr"):  # sample spectrum = geometric, kappa as named (whitened draw, as ell_cases does it)
        lam = _geo(d, float(name[4:]))
        x = (_whitened(rng, n, d) * np.sqrt(lam)) @ _rotation(rng, d).T
        return 0.5 + x * (0.45 / np.abs(x).max())
    if name.startswith("blobs"):  # k separated blobs of width 0.01, shuffled
        k = int(name[5:])
        ctr = 0.15 + 0.7 * rng.permutation(k)[:, None] / (k - 1.0) + 0.02 * rng.uniform(-1, 1, (k, d))
        own = np.arange(n) % k
        return (ctr[own] + 0.01 * rng.standard_normal((n, d)))[rng.permutation(n)]
    if name in ("chain", "chain_shuffled"):  # a chain whose links are 0.6 long in the previous metric
        t = np.arange(n)[:, None] * (0.9 / n) / np.sqrt(d)
        x = 0.05 + t + (0.03 / n) * np.random.default_rng(_seed("cloud", "chain", d, n)).uniform(-1, 1, (n, d))
        return x if name == "chain" else x[rng.permutation(n)]
    if name == "dup":  # the first half in triples (nearest-neighbour distance 0 for those; the radius from the rest)
        base = 0.5 + 0.1 * rng.standard_normal((n, d))
        idx = np.arange(n)
        for i in range(0, n // 2 - 2, 3):
            idx[i + 1] = idx[i + 2] = i
        return base[idx][rng.permutation(n)]
    if name == "const":  # the last coordinate is the same number in every point
        x = 0.5 + 0.1 * rng.standard_normal((n, d))
        x[:, -1] = 0.375
        return x
    raise KeyError(name)


def prev_metric(name, d, n):
    """The metric of the PREVIOUS bound for the clustering, or None (use_clustering=False).  Never one a radius of
    these points was derived from (that knife edge stays with tests/test_gpu_friends.py): a mildly anisotropic matrix
    Q diag(1 / s_k^2) Q^T whose scale s links neighbours of one blob / the chain and nothing else."""
    rng = np.random.default_rng(_seed("prev", name, d, n))
    if name.startswith("blobs"):
        s = 0.01 * (1.5 * np.sqrt(2.0 * d) + 2.0)
    elif name.startswith("chain"):
        s = (0.9 / n) / 0.6
    elif name == "late":
        s = 1e-7 * (2.0 * np.sqrt(2.0 * d) + 4.0)
    else:  # one cluster: every pair well inside the threshold
        s = 0.1 * (3.0 * np.sqrt(2.0 * d) + 8.0)
    q = _rotation(rng, d)
    a = (q * (rng.uniform(0.8, 1.25, d) / s**2)) @ q.T
    return 0.5 * (a + a.T)


def _mask_spec(n):
    """Which bootstrap masks the n-edge series carries at this n (see masks())."""
    return {63: "boot1", 64: "boot5", 65: "tile64", 255: "full1of5", 256: "single", 257: "block256",
            1025: "tile64"}[n]


def masks(spec, n):
    """(B, n) bool in-sample masks (True = resampled), or None for the leave-one-out radius."""
    if spec is None:
        return None
    from dynesty_amd.bootstrap import resample_mask
    rng = np.random.default_rng(_seed("mask", spec, n))
    if spec == "boot1":
        return np.array([resample_mask(n, rng)])
    if spec == "boot5":
        return np.array([resample_mask(n, rng) for _ in range(5)])
    if spec == "full1of5":  # replica 2 leaves nothing out: it contributes nothing
        m = np.array([resample_mask(n, rng) for _ in range(5)])
        m[2] = True
        return m
    m = np.ones((1, n), dtype=bool)
    if spec == "single":
        m[0, n // 3] = False
    elif spec == "tile64":  # left-out points only in the last partial tile of 64 (every other point of it)
        m[0, 64 * ((n - 1) // 64)::2] = False
    elif spec == "block256":  # ... only in the last partial block of 256
        m[0, 256 * ((n - 1) // 256):] = False
    else:
        raise KeyError(spec)
    return m


def update_cases():
    """[(key, cloud name, d, n, clustering, mask spec, fails)], one list for both kinds."""
    out = []

    def add(name, d, n, clustering=True, spec=None, fails=False):
        clustering = clustering and d <= CLUSTER_DMAX
        key = f"{name}/{d}/{n}" + ("/c" if clustering else "") + (f"/{spec}" if spec else "")
        assert n > d and key not in [c[0] for c in out], key
        out.append((key, name, d, n, clustering, spec, fails))

    add("iso", 1, 2, clustering=False)
    for i, d in enumerate(DIMS):
        add("iso", d, d + 2, clustering=False)  # every d at a small n ...
        big = [n for n in N_EDGES[:6] if n > d + 2]
        add("iso", d, big[i % len(big)], spec=("boot5", None, "boot1")[i % 3])  # ... and at a large one
    for d in (2, 60):  # every n edge at a small and a large d
        for n in N_EDGES:
            add("iso", d, n, spec=_mask_spec(n))
            add("tail", d, n)  # leave-one-out, the radius on the last candidate
    add("iso", 64, 1025, spec="boot1")
    for name, dims in (("corr1e3", (2, 8, 33, 64)), ("corr1e8", (3, 25, 52)), ("corr1e12", (2, 8, 31))):
        for d in dims:
            add(name, d, 65 if d < 60 else 129, clustering=d % 2 == 0)
    for d in (1, 3, 32, 64):
        add("late", d, 130)
    for name, dn in (("blobs2", ((2, 65), (25, 257), (63, 129))), ("blobs5", ((3, 63), (32, 256), (60, 255)))):
        for d, n in dn:
            add(name, d, n, spec="boot5" if d > 30 else None)
    add("chain", 2, 1025)
    add("chain_shuffled", 2, 1025)
    add("dup", 2, 66)
    add("dup", 33, 129, spec="boot1")
    for d, n in ((2, 64), (33, 65), (64, 130)):
        add("const", d, n, clustering=d == 33, fails=True)
    return out


# ---- membership -----------------------------------------------------------------------------------------------------
RING = (1e-3, 1e-6, 1e-9)
WITHIN_SHAPES = ((1, 65), (63, 63), (64, 1), (65, 65), (129, 63))  # (centres, probes)


def within_cases():
    """[(key, cloud name, d, n centres, m probes)]"""
    out = []
    for d in (1, 3, 33, 64):
        for n, m in WITHIN_SHAPES:
            out.append((f"w/iso/{d}/{n}/{m}", "iso", d, n, m))
    for d in (3, 64):
        for n, m in ((65, 65), (129, 63)):
            out.append((f"w/late/{d}/{n}/{m}", "late", d, n, m))
    return out


def within_inputs(name, d, n, m, kind):
    """Centres (the first n points of a 130-point cloud), the fp64 axes / axes_inv of that cloud's own bound (float64
    NumPy: input data, an exact datum for the reference from there on), and m probes: rays from a centre to whitened
    distance 1 -+ RING (balls: random directions; cubes: three face normals and three diagonals) as far as m allows,
    then random points of the union.  Returns dict(ctrs, axes, axes_inv, x, ring (m,) the offset aimed at or 0)."""
    pts = cloud(name, d, 130)
    cov = np.atleast_2d(np.cov(pts, rowvar=False))
    lam, vec = np.linalg.eigh(cov)
    y = pts @ ((vec / np.sqrt(lam)) @ vec.T)
    if kind == "balls":
        dist = np.sqrt(((y[:, None, :] - y[None, :, :])**2).sum(-1))
    else:
        dist = np.abs(y[:, None, :] - y[None, :, :]).max(-1)
    np.fill_diagonal(dist, np.inf)
    r = dist.min(axis=1).max()
    axes = (vec * (np.sqrt(lam) * r)) @ vec.T
    axes_inv = (vec / (np.sqrt(lam) * r)) @ vec.T
    axes, axes_inv = 0.5 * (axes + axes.T), 0.5 * (axes_inv + axes_inv.T)
    ctrs = pts[:n]
    rng = np.random.default_rng(_seed("probe", name, d, n, m, kind))
    xs, ring = [], []
    for ray in range(6):
        if kind == "balls":
            u = rng.standard_normal(d)
            u /= np.linalg.norm(u)
        elif ray < 3:  # a face normal
            u = np.zeros(d)
            u[rng.integers(d)] = rng.choice([-1.0, 1.0])
        else:  # a diagonal
            u = rng.choice([-1.0, 1.0], size=d)
        c = ctrs[rng.integers(n)]
        for off in RING:
            for sign in (-1.0, 1.0):
                xs.append(c + (1.0 + sign * off) * (u @ axes))
                ring.append(sign * off)
    while len(xs) < m:
        u = rng.standard_normal(d)
        u *= rng.uniform()**(1.0 / d) / (np.linalg.norm(u) if kind == "balls" else np.abs(u).max())
        xs.append(ctrs[rng.integers(n)] + 1.3 * (u @ axes))
        ring.append(0.0)
    # the rings come first: m = 1 is the probe at 1 - 1e-3
    return dict(ctrs=ctrs, axes=axes, axes_inv=axes_inv, x=np.array(xs[:m]), ring=np.array(ring[:m]))
