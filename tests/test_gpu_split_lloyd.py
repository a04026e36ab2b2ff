"""The Lloyd iteration of a split (node_kmeans_part in csrc/rebuild.hip) against the oracle, at the sizes where its two
forms change path.

A 128-point part (D > 13) runs the WIDE form: one lane per (point, centroid) pair, the label sums' two accumulator
chains on two wavefronts; a 256-point part (D <= 13) keeps one point per thread.  The dimensions are the 16-column
block edges of the label sums (16 | 17, 32 | 33), every remainder class of the distance chain's blocks of eight that
those bring (D & 7 = 6, 0, 1, 1, 0, 1, 4), and the three-block form (D > 32); the sizes give parts of 1, 127 and 128
points, nodes of one, two, three and nine parts, and trees several levels deep.

The reference is the oracle (oracle.bounding_ref.multi_update with its split trace), never the device.  A k-means
label is a comparison of two distances, so before the device is asked the test computes, with NumPy, how close any
point of any iteration of any node comes to a tie: the smallest |d1 - d0| / (d0 + d1) must be above 1e-9 (rounding
differences between the device's fma chain and NumPy's sum are ~1e-15), or the comparison would be of rounding noise.
"""
import functools
import warnings

import numpy as np
import pytest
from scipy.cluster.vq import kmeans2
from scipy.special import logsumexp

from oracle import bounding_ref as B

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # covariances, axis lengths (tests/test_gpu_rebuild.py::test_multi_update_golden)
MIN_MARGIN = 1e-9

DIMS_WIDE = (14, 16, 17, 25, 32, 33, 44)
DIMS_NARROW = (2, 5, 13)


def sizes(d):
    if d in DIMS_NARROW:
        return (255, 256, 257, 513)
    return tuple(sorted({n for n in (4 * d, 4 * d + 1, 127, 128, 129, 255, 256, 257, 385, 513, 1100) if n >= 4 * d}))


CASES = [(d, n) for d in DIMS_WIDE + DIMS_NARROW for n in sizes(d)]


def cloud(d, n, offset=0):
    rng = np.random.default_rng(1000 * d + n + offset)
    x = rng.standard_normal((n, d)) * 0.02 + 0.5
    x[:n // 2, 0] -= 0.07
    x[n // 2:, 0] += 0.07
    return x


def lloyd_margin(x, seeds):
    """kmeans2(x, seeds, iter=10, minit='matrix') restated with NumPy: (labels, smallest |d1 - d0| / (d0 + d1) over
    the iterations and points, iterations until the labels repeat)."""
    cen = seeds.copy()
    margin, prev, its = np.inf, None, 0
    for it in range(10):
        d0 = ((x - cen[0]) ** 2).sum(axis=1)
        d1 = ((x - cen[1]) ** 2).sum(axis=1)
        margin = min(margin, float((np.abs(d1 - d0) / (d0 + d1)).min()))
        lab = (d1 < d0).astype(np.int64)
        its = it + 1
        if prev is not None and np.array_equal(lab, prev):
            break  # a fixed point: the remaining iterations reproduce this one
        prev = lab
        for c in (0, 1):
            if np.any(lab == c):
                cen[c] = x[lab == c].mean(axis=0)
    return lab, margin, its


@functools.lru_cache(maxsize=None)
def reference(d, n, offset=0):
    """The oracle's MultiEllipsoid.update of the cloud: (points, MultiEll, leaf index sets, smallest label margin
    over the tree).  The leaves come from the oracle's recursion restated over index arrays (split_tree,
    bounding.py:1464-1563) and are checked against the oracle proper, node by node through its trace."""
    pts = cloud(d, n, offset)
    pts.setflags(write=False)
    trace = []
    mell = B.multi_update(pts, trace=trace)
    visited = []
    state = dict(margin=np.inf)

    def rec(idx, ell, scale):
        sub = pts[idx]
        m = len(idx)
        if m < 4 * d:
            return [(idx, ell)]
        p1, p2 = B.major_axis_endpoints(ell)
        seeds = np.vstack((p1, p2)) / scale
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, labels = kmeans2(sub / scale, k=seeds, iter=10, minit='matrix', check_finite=False)
        mine, margin, _ = lloyd_margin(sub / scale, seeds)
        assert np.array_equal(mine, labels), "the NumPy restatement of the Lloyd iteration left kmeans2"
        state["margin"] = min(state["margin"], margin)
        visited.append((m, labels))
        parts = [idx[labels == k] for k in (0, 1)]
        if min(len(parts[0]), len(parts[1])) < 2 * d:
            return [(idx, ell)]
        kids = [B.bounding_ellipsoid(pts[p]) for p in parts]
        dec = (d * (d + 3)) // 2 * np.log(m) / m
        out = rec(parts[0], kids[0], scale) + rec(parts[1], kids[1], scale)
        if np.logaddexp(kids[0].logvol, kids[1].logvol) - ell.logvol < -dec:
            return out
        if logsumexp([e.logvol for _, e in out]) - ell.logvol < -dec * (len(out) - 1):
            return out
        return [(idx, ell)]

    leaves = rec(np.arange(n), B.bounding_ellipsoid(pts), pts.std(axis=0)[None, :])
    assert len(visited) == len(trace)
    for (m, labels), tr in zip(visited, trace):
        assert m == tr["npoints"] and np.array_equal(labels, tr["labels"])
    assert len(leaves) == mell.nells
    for (_, e), r in zip(leaves, mell.ells):
        assert np.array_equal(e.ctr, r.ctr)
    return pts, mell, [ix for ix, _ in leaves], state["margin"]


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def match_by_centre(ctrs_a, ctrs_b):
    dist = np.linalg.norm(ctrs_a[:, None, :] - ctrs_b[None, :, :], axis=2)
    p = dist.argmin(axis=1)
    assert len(set(p.tolist())) == len(ctrs_a), "ellipsoid centres do not match one-to-one"
    return p


@pytest.mark.parametrize("d,n", CASES)
def test_split_matches_oracle(ctx, d, n):
    pts, mell, leaves, margin = reference(d, n)
    print(f"d={d} n={n}: nells={mell.nells} smallest label margin={margin:.3g}")
    assert margin > MIN_MARGIN, f"a label of this cloud is decided by rounding (margin {margin:.3g})"
    got = ctx.rebuild(pts, multi=True, want_labels=True)
    assert got["nells"] == mell.nells
    # the leaf partition, as a partition
    lab = got["labels"]
    assert lab.min() >= 0 and lab.max() == got["nells"] - 1
    ref_sets = {frozenset(ix.tolist()) for ix in leaves}
    assert len(ref_sets) == len(leaves)
    for i in range(got["nells"]):
        mine = frozenset(np.flatnonzero(lab == i).tolist())
        assert mine in ref_sets, f"device cluster {i} is not a leaf of the oracle's tree"
        ref_sets.discard(mine)
    assert not ref_sets
    # the ellipsoids, matched by centre (the child order follows an eigenvector's sign)
    p = match_by_centre(got["ctrs"], mell.ctrs)
    for i in range(got["nells"]):
        e = mell.ells[p[i]]
        np.testing.assert_allclose(got["ctrs"][i], e.ctr, rtol=0, atol=1e-13)
        np.testing.assert_allclose(got["covs"][i], e.cov, rtol=RTOL, atol=RTOL * np.abs(e.cov).max())
        np.testing.assert_allclose(got["logvol_ells"][i], e.logvol, rtol=0, atol=1e-9)


def test_batch_equals_single_calls(ctx):
    """16 clouds of d = 25, n = 1100 in one launch: many nine-part nodes exchanging their partial sums at once.  Every
    run must equal its single-call result bit for bit (and the first of them the oracle, above)."""
    sets = [cloud(25, 1100, k) for k in range(16)]
    many = ctx.rebuild_many(sets)
    for k, pts in enumerate(sets):
        one = ctx.rebuild(pts, multi=True)
        assert many[k]["nells"] == one["nells"], k
        for key in ("ctrs", "covs", "ams", "axes", "axlens", "logvol_ells"):
            assert np.array_equal(many[k][key], one[key]), (k, key)
