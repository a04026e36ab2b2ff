"""dh_friends_update_batch (the resident loop's friends update, one launch per stage over all runs) against
dh_friends_update on each run's points alone: cov, am, axes, axes_inv, the radius and the cluster count bit for bit,
ln V to 1e-14 times max(1, |ln V|) (it may take the device's log / lgamma); runs outside the active mask keep their outputs."""
import numpy as np
import pytest

import inputs
from dynesty_amd.bootstrap import resample_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def run_points(n, d, runs, seed):
    """runs x n x d: d = 2 -> draws from the 13-mode eggbox-like cloud; otherwise two separated blobs."""
    rng = np.random.default_rng(seed)
    out = np.empty((runs, n, d))
    egg = inputs.cloud("c3") if d == 2 else None
    for r in range(runs):
        if d == 2:
            out[r] = egg[rng.choice(len(egg), size=n, replace=False)]
        else:
            na = (3 * n) // 5
            a = 0.3 + 0.02 * rng.standard_normal((na, d))
            b = 0.7 + 0.03 * rng.standard_normal((n - na, d))
            out[r] = np.vstack([a, b])[rng.permutation(n)]
    return out


CASES = [  # kind, n, d, runs, previous metric, bootstrap replicas
    ("balls", 50, 2, 1, False, 0),
    ("cubes", 50, 5, 3, True, 5),
    ("balls", 500, 2, 64, True, 5),
    ("cubes", 500, 2, 64, True, 0),
    ("balls", 500, 32, 64, False, 5),
    ("cubes", 500, 25, 3, True, 5),
    ("balls", 2000, 25, 3, True, 0),
    ("cubes", 2000, 32, 3, True, 5),
    ("balls", 2000, 2, 3, True, 5),
    ("cubes", 2000, 5, 1, False, 0),
]


@pytest.mark.parametrize("kind,n,d,runs,prev,nboot", CASES)
def test_batch_equals_single_updates(ctx, kind, n, d, runs, prev, nboot):
    pts = run_points(n, d, runs, 1000 * n + 10 * d + runs)
    am_prev = None
    if prev:
        # the metric of an earlier update (clustering from the identity), as the loop carries it; at d >= 25 that of
        # an update enlarged by 2^d in volume (am / 4): 500 - 2000 points in the plain one's linkage are mostly
        # singletons, whose re-centred covariance is singular
        am_prev = np.array([ctx.friends_update(p, kind, am_prev=np.eye(d))["am"] for p in pts])
        if d >= 25:
            am_prev = am_prev / 4.0
    masks = None
    if nboot:
        rng = np.random.default_rng(n + d)
        masks = np.array([[resample_mask(n, rng) for _ in range(nboot)] for _ in range(runs)])
    active = np.ones(runs, dtype=bool)
    if runs > 1:
        active[1::3] = False
    sentinel = 7.25
    out = dict(cov=np.full((runs, d, d), sentinel), am=np.full((runs, d, d), sentinel),
               axes=np.full((runs, d, d), sentinel), axes_inv=np.full((runs, d, d), sentinel),
               logvol=np.full(runs, sentinel), rmax=np.full(runs, sentinel),
               nclusters=np.full(runs, -3, dtype=np.int32), status=np.full(runs, -3, dtype=np.int32))
    b = ctx.friends_update_batch(pts, kind, am_prev=am_prev, in_masks=masks, active=active if runs > 1 else None,
                                 out=out)
    ncl = []
    for r in range(runs):
        if not active[r]:
            for k in ("cov", "am", "axes", "axes_inv"):
                assert (b[k][r] == sentinel).all(), (r, k)
            assert b["logvol"][r] == sentinel and b["rmax"][r] == sentinel
            assert b["nclusters"][r] == -3 and b["status"][r] == -3
            continue
        s = ctx.friends_update(pts[r], kind, am_prev=None if am_prev is None else am_prev[r],
                               in_masks=None if masks is None else masks[r])
        assert b["status"][r] == 0, b["status"]
        for k in ("cov", "am", "axes", "axes_inv"):
            np.testing.assert_array_equal(b[k][r], s[k], err_msg=f"run {r} {k}")
        assert b["rmax"][r] == s["rmax"]
        assert b["nclusters"][r] == s["nclusters"]
        assert abs(b["logvol"][r] - s["logvol"]) <= 1e-14 * max(1.0, abs(s["logvol"])), (b["logvol"][r], s["logvol"])
        ncl.append(int(s["nclusters"]))
    if prev and d == 2:
        assert max(ncl) > 1  # the eggbox-like cloud splits into clusters in the previous metric


def test_batch_reports_a_failed_run_and_leaves_the_others(ctx):
    """A run whose points are all equal has a zero covariance: DH_ERR_VALUE for that run alone (the single call
    fails), its outputs untouched; the other runs are as dh_friends_update gives them."""
    from dynesty_amd import _lib
    pts = run_points(64, 3, 3, 5)
    pts[1] = 0.5
    out = ctx.friends_update_batch(pts, "balls", am_prev=np.array([np.eye(3)] * 3))
    assert out["status"].tolist() == [0, _lib.ERR_VALUE, 0]
    assert (out["cov"][1] == 0).all()
    for r in (0, 2):
        s = ctx.friends_update(pts[r], "balls", am_prev=np.eye(3))
        np.testing.assert_array_equal(out["axes"][r], s["axes"])
