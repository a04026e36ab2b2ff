"""friends.hip against the high-precision reference tests/friends_hp_ref.py, at the shapes tests/friends_cases.py lists:
every d of 1 ... 64 where a route or a limit changes, n on the tile, block and stride edges, correlated, late-run,
clustered, chained, duplicated and singular clouds, bootstrap masks that leave out nothing, one point or only the tail.

Updates of one (kind, n, d, clustering, replicas) go through ONE dh_friends_update_batch call (pinned bit for bit to
the single call up to d = 32 by tests/test_gpu_friends_batch.py, and at d = 33 and 64 here); groups with d > 32 and the
n = 2 case go through dh_friends_update.  Every case prints its error / bound line; test_report_worst prints the worst
per entry point and kind.
"""
import numpy as np
import pytest

import friends_cases as FC
import friends_hp_ref as R
from ell_hp_ref import Ratios
from oracle import friends_ref as F

pytestmark = pytest.mark.gpu

WORST = {}
SENTINEL = 7.25


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def fix():
    return R.load_fixture()


def _groups():
    g = {}
    for case in FC.update_cases():
        key, name, d, n, clustering, spec, fails = case
        nb = 0 if spec is None else len(FC.masks(spec, n))
        g.setdefault((n, d, clustering, nb), []).append(case)
    return g


GROUPS = _groups()


def _note(entry, kind, r):
    WORST.setdefault((entry, kind), Ratios()).merge(r)


def _sentinel_out(runs, d):
    return dict(cov=np.full((runs, d, d), SENTINEL), am=np.full((runs, d, d), SENTINEL),
                axes=np.full((runs, d, d), SENTINEL), axes_inv=np.full((runs, d, d), SENTINEL),
                logvol=np.full(runs, SENTINEL), rmax=np.full(runs, SENTINEL),
                nclusters=np.full(runs, -3, dtype=np.int32), status=np.full(runs, -3, dtype=np.int32))


def _batch(ctx, cases, kind):
    n, d = cases[0][3], cases[0][2]
    pts = np.array([FC.cloud(c[1], d, n) for c in cases])
    prev = np.array([FC.prev_metric(c[1], d, n) for c in cases]) if cases[0][4] else None
    masks = np.array([FC.masks(c[5], n) for c in cases]) if cases[0][5] else None
    out = ctx.friends_update_batch(pts, kind, am_prev=prev, in_masks=masks, out=_sentinel_out(len(cases), d))
    return pts, prev, masks, out


@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("gkey", sorted(GROUPS), ids=lambda k: f"n{k[0]}-d{k[1]}-{'c' if k[2] else 'nc'}-b{k[3]}")
def test_update_within_bounds(ctx, fix, gkey, kind):
    from dynesty_amd import _lib
    urec, _ = fix
    cases = GROUPS[gkey]
    n, d = gkey[0], gkey[1]
    single = d > 32 or n == 2
    pts, prev, masks, out = _batch(ctx, cases, kind)
    for i, case in enumerate(cases):
        key, fails, rec = case[0], case[6], urec[case[0]]
        mk = None if masks is None else masks[i].astype(bool)
        if fails:
            # DH_ERR_VALUE for that run alone, its outputs untouched (the batch); ValueError from the single call, whose
            # output arrays include/dynhip.h leaves unspecified on error
            assert out["status"][i] == _lib.ERR_VALUE, (key, out["status"])
            for k in ("cov", "am", "axes", "axes_inv", "logvol", "rmax"):
                assert np.all(out[k][i] == SENTINEL), (key, k)
            assert out["nclusters"][i] == -3
            with pytest.raises(ValueError):
                ctx.friends_update(pts[i], kind, am_prev=None if prev is None else prev[i], in_masks=mk)
            continue
        assert out["status"][i] == 0, (key, out["status"])
        res = {k: out[k][i] for k in ("cov", "am", "axes", "axes_inv", "logvol", "rmax", "nclusters")}
        entry = "update_batch"
        if single:
            res = ctx.friends_update(pts[i], kind, am_prev=None if prev is None else prev[i], in_masks=mk)
            entry = "update"
        r = R.check_update(pts[i], kind, mk, res, rec, rec["labels"])
        _note(entry, kind, r)
        R.assert_ok(r, f"{entry} {key}/{kind}")
        if single:  # the batch's answer is held too: it is the resident loop's route
            rb = R.check_update(pts[i], kind, mk, {k: out[k][i] for k in res}, rec, rec["labels"])
            _note("update_batch", kind, rb)
            R.assert_ok(rb, f"update_batch {key}/{kind}")


@pytest.mark.parametrize("kind,d,n,prev,nboot", [("balls", 33, 65, True, 5), ("cubes", 33, 130, False, 0),
                                                 ("balls", 64, 130, False, 5), ("cubes", 64, 65, False, 0),
                                                 ("cubes", 63, 65, True, 1)])
def test_batch_equals_single_above_32(ctx, kind, d, n, prev, nboot):
    """tests/test_gpu_friends_batch.py's identity above the resident loop's d = 32: cov, am, axes, axes_inv, the radius
    and the cluster count bit for bit, ln V to 1e-14 max(1, |ln V|); an inactive run keeps its outputs."""
    from dynesty_amd.bootstrap import resample_mask
    runs = 3
    pts = np.array([FC.cloud("iso", d, n), FC.cloud("blobs2", d, n), FC.cloud("late", d, n)])
    am_prev = np.array([FC.prev_metric(nm, d, n) for nm in ("iso", "blobs2", "late")]) if prev else None
    rng = np.random.default_rng(d + n)
    masks = np.array([[resample_mask(n, rng) for _ in range(nboot)] for _ in range(runs)]) if nboot else None
    active = np.array([True, False, True])
    b = ctx.friends_update_batch(pts, kind, am_prev=am_prev, in_masks=masks, active=active, out=_sentinel_out(runs, d))
    for r in range(runs):
        if not active[r]:
            assert all(np.all(b[k][r] == SENTINEL) for k in ("cov", "am", "axes", "axes_inv", "logvol", "rmax"))
            assert b["nclusters"][r] == -3 and b["status"][r] == -3
            continue
        s = ctx.friends_update(pts[r], kind, am_prev=None if am_prev is None else am_prev[r],
                               in_masks=None if masks is None else masks[r])
        assert b["status"][r] == 0
        for k in ("cov", "am", "axes", "axes_inv"):
            np.testing.assert_array_equal(b[k][r], s[k], err_msg=f"run {r} {k}")
        assert b["rmax"][r] == s["rmax"] and b["nclusters"][r] == s["nclusters"]
        assert abs(b["logvol"][r] - s["logvol"]) <= 1e-14 * max(1.0, abs(s["logvol"]))


def test_clustering_limit(ctx, fix):
    """d = 63 with a previous metric is served (the cases of test_update_within_bounds hold its results to the
    bounds); d = 64 with one is DH_ERR_ARG whose message names that limit, from both entry points; d = 64 without
    works; and the context is as usable afterwards as before."""
    from dynesty_amd import _lib
    small = FC.cloud("iso", 3, 65)
    before = ctx.friends_update(small, "balls", am_prev=FC.prev_metric("iso", 3, 65))
    pts = FC.cloud("iso", 64, 130)
    for call in (lambda: ctx.friends_update(pts, "balls", am_prev=FC.prev_metric("iso", 64, 130)),
                 lambda: ctx.friends_update_batch(pts[None], "cubes", am_prev=FC.prev_metric("iso", 64, 130)[None])):
        with pytest.raises(_lib.DynHipError) as err:
            call()
        assert f"error {_lib.ERR_ARG}" in str(err.value) and f"d <= {FC.CLUSTER_DMAX}" in str(err.value), str(err.value)
        after = ctx.friends_update(small, "balls", am_prev=FC.prev_metric("iso", 3, 65))
        for k in ("cov", "am", "axes", "axes_inv"):
            np.testing.assert_array_equal(after[k], before[k])
    assert ctx.friends_update(pts, "balls", am_prev=None)["rmax"] > 0
    assert ctx.friends_update(FC.cloud("iso", FC.CLUSTER_DMAX, 65), "balls",
                              am_prev=FC.prev_metric("iso", FC.CLUSTER_DMAX, 65))["nclusters"] == 1


@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("case", FC.within_cases(), ids=lambda c: c[0])
def test_within_decided_probes_exact(ctx, fix, case, kind):
    _, wrec = fix
    key, name, d, n, m = case
    w = FC.within_inputs(name, d, n, m, kind)
    gap, bound = R.within_reference(w["ctrs"], w["axes_inv"], w["x"], kind, wrec[(key, kind)])
    counts, bits = ctx.friends_within(w["ctrs"], kind, w["axes_inv"], w["x"], want_bits=True)
    share, on_ring = R.check_within(counts, bits, gap, bound, w["ring"], f"{key}/{kind}",
                                    free_ring=1e-9 if name == "late" else 0.0)
    c2, _ = ctx.friends_within(w["ctrs"], kind, w["axes_inv"], w["x"])  # the route without bit rows
    np.testing.assert_array_equal(c2, counts)
    print(f"friends_hp within {key}/{kind}: undecided share {share:.3g}, undecided on the 1e-9 ring {on_ring}, "
          f"decision distance max {bound.max():.3g}")
    assert share <= 0.02


DRAW_SHAPES = [(1, 65), (3, 1), (33, 65), (64, 65)]  # (d, centres): what tests/golden/friends.npz lacks


@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("d,n", DRAW_SHAPES)
def test_draws_stream_exact(ctx, d, n, kind):
    from dynesty_amd import _lib
    w = FC.within_inputs("iso", d, n, 1, kind)
    fr = F.Friends(kind, w["axes"] @ w["axes"], None, w["axes"], w["axes_inv"], 0.0, w["ctrs"])
    for return_q, seed in ((False, 13), (True, 14)):
        rs = np.random.default_rng(seed)
        xs, qs, state = ctx.friends_draw(_lib.pcg_state6(rs.bit_generator), 12, w["ctrs"], kind, w["axes"],
                                         w["axes_inv"], return_q=return_q)
        ref = [F.friends_sample(fr, rs, return_q=True) if return_q else (F.friends_sample(fr, rs), None)
               for _ in range(12)]
        np.testing.assert_allclose(xs, np.array([x for x, _ in ref]), rtol=0, atol=1e-13)
        np.testing.assert_array_equal(state, _lib.pcg_state6(rs.bit_generator))
        gap, bound = R.within_reference(w["ctrs"], w["axes_inv"], xs, kind)
        assert np.all(np.min(gap - bound, axis=1) <= 0), "a returned point lies in no shape"
        if return_q:
            np.testing.assert_array_equal(qs, [q for _, q in ref])
            decided = np.all(np.abs(gap) > bound, axis=1)
            np.testing.assert_array_equal(qs[decided], (gap <= 0).sum(axis=1)[decided])
            assert decided.sum() >= 10


@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("d,n", [(1, 65), (3, 1)])
def test_unif_friends_batch_stream_exact(ctx, d, n, kind):
    from dynesty_amd import problems
    from oracle_backend import OracleBackend
    prob = problems.gauss_iid(d, 10.0, f"I{d}")
    w = FC.within_inputs("iso", d, n, 1, kind)
    _, ll = ctx.problem_eval(prob, w["ctrs"])
    loglstar = float(np.min(ll)) - 2.0
    states = ctx.seed_children(np.array([5, 6, 7, 8]), 0, 12)
    dev = ctx.unif_friends_batch(prob, loglstar, states, w["ctrs"], kind, w["axes"], w["axes_inv"])
    ref = OracleBackend().unif_friends_batch(prob, loglstar, states, w["ctrs"], kind, w["axes"], w["axes_inv"])
    np.testing.assert_array_equal(dev["ncalls"], ref["ncalls"])
    np.testing.assert_array_equal(dev["rng_out"], ref["rng_out"])
    np.testing.assert_allclose(dev["u"], ref["u"], rtol=0, atol=1e-13)
    gap, bound = R.within_reference(w["ctrs"], w["axes_inv"], dev["u"], kind)
    assert np.all(np.min(gap - bound, axis=1) <= 0)


def test_unif_friends_batch_refuses_above_32(ctx):
    """dh_unif_friends_batch is built for ndim <= 32 (the register forms of walk2.hip): d = 33 and 64 are a clean
    DH_ERR_ARG, so the stream-exact draws at those d are dh_friends_draw's (above)."""
    from dynesty_amd import _lib, problems
    for d in (33, 64):
        w = FC.within_inputs("iso", d, 65, 1, "balls")
        with pytest.raises(_lib.DynHipError, match="not built"):
            ctx.unif_friends_batch(problems.gauss_iid(d, 10.0, f"I{d}"), -1e30, ctx.seed_children(np.array([5, 6, 7, 8]), 0, 4),
                                   w["ctrs"], "balls", w["axes"], w["axes_inv"])


def test_report_worst():
    """Not a check of its own: the worst error / bound per entry point and kind of this session."""
    for (entry, kind), r in sorted(WORST.items()):
        R.report(r, f"WORST {entry} {kind}")
        assert all(v <= 1.0 for v in r.values())
