"""Marginals of the device's merged run (csrc/merge_marginals.hip: dh_merged_quantile, dh_merged_hist1d, dh_merged_hist2d).

Quantiles are held to the exact quantile function of tests/marginals_hp_ref.py by their backward error in q, at the
budget derived there (the weight quantisation M 2^-63 / Norm plus 8 roundings); q = 0 and q = 1 are the column's
minimum and maximum exactly.  Histogram counts are NumPy's exactly (membership); weighted bins within
n_b (2^-63 + 2^-53 H_b) + 2^-53 H_b of NumPy's (n_b points of quantised weight, NumPy's own n_b additions, one rounding
of the integer sum).  Every call is made twice and must return the same bits.

Worst measured error / budget per case is recorded in DESIGN.md section 3.8.1."""
import os

import numpy as np
import pytest

import inputs
import marginals_hp_ref as mq
import merge_cases
from test_gpu_merge import golden_args, problem_for

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Q16 = [0, 1e-4, 0.001, 0.01, 0.025, 0.1, 0.16, 0.3, 0.5, 0.7, 0.84, 0.9, 0.975, 0.99, 0.999, 1]
CASES = merge_cases.cases()


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "merge.npz")), np.load(os.path.join(GOLD, "merge_marginals.npz"))


class Run:
    """A merged run on the device with its samples and weights downloaded once."""

    def __init__(self, c, prob, args):
        self.d = c.merge_runs(prob, **args)
        self.x = self.d.field("samples")
        self.w = self.d.importance_weights()


@pytest.fixture(scope="module")
def gold_run(gold):
    from dynesty_amd import _lib
    return Run(_lib.Context(0), inputs.problem("C1"), golden_args(gold[0]))


@pytest.fixture(scope="module")
def large_run():
    from dynesty_amd import _lib
    return Run(_lib.Context(0), problem_for(7), CASES["e_large"])


@pytest.fixture(scope="module")
def wide_run():
    from dynesty_amd import _lib
    return Run(_lib.Context(0), problem_for(40), CASES["f_wide"])


def twice(fn):
    a, b = fn(), fn()
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert u.tobytes() == v.tobytes()
    return a


def check_quantiles(run, q, label, columns=None):
    cols = list(range(run.x.shape[1])) if columns is None else list(columns)
    got = twice(lambda: run.d.quantile(q, columns))
    assert got.shape == (len(cols), len(q))
    ratio, err, eps = mq.worst(run.x, run.w, cols, q, got, "device")
    print(f"[marginals {label}] quantiles: worst backward error / budget = {ratio:.3g} ({err:.3g} / {eps:.3g})")
    assert ratio <= 1, (label, ratio, err, eps)
    for j, qq in enumerate(q):
        if qq == 0:
            np.testing.assert_array_equal(got[:, j], run.x[:, cols].min(axis=0))
        if qq == 1:
            np.testing.assert_array_equal(got[:, j], run.x[:, cols].max(axis=0))
    return got


def test_golden_quantiles(gold, gold_run):
    g, gm = gold
    got = check_quantiles(gold_run, gm["q"], "golden")
    # the device's answers to the reference's own problem (its samples and weights), at the reference's budget
    ratio, err, eps = mq.worst(g["ref/samples"], g["ref/importance_weights"], range(3), gm["q"], got, "reference")
    print(f"[marginals golden] against the reference's run: worst backward error / budget = {ratio:.3g} ({err:.3g} / {eps:.3g}); "
          f"largest difference from its values {np.max(np.abs(got - gm['quantile'])):.3g}")
    assert ratio <= 1
    sub = gold_run.d.quantile(gm["q"], columns=[2, 0])
    np.testing.assert_array_equal(sub, got[[2, 0]])


def test_large_sixteen_quantiles(large_run):
    assert large_run.d.niter == 13943
    check_quantiles(large_run, Q16, "e_large")


def test_wide_column_tiling(wide_run):
    check_quantiles(wide_run, [0, 0.025, 0.16, 0.5, 0.84, 0.975, 1], "f_wide")
    check_quantiles(wide_run, [0.16, 0.5, 0.84], "f_wide one tile")  # 40 columns side by side: the plain LDS atomics
    check_quantiles(wide_run, [0.5], "f_wide one q", columns=[39, 0, 17, 17])


def test_span_of_2000_nats(ctx):
    run = Run(ctx, problem_for(3), CASES["g_span"])
    W = np.rint(run.w.astype(np.longdouble) * np.longdouble(2.0 ** 62))
    assert (W == 0).mean() > 0.5  # most weights quantise to zero
    check_quantiles(run, [0, 0.001, 0.5, 0.999, 1], "g_span")
    # the host's methods give the same ends (np.interp alone returns the last of the zero-weight points at q = 0)
    host = run.d.to_merged_run()
    np.testing.assert_array_equal(host.quantile([0, 1]), run.d.quantile([0, 1]))
    np.testing.assert_array_equal(host.quantile([0, 1]), np.stack([run.x.min(axis=0), run.x.max(axis=0)], axis=1))


def tie_case(at_max):
    """Column 1 constant over 300 consecutive dead points of run 1: a tie group larger than a wavefront, spread over
    more than one workgroup's rows of the merged run; at_max: the constant is the column's maximum, so that Norm
    (which leaves out the LAST point of the stable order) depends on the order inside the group."""
    args = merge_cases.make(np.random.default_rng(11), [700, 900, 650], 50, 3)
    for u in args["dead_u"] + [args["live_u"]]:
        u[..., 1] *= 0.98
    args["dead_u"][1][400:700, 1] = 0.99 if at_max else 0.5
    return args


@pytest.mark.parametrize("name", ["a_copy", "tie300", "tie300_max"])
def test_ties(ctx, name):
    args = CASES["a_copy"] if name == "a_copy" else tie_case(name == "tie300_max")
    run = Run(ctx, problem_for(3), args)
    if name != "a_copy":
        vals, cnt = np.unique(run.x[:, 1], return_counts=True)
        k = np.flatnonzero(run.x[:, 1] == vals[cnt.argmax()])
        assert len(k) == 300 and k[-1] // 256 > k[0] // 256
        assert (run.x[k[0], 1] == run.x[:, 1].max()) == (name == "tie300_max")
    else:
        assert len(np.unique(run.x[:, 0])) < run.d.niter
    # quantiles spread so that some fall inside the tie group (its share of the weight is what it is: all are checked)
    check_quantiles(run, list(np.linspace(0, 1, 16)), name)


def bin_index(x, edges):
    """NumPy's membership: edges[i] <= x < edges[i + 1], the last bin closed; -1 outside."""
    i = np.searchsorted(edges, x, side="right") - 1
    i[x == edges[-1]] = len(edges) - 2
    i[(x < edges[0]) | (x > edges[-1])] = -1
    return i


def weighted_bound(n_b, H_b):
    return n_b * (2.0 ** -63 + 2.0 ** -53 * H_b) + 2.0 ** -53 * H_b


def test_histogram_counts_are_numpys(large_run):
    r = large_run
    D = r.x.shape[1]
    h, e = twice(lambda: r.d.histogram(bins=37, weighted=False))
    assert h.shape == (D, 37) and e.shape == (D, 38)
    for c in range(D):
        want, edges = np.histogram(r.x[:, c], bins=37)
        np.testing.assert_array_equal(e[c], edges)
        np.testing.assert_array_equal(h[c], want)
    h, _ = twice(lambda: r.d.histogram(columns=[4, 1], bins=50, range=(-0.7, 1.3), weighted=False))
    for i, c in enumerate([4, 1]):
        np.testing.assert_array_equal(h[i], np.histogram(r.x[:, c], bins=50, range=(-0.7, 1.3))[0])
    # edges ON sample values, the column minimum first and the maximum last: every edge has a point on it
    for c in (0, 6):
        xs = np.sort(r.x[:, c])
        edges = np.unique(np.concatenate([[xs[0]], xs[np.arange(100, len(xs) - 1, 977)], [xs[-1]]]))
        h, _ = twice(lambda: r.d.histogram(columns=[c], bins=edges, weighted=False))
        want = np.histogram(r.x[:, c], bins=edges)[0]
        np.testing.assert_array_equal(h[0], want)
        assert h[0].sum() == len(xs) and want[0] >= 1 and want[-1] >= 2
        np.testing.assert_array_equal(h[0], np.bincount(bin_index(r.x[:, c], edges), minlength=len(edges) - 1))


def test_histogram_weights_within_the_bound(large_run):
    r = large_run
    for c in (0, 3):
        # edges planted on the 40 heaviest points of the column: a point on the wrong side of its edge would move its
        # whole weight, at least 100 bounds of the bin
        heavy = np.argsort(r.w, kind="stable")[-40:]
        edges = np.unique(r.x[heavy, c])
        assert len(edges) == 40
        h, _ = twice(lambda: r.d.histogram(columns=[c], bins=edges))
        idx = bin_index(r.x[:, c], edges)
        ok = idx >= 0
        n_b = np.bincount(idx[ok], minlength=39)
        want = np.bincount(idx[ok], weights=r.w[ok], minlength=39)
        bound = weighted_bound(n_b, want)
        for p in heavy:
            assert r.w[p] >= 100 * bound[idx[p]], (p, r.w[p], bound[idx[p]])
        err = np.abs(h[0] - want)
        print(f"[marginals e_large] histogram column {c}: worst error / bound = {np.max(err / bound):.3g}")
        assert (err <= bound).all()
        np.testing.assert_array_equal(twice(lambda: r.d.histogram(columns=[c], bins=edges, weighted=False))[0][0], n_b)
    h, e = twice(lambda: r.d.histogram(bins=50))
    for c in range(r.x.shape[1]):
        want = np.histogram(r.x[:, c], bins=50, weights=r.w)[0]
        n_b = np.histogram(r.x[:, c], bins=50)[0]
        assert (np.abs(h[c] - want) <= weighted_bound(n_b, want)).all()


def test_histogram2d(wide_run):
    r = wide_run
    pairs = [(0, 39), (17, 3), (5, 5)]
    H, xe, ye = twice(lambda: r.d.histogram2d(pairs, bins=(9, 14), weighted=False))
    assert H.shape == (3, 9, 14)
    for k, (i, j) in enumerate(pairs):
        want, wx, wy = np.histogram2d(r.x[:, i], r.x[:, j], bins=(9, 14))
        np.testing.assert_array_equal(xe[k], wx)
        np.testing.assert_array_equal(ye[k], wy)
        np.testing.assert_array_equal(H[k], want)
    rng = ((-0.5, 0.75), (-1.0, 0.25))
    H, xe, ye = twice(lambda: r.d.histogram2d(pairs, bins=21, range=rng, weighted=False))
    Hw = twice(lambda: r.d.histogram2d(pairs, bins=21, range=rng))[0]
    for k, (i, j) in enumerate(pairs):
        n_b = np.histogram2d(r.x[:, i], r.x[:, j], bins=21, range=rng)[0]
        np.testing.assert_array_equal(H[k], n_b)
        want = np.histogram2d(r.x[:, i], r.x[:, j], bins=21, range=rng, weights=r.w)[0]
        assert (np.abs(Hw[k] - want) <= weighted_bound(n_b, want)).all()
    # edges on sample values, minimum first and maximum last, per pair
    def on_values(c, step):
        xs = np.sort(r.x[:, c])
        return np.unique(np.concatenate([[xs[0]], xs[5:-1:step], [xs[-1]]]))
    exs = [on_values(i, 131) for i, _ in pairs]
    eys = [on_values(j, 97) for _, j in pairs]
    assert len({len(e) for e in exs}) == 1 and len({len(e) for e in eys}) == 1
    H = twice(lambda: r.d.histogram2d(pairs, bins=(np.array(exs), np.array(eys)), weighted=False))[0]
    for k, (i, j) in enumerate(pairs):
        np.testing.assert_array_equal(H[k], np.histogram2d(r.x[:, i], r.x[:, j], bins=(exs[k], eys[k]))[0])
        assert H[k].sum() == r.d.niter


def test_corner_data_equals_its_parts(gold_run):
    d = gold_run.d
    cd = d.corner_data(bins=16)
    sp = d.quantile([0.5 - 0.5 * 0.999999426697, 0.5 + 0.5 * 0.999999426697])
    np.testing.assert_array_equal(cd["span"], sp)
    np.testing.assert_array_equal(cd["hist"], d.histogram(bins=16, range=sp)[0])
    np.testing.assert_array_equal(cd["pairs"], [(0, 1), (0, 2), (1, 2)])
    H = d.histogram2d(cd["pairs"], bins=16, range=[(sp[i], sp[j]) for i, j in cd["pairs"]])[0]
    np.testing.assert_array_equal(cd["hist2d"], H)
    assert H.shape == (3, 16, 16) and abs(cd["hist"].sum(axis=1) - 1).max() < 1e-5
    assert d.corner_data(bins=16)["hist2d"].tobytes() == cd["hist2d"].tobytes()


def test_kept_path_agrees_with_the_host_methods(ctx):
    """The smallest shape of tests/test_gpu_merge_kept.py, merged where it ran."""
    from dynesty_amd import backend, ensemble
    prob = inputs.problem("C1")
    backend.set_backend(ctx)
    try:
        d = ensemble.run_ensemble_merged(prob, 4, merge='device', nlive=100, queue_size=16, entropy=[5, 9], walks=23,
                                         bound="single", dlogz=0.1)
    finally:
        backend.set_backend(None)
    host = d.to_merged_run()
    x, w_dev, w_host = host.samples, d.importance_weights(), host.importance_weights()
    q = [0, 0.025, 0.16, 0.5, 0.84, 0.975, 1]
    got_d, got_h = twice(lambda: d.quantile(q)), host.quantile(q)
    rd = mq.worst(x, w_dev, range(3), q, got_d, "device")
    rh = mq.worst(x, w_host, range(3), q, got_h, "reference")
    print(f"[marginals kept] device quantiles: worst backward error / budget = {rd[0]:.3g}; host's: {rh[0]:.3g}; "
          f"largest difference {np.max(np.abs(got_d - got_h)):.3g}")
    assert rd[0] <= 1 and rh[0] <= 1
    np.testing.assert_array_equal(got_d[:, [0, -1]], got_h[:, [0, -1]])
    sp = got_h[:, [1, 5]]
    (hd, ed), (hh, eh) = twice(lambda: d.histogram(bins=30, range=sp)), host.histogram(bins=30, range=sp)
    np.testing.assert_array_equal(ed, eh)
    np.testing.assert_array_equal(d.histogram(bins=30, range=sp, weighted=False)[0], host.histogram(bins=30, range=sp, weighted=False)[0])
    for c in range(3):
        idx = bin_index(x[:, c], ed[c])
        ok = idx >= 0
        n_b = np.bincount(idx[ok], minlength=30)
        # the two sides sum different weights (the host recomputes its own from logwt): that difference, bin by bin,
        # comes on top of the bound
        moved = np.bincount(idx[ok], weights=np.abs(w_dev - w_host)[ok], minlength=30)
        assert (np.abs(hd[c] - hh[c]) <= weighted_bound(n_b, hh[c]) + moved).all()
        want = np.histogram(x[:, c], bins=30, range=tuple(sp[c]), weights=w_dev)[0]
        assert (np.abs(hd[c] - want) <= weighted_bound(n_b, want)).all()
    d.release()


def test_errors_leave_the_run_in_place(ctx, gold):
    d = ctx.merge_runs(inputs.problem("C1"), **golden_args(gold[0]))
    summary = dict(d.summary)
    mean, cov = d.mean_and_cov()
    good = np.linspace(-1, 1, 5)

    def intact():
        assert d.summary == summary
        m2, c2 = d.mean_and_cov()
        np.testing.assert_array_equal(m2, mean)
        np.testing.assert_array_equal(c2, cov)
    calls = [lambda: d.quantile(-0.1), lambda: d.quantile(1.1), lambda: d.quantile(np.nan),
             lambda: d.quantile(np.linspace(0, 1, 17)), lambda: d.quantile(0.5, columns=[3]),
             lambda: d.histogram(columns=[3]), lambda: d.histogram(columns=[-1], bins=good),
             lambda: d.histogram(bins=[0., 2., 1.]), lambda: d.histogram(bins=[0., np.inf]),
             lambda: d.histogram(bins=4097, range=(0., 1.)),
             lambda: d.histogram2d([(0, 3)], bins=(good, good)), lambda: d.histogram2d([(0, 1)], bins=(good, good[::-1])),
             lambda: d.histogram2d([(0, 1)], bins=(128, 129), range=((0., 1.), (0., 1.)))]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} did not raise")
        intact()
    assert d.quantile(np.linspace(0, 1, 16)).shape == (3, 16)
    assert d.histogram2d([(0, 1)], bins=128, range=((0., 1.), (0., 1.)))[0].shape == (1, 128, 128)
    d.release()
    for call in (lambda: d.quantile(0.5), lambda: d.histogram(bins=good), lambda: d.histogram2d([(0, 1)], bins=(good, good))):
        with pytest.raises(ValueError):
            call()
    for fn, args in ((ctx.lib.dh_merged_quantile, (1, good.ctypes.data, 3, None, good.ctypes.data)),
                     (ctx.lib.dh_merged_hist1d, (3, None, 1, good.ctypes.data, 1, good.ctypes.data))):
        with pytest.raises(ValueError):  # nothing on the device any more
            ctx._check_merge(fn(ctx.handle, *args))
