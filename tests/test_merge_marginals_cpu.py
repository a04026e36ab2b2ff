"""Marginals of a merged run without a device: the three exports are declared, exported and bound; MergedRun's
quantile / histogram / histogram2d / corner_data are the reference's and NumPy's; the exact quantile function of
tests/marginals_hp_ref.py holds the reference's own values at its budget, and an integer-weight restatement of the
device's method at the device's."""
import ctypes
import os

import numpy as np
import pytest

import marginals_hp_ref as mq
from test_abi import header_functions

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEW = {"dh_merged_quantile": 6, "dh_merged_hist1d": 7, "dh_merged_hist2d": 9}


def test_new_symbols_declared_exported_and_bound():
    from dynesty_amd import _lib
    fns = header_functions()
    lib = ctypes.CDLL(_lib.lib_path())
    for name, nargs in NEW.items():
        assert name in fns and len(fns[name]) == nargs, name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.dh_version() == 100
    for name in ("quantile", "histogram", "histogram2d", "corner_data"):
        assert hasattr(_lib.DeviceMergedRun, name), name


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "merge.npz")), np.load(os.path.join(GOLD, "merge_marginals.npz"))


@pytest.fixture(scope="module")
def merged(gold):
    """The golden merged run as a MergedRun: the reference's own fields."""
    from dynesty_amd import ensemble
    g, _ = gold
    m = ensemble.MergedRun(niter=int(g["ref/niter"]))
    for k in ("logwt", "logz", "samples"):
        m[k] = g["ref/" + k]
    return m


def test_quantile_equals_the_reference(gold, merged):
    g, gm = gold
    # the same operations on the same numbers: the run has no ties, so the stable order is the reference's
    np.testing.assert_array_equal(merged.importance_weights(), g["ref/importance_weights"])
    got = merged.quantile(gm["q"])
    assert got.shape == (3, 9)
    np.testing.assert_array_equal(got, gm["quantile"])
    np.testing.assert_array_equal(merged.quantile(gm["q"], columns=[2, 0]), gm["quantile"][[2, 0]])
    np.testing.assert_array_equal(got[:, 0], merged.samples.min(axis=0))
    np.testing.assert_array_equal(got[:, -1], merged.samples.max(axis=0))
    assert merged.quantile(0.5, columns=1).shape == (1, 1)


def test_exact_quantile_function_holds_the_reference_values(gold):
    g, gm = gold
    x, w = g["ref/samples"], g["ref/importance_weights"]
    ratio, err, eps = mq.worst(x, w, range(3), gm["q"], gm["quantile"], "reference")
    print(f"[marginals golden] reference quantiles: worst backward error / budget = {ratio:.3g} ({err:.3g} / {eps:.3g})")
    assert ratio <= 1
    # the helper tells a wrong answer from a right one: the neighbouring point in the order is many budgets away
    col = mq.Column(x[:, 0], w)
    k = int(np.searchsorted(col.xs, gm["quantile"][0, 4]))
    assert col.backward_error(0.5, col.xs[k + 2]) > 1e3 * col.eps_reference()
    assert col.backward_error(0.5, col.xs[0] - 1.0) == np.inf
    assert col.backward_error(0.0, col.xs[0]) == 0 and col.backward_error(1.0, col.xs[-1]) == 0


def integer_weight_quantile(x, w, q):
    """The device's method with a sort in place of the selection."""
    W = [int(v) for v in np.rint(np.asarray(w, dtype=np.longdouble) * np.longdouble(2.0 ** 62)).astype(np.uint64)]
    order = np.argsort(x, kind="stable")
    xs = x[order]
    C = np.cumsum([0] + [W[i] for i in order[:-1]], dtype=object)
    norm = int(C[-1])
    out = []
    for qq in q:
        t = float(qq) * float(norm)
        if qq == 0:
            out.append(xs[0])
        elif qq == 1 or t >= float(norm):
            out.append(xs[-1])
        else:
            ti = int(t)
            k = int(np.searchsorted(np.array(C, dtype=object), ti, side="right")) - 1
            frac = (float(ti - int(C[k])) + (t - float(ti))) / float(W[order[k]])
            out.append(xs[k] + frac * (xs[k + 1] - xs[k]))
    return np.array(out)


def test_integer_weight_restatement_within_the_device_budget(gold):
    g, gm = gold
    x, w = g["ref/samples"], g["ref/importance_weights"]
    got = np.array([integer_weight_quantile(x[:, c], w, gm["q"]) for c in range(3)])
    ratio, err, eps = mq.worst(x, w, range(3), gm["q"], got, "device")
    print(f"[marginals golden] integer weights: worst backward error / budget = {ratio:.3g} ({err:.3g} / {eps:.3g})")
    assert ratio <= 1
    np.testing.assert_array_equal(got[:, 0], x.min(axis=0))
    np.testing.assert_array_equal(got[:, -1], x.max(axis=0))


def test_histograms_equal_numpy(merged):
    x, w = merged.samples, merged.importance_weights()
    h, e = merged.histogram(bins=20)
    assert h.shape == (3, 20) and e.shape == (3, 21)
    counts = merged.histogram(bins=20, weighted=False)[0]
    for c in range(3):
        want, edges = np.histogram(x[:, c], bins=20, weights=w)
        np.testing.assert_array_equal(e[c], edges)
        np.testing.assert_array_equal(h[c], want)
        np.testing.assert_array_equal(counts[c], np.histogram(x[:, c], bins=20)[0])
        np.testing.assert_array_equal(merged.histogram(columns=[c], bins=edges)[0][0],
                                      np.histogram(x[:, c], bins=edges, weights=w)[0])
    h, e = merged.histogram(columns=[1], bins=7, range=(-1., 2.), weighted=False)
    np.testing.assert_array_equal(h[0], np.histogram(x[:, 1], bins=7, range=(-1., 2.))[0])
    H, xe, ye = merged.histogram2d([(0, 2), (1, 1)], bins=(6, 9), range=((-1., 1.), (0., 3.)))
    assert H.shape == (2, 6, 9)
    for k, (i, j) in enumerate([(0, 2), (1, 1)]):
        np.testing.assert_array_equal(H[k], np.histogram2d(x[:, i], x[:, j], bins=(6, 9), range=((-1., 1.), (0., 3.)),
                                                           weights=w)[0])
    ex, ey = np.linspace(-2, 2, 8), np.linspace(-1, 3, 5)  # explicit edges, a set for all pairs or one per pair
    H, xe, ye = merged.histogram2d([(0, 2), (1, 0)], bins=(ex, np.array([ey, ey + 0.5])))
    assert H.shape == (2, 7, 4) and xe.shape == (2, 8)
    np.testing.assert_array_equal(H[1], np.histogram2d(x[:, 1], x[:, 0], bins=(ex, ey + 0.5), weights=w)[0])
    H, xe, ye = merged.histogram2d((0, 1), bins=5)
    np.testing.assert_array_equal(H[0], np.histogram2d(x[:, 0], x[:, 1], bins=5, weights=w)[0])


def test_corner_data_equals_its_parts(merged):
    cd = merged.corner_data(span=0.95, bins=12)
    sp = merged.quantile([0.5 - 0.5 * 0.95, 0.5 + 0.5 * 0.95])
    np.testing.assert_array_equal(cd["span"], sp)
    np.testing.assert_array_equal(cd["hist"], merged.histogram(bins=12, range=sp)[0])
    np.testing.assert_array_equal(cd["pairs"], [(0, 1), (0, 2), (1, 2)])
    H = merged.histogram2d(cd["pairs"], bins=12, range=[(sp[i], sp[j]) for i, j in cd["pairs"]])[0]
    np.testing.assert_array_equal(cd["hist2d"], H)
    assert cd["hist2d"].shape == (3, 12, 12)


@pytest.mark.parametrize("q", [-0.1, 1.1, np.nan, [0.5, 2.0]])
def test_bad_quantiles_raise(merged, q):
    with pytest.raises(ValueError):
        merged.quantile(q)


def test_bad_columns_and_edges_raise(merged):
    with pytest.raises(ValueError):
        merged.quantile(0.5, columns=[3])
    with pytest.raises(ValueError):
        merged.quantile(0.5, columns=[-1])
    with pytest.raises(ValueError):
        merged.histogram(columns=[3])
    with pytest.raises(ValueError):
        merged.histogram2d([(0, 3)])
    with pytest.raises(ValueError):
        merged.histogram(bins=[0., 2., 1.])
