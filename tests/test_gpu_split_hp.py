"""The split tree of MultiEllipsoid.update on the device (k_root, k_split / node_kmeans_part, k_ell, k_tree, k_finish,
k_out_eig in csrc/rebuild.hip; the host recursion of csrc/wide.hip) held to the high-precision reference of
tests/split_hp_ref.py on the cases of tests/split_cases.py: nells and nnodes exact, the leaf of every point exact and
in the reference's list order, every leaf ellipsoid inside the derived bounds of tests/ell_hp_ref.py against its own
leaf's record, every point inside the union by more than its quadratic form's bound -- through the single call, the
batched call grouped by shape, and the ragged call with every case padded beside neighbours of other sizes.  Then
dh_bootstrap_expand: masks exact, boot_expand_kernel's own chain, and the factor end to end.

No mpmath and no oracle tree runs here: the reference's side is tests/golden/split_hp.npz (tools/make_golden.py
split_hp) and long-double residuals.  tests/test_split_hp_cpu.py shows, without a device, that every decision of every
case is decidable and that the float64 oracle passes the same checker.
"""
import math

import numpy as np
import pytest

import ell_hp_ref as H
import split_cases as SC
import split_hp_ref as S

pytestmark = pytest.mark.gpu

ALL_D = [d for g in SC.GROUPS for d in g]
NARROW_D = [d for d in ALL_D if d <= 44]  # the ragged batch is a narrow-D launch; above, rebuild_many loops over rebuild
KEYS = ("ctrs", "covs", "ams", "axes", "axlens", "logvol_ells")


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.fixture(scope="module")
def fix():
    return S.load_fixture()


@pytest.fixture(scope="module")
def single(ctx):
    """ctx.rebuild of every case, once."""
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = ctx.rebuild(SC.points(key), multi=True, want_labels=True)
        return cache[key]
    return get


def _cases_of(d):
    return [c for c in SC.CASES if c[2] == d]


def _finish(failures, worst, what):
    print(f"split_hp WORST {what}: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not failures, f"{what}: {len(failures)} case(s) fail: {failures[:6]}"


@pytest.mark.parametrize("d", ALL_D)
def test_rebuild(single, fix, d):
    failures, worst = [], H.Ratios()
    for key, _, _, n, _ in _cases_of(d):
        got = single(key)
        try:
            r = S.check_tree(SC.points(key), got, fix[0][key], key, logvol_from_spectrum=d > 44)
        except AssertionError as e:
            print(f"split_hp {key}: {e}")
            failures.append((key, str(e)))
            continue
        print(f"split_hp {key}: nells {got['nells']} nnodes {got['nnodes']}  "
              + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
        worst.merge(r)
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        if bad:
            failures.append((key, bad))
    _finish(failures, worst, f"rebuild D={d}")


def _same_bits(res, one, what):
    assert res["nells"] == one["nells"], what
    for k in KEYS:
        np.testing.assert_array_equal(res[k], one[k], err_msg=f"{what} {k}")


@pytest.mark.parametrize("d", NARROW_D)
def test_rebuild_many_by_shape(ctx, single, d):
    """The cases of one (n, d) in one batched launch: bit for bit the single calls, which test_rebuild holds to the
    reference."""
    shapes = {}
    for key, _, _, n, _ in _cases_of(d):
        shapes.setdefault(n, []).append(key)
    for n, keys in shapes.items():
        for key, res in zip(keys, ctx.rebuild_many([SC.points(k) for k in keys])):
            _same_bits(res, single(key), f"{key} in a batch of {len(keys)}")
    print(f"split_hp WORST rebuild_many D={d}: equal to the single calls in {len(shapes)} shape(s)")


@pytest.mark.parametrize("d", NARROW_D)
def test_rebuild_ragged(ctx, single, d):
    """Every case of one d in one ragged launch, each the first n rows of a block padded to the length of a longer
    neighbour (a uniform cloud nobody checks): bit for bit the single calls."""
    keys = [c[0] for c in _cases_of(d)]
    longest = max(c[3] for c in _cases_of(d))
    filler = np.random.default_rng(d).uniform(0.1, 0.9, (longest + 7, d))
    sets = [SC.points(k) for k in keys]
    res = ctx.rebuild_many(sets[:1] + [filler] + sets[1:])
    for key, r in zip(keys, res[:1] + res[2:]):
        _same_bits(r, single(key), f"{key} in the ragged batch")
    print(f"split_hp WORST rebuild ragged D={d}: equal to the single calls in {len(keys)} case(s)")


# ---- bootstrap expansion ----
def test_bootstrap_expand(ctx, fix):
    worst = H.Ratios()
    failures = []
    for key, fam, d, n, multi in SC.BOOT_CASES:
        fx = fix[1][key]
        pts = S.boot_points(key)
        ent = SC.boot_entropy(key)
        expand, n_in = ctx.bootstrap_expand(pts, ent, SC.BOOT_B, multi, want_n_in=True)
        expand = float(expand[0])
        # masks: NumPy's Generator.integers on the replica streams, with the two repairs
        masks = S.boot_masks(n, ent, SC.BOOT_B)
        np.testing.assert_array_equal(n_in[0], [m.sum() for m in masks], err_msg=key)
        np.testing.assert_array_equal(n_in[0], fx["nin"], err_msg=key)
        # the kernel alone: the replicas' ellipsoids from the ragged call (the launch dh_bootstrap_expand makes:
        # rebuild_launch_full with n_arr), then the long-double form with those centres and precision matrices
        res = ctx.rebuild_many([pts[m] for m in masks], multi=multi)
        vals = [S.expand2_with_own_ellipsoids(pts[~m], r["ctrs"], r["ams"]) for m, r in zip(masks, res)]
        np.testing.assert_array_equal([r["nells"] for r in res], fx["nells"], err_msg=key)
        val = float(max(v for v, _ in vals))
        vb = max(b for _, b in vals)
        own = max(1.0, math.sqrt(val))
        r = H.Ratios()
        r.add("kernel_only", abs(expand - own), vb / (2 * math.sqrt(val)) + 2 * H.EPS * own if val > 1 else 0.0)
        # end to end: the reference tree of the in-sample points, then distances (the fixture)
        q2, q2b = float(np.max(fx["q2"])), float(np.max(fx["q2b"]))
        want = max(1.0, math.sqrt(q2))
        r.add("end_to_end", abs(expand - want), q2b / (2 * math.sqrt(q2)) + 2 * H.EPS * want if q2 > 1 else 0.0)
        if q2 < 1:
            assert expand == 1.0, key
        print(f"split_hp {key}: expand {expand!r}  " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()))
        worst.merge(r)
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        if bad:
            failures.append((key, bad))
    _finish(failures, worst, "bootstrap_expand")
