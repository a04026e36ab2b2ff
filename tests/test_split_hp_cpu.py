"""tests/split_hp_ref.py without a device: the reference tree is reproducible, every decision of every case is
decidable, the set of cases sees what it is meant to see, and the float64 oracle passes the very checker the device
goes through (tests/test_gpu_split_hp.py).

  * the fixture tests/golden/split_hp.npz is what the generator produces now (the cases with d <= 3), and the
    long-double form of the reference (no mpmath) takes the same decisions on EVERY case;
  * margin / bound > 1 for every label of every iteration, every accept test and every axis sign of every node;
  * the coverage conditions: a split decided by the second disjunct alone, a rejected parent over an accepted split, a
    node still moving at the tenth iteration, children of exactly 2 d - 1 (rejected) and 2 d (tried) points, deep
    trees, multi-part nodes in every group of dimensions, an order check with at least three leaves;
  * every wrong rule of split_hp_ref.PERTURBATIONS changes the leaves, their order or nnodes of at least one case;
  * oracle.bounding_ref.multi_update (NumPy / LAPACK / SciPy's kmeans2), its axis signs normalised, gives the same
    leaves in the same order, the same node count, and leaf ellipsoids inside every bound;
  * bootstrap expansion: the oracle's factors are inside the end-to-end bound and the kernel-only bound.
"""
import math
import os

import numpy as np
import pytest

import ell_hp_ref as H
import split_cases as SC
import split_hp_ref as S
from oracle import bounding_ref as B


@pytest.fixture(scope="module")
def fix():
    return S.load_fixture()


@pytest.fixture()
def canonical_oracle(monkeypatch):
    """The oracle with the device's sign convention and LAPACK's divide-and-conquer driver (see
    tests/test_ell_hp_cpu.py: the MRRR default is not what the eigen bounds speak of)."""
    import types
    from scipy import linalg as sla
    shim = types.SimpleNamespace(eigh=lambda a, **kw: sla.eigh(a, driver="evd", **kw), LinAlgError=sla.LinAlgError,
                                 norm=sla.norm)
    monkeypatch.setattr(B, "sla", shim)
    monkeypatch.setattr(B, "CANON_SIGNS", True)


def test_fixture_is_data_only_and_small(fix):
    g = np.load(S.FIXTURE)
    assert all(g[k].dtype.kind in "fi" for k in g.files)
    gold = os.path.dirname(S.FIXTURE)
    assert os.path.getsize(S.FIXTURE) <= os.path.getsize(os.path.join(gold, "ell_hp.npz"))
    assert 40 <= len(SC.KEYS) <= 60 and len(set(SC.KEYS)) == len(SC.KEYS)
    built = sum(int(fix[0][k]["head"][1]) for k in SC.KEYS)
    print(f"split_hp: {len(SC.KEYS)} cases, {built} high-precision node ellipsoids")
    assert built <= 2200


def test_fixture_is_what_the_generator_produces(fix):
    n = 0
    for key, _, d, _, _ in SC.CASES:
        if d > 3:
            continue
        now, then = S.case_record(key), fix[0][key]
        assert sorted(now) == sorted(then), key
        for name in now:
            if now[name].dtype.kind == "f" and name.startswith("node_"):
                # margins and ratios pass through libm's log / exp in long double: equal to rounding, not to the bit
                np.testing.assert_allclose(now[name], then[name], rtol=1e-9, err_msg=f"{key}/{name}")
            else:
                np.testing.assert_array_equal(now[name], then[name], err_msg=f"{key}/{name}")
        n += 1
    print(f"split_hp fixture: {n} cases regenerated and equal")
    assert n >= 10


def test_long_double_form_takes_the_same_decisions(fix):
    """The reference once more without mpmath (LDL^T pivots, Gaussian solves): the same leaves in the same order, the
    same nnodes, the same verdict at every node -- on every case, the wide ones included."""
    for key, _, d, n, _ in SC.CASES:
        fx = fix[0][key]
        tree = S.split_tree_ref(SC.points(key), "ld")
        lab = np.full(n, -1)
        for i, ix in enumerate(tree["leaves"]):
            lab[ix] = i
        np.testing.assert_array_equal(lab, fx["labels"], err_msg=key)
        assert tree["nnodes"] == fx["head"][1] and tree["depth"] == fx["head"][2], key
        np.testing.assert_array_equal([nd["code"] for nd in tree["nodes"]], fx["node_code"], err_msg=key)
        np.testing.assert_array_equal([nd["n0"] for nd in tree["nodes"]], fx["node_n0"], err_msg=key)
        np.testing.assert_allclose([nd["accept_margin"] for nd in tree["nodes"]], fx["node_accept_margin"], rtol=1e-6,
                                   atol=1e-12, err_msg=key)


def test_every_decision_is_decidable(fix):
    """margin / bound > 1 at every node of every case; no case is exempt from any part of any check."""
    worst = {}
    for key, fam, d, _, _ in SC.CASES:
        fx = fix[0][key]
        for name in ("label", "accept", "order"):
            r = fx[f"node_{name}_ratio"]
            assert np.all(r > 1), f"{key}: a {name} decision is within its bound (margin / bound = {r.min():.3g})"
            if len(r):
                worst[(fam, name)] = min(worst.get((fam, name), math.inf), float(r.min()))
    for fam in SC.FAMILIES:
        print(f"split_hp DECIDABILITY {fam}: " + "  ".join(f"{name} {worst.get((fam, name), math.inf):.3g}"
                                                            for name in ("label", "accept", "order")))
    assert min(worst.values()) > 1e3


def test_statistics_and_coverage(fix):
    stats = {}
    for key, fam, d, n, _ in SC.CASES:
        st = S.statistics(fix[0][key], d)
        stats[key] = st
        print(f"split_hp STATS {key}: nells {st['nells']} nnodes {st['nnodes']} depth {st['depth']} k-means {st['kmeans']} "
              f"first {st['first']} second {st['second']} rejected {st['rejected']} ({st['accdesc']}) too-small "
              f"{st['too_small']} moving {st['moving']} empty {st['empty']} label margin {st['label_margin']:.2g} "
              f"accept margin {st['accept_margin']:.2g}")
    fams = {fam for _, fam, _, _, _ in SC.CASES}
    assert fams == set(SC.FAMILIES)
    dims = {d for _, _, d, _, _ in SC.CASES}
    assert dims == {d for g in SC.GROUPS for d in g}
    for g, d in ((0, 5), (1, 17), (2, 45)):  # the split threshold from both sides in every group
        assert {n for _, _, dd, n, _ in SC.CASES if dd == d} >= {4 * d - 1, 4 * d, 4 * d + 1}
        assert stats[f"blobs/{d}/{4 * d - 1}"]["kmeans"] == 0 and stats[f"blobs/{d}/{4 * d}"]["kmeans"] == 1
    # a case decided by the second disjunct alone
    assert any(st["second"] > 0 for st in stats.values())
    # a rejected parent with an accepted descendant
    assert any(st["accdesc"] > 0 for st in stats.values())
    # a node still moving at the tenth iteration; several in one case of the overlapping or broad families
    assert any(st["moving"] > 0 for st in stats.values())
    assert max(st["moving"] for st in stats.values()) >= 3
    # a child of exactly 2 d - 1 points, rejected; one of exactly 2 d, tried
    for key, fam, d, n, k in SC.CASES:
        if fam != "side" or d == 3:  # (at d = 3 the root's k-means cuts the main blob instead: deep trees, kept for those)
            continue
        fx = fix[0][key]
        small = np.minimum(fx["node_n0"], fx["node_m"] - fx["node_n0"])
        if k == 2 * d - 1:
            assert small[0] == k and fx["node_code"][0] == S.TOO_SMALL and stats[key]["nnodes"] == 1, key
        else:
            assert small[0] == k and fx["node_code"][0] != S.TOO_SMALL, key
    assert any(k == 2 * d for _, fam, d, _, k in SC.CASES if fam == "side" and d > 3)
    # trees at least 6 levels deep at d <= 3
    assert sum(stats[k]["depth"] >= 6 for k, _, d, _, _ in SC.CASES if d <= 3) >= 3
    # a multi-part node in every group that has parts; more than one level of the host recursion in the wide group
    for g in (0, 1):
        assert any(stats[k]["multipart"] > 0 for k, _, d, _, _ in SC.CASES if SC.group_of(d) == g)
        assert any(stats[k]["nells"] > 1 for k, _, d, _, _ in SC.CASES if SC.group_of(d) == g)
    for d in SC.GROUPS[2]:
        assert any(np.any(fix[0][k]["node_depth"] >= 1) for k, _, dd, _, _ in SC.CASES if dd == d)
        assert any(stats[k]["nells"] > 1 for k, _, dd, _, _ in SC.CASES if dd == d) or d == 45
    assert any(stats[k]["nells"] > 1 for k, _, d, _, _ in SC.CASES if SC.group_of(d) == 2)
    # the order check is live: at least three leaves (every node's sign is decidable: test_every_decision_is_decidable)
    assert sum(st["nells"] >= 3 for st in stats.values()) >= 4
    # everything rejected in the uniform box: one ellipsoid out of many nodes
    assert all(stats[k]["nells"] == 1 for k, fam, _, _, _ in SC.CASES if fam == "box")
    assert stats["box/25/1100"]["nnodes"] >= 25
    # no empty cluster: k = 2 Lloyd from seeds symmetric about the mean cannot produce one
    assert all(st["empty"] == 0 for st in stats.values())


def test_every_wrong_rule_is_visible():
    """Each perturbed rule changes the leaves, their order or nnodes of at least one case (cheapest cases first; the
    search stops at the first).  Two rules are invisible, and are asserted to be: '<=' for '<' differs only at an
    exact tie d1 == d0 in long double, and no case has one (the smallest label margin is far above zero); ddof = 1 in
    the root's scale is a common factor on every coordinate, to which no label of any cloud can react."""
    order = sorted(SC.CASES, key=lambda c: c[2]**2 * c[3])
    base = {}

    def sig(key, rules):
        pts = SC.points(key)
        return S.signature(S.split_tree_ref(pts, "ld", rules), len(pts))

    for name, rules in S.PERTURBATIONS.items():
        seen = None
        for key, _, d, n, _ in order:
            if key not in base:
                base[key] = sig(key, S.RULES)
            if sig(key, rules) != base[key]:
                seen = key
                break
        print(f"split_hp PERTURBATION {name}: " + (f"visible in {seen}" if seen else "invisible in every case"))
        if name == "<= in the label comparison":
            assert seen is None, "an exact tie exists: state it in DESIGN.md 3.3.1"
        elif name == "scale with ddof = 1":
            # invisible to ANY cloud, not for want of a case: ddof = 1 multiplies the root's scale by sqrt(n / (n - 1))
            # in EVERY coordinate alike, d0 and d1 of every point by (n - 1) / n, and a label is the sign of d1 - d0.
            # (It would show only together with "scale from the node", where the factor differs between nodes -- and
            # still not between coordinates.)
            assert seen is None, "a common factor on every coordinate changed a label: the reference is wrong"
        else:
            assert seen is not None, f"no case sees the wrong rule '{name}': add one"


def _oracle_tree(pts, fx):
    """oracle.bounding_ref.multi_update as the dict the checker takes.  The oracle returns ellipsoids, not index sets:
    a leaf's centre is np.mean of its points in their original order, so each returned centre is looked up, bit for
    bit, among the means of the reference's leaves."""
    n, d = pts.shape
    trace = []
    mell = B.multi_update(pts, trace=trace)
    nnodes = 1 + 2 * sum(min(np.bincount(t["labels"], minlength=2)) >= 2 * d for t in trace)
    means = [np.mean(pts[fx["labels"] == i], axis=0) for i in range(int(fx["head"][0]))]
    lab = np.full(n, -1, dtype=np.int64)
    for i, e in enumerate(mell.ells):
        hit = [j for j, m in enumerate(means) if np.array_equal(m, e.ctr)]
        if len(hit) == 1:
            lab[fx["labels"] == hit[0]] = i
    return dict(nells=mell.nells, nnodes=nnodes, labels=lab, ctrs=mell.ctrs, covs=mell.covs, ams=mell.ams,
                axes=np.array([e.axes for e in mell.ells]), axlens=np.array([e.axlens for e in mell.ells]),
                logvol_ells=mell.logvol_ells)


def test_float64_oracle_passes_the_checker(fix, canonical_oracle):
    worst = {}
    failures = []
    for key, _, d, n, _ in SC.CASES:
        pts = SC.points(key)
        fx = fix[0][key]
        r = S.check_tree(pts, _oracle_tree(pts, fx), fx, key, canonical=False)
        w = worst.setdefault(SC.group_of(d), H.Ratios())
        w.merge(r)
        bad = {k: v for k, v in r.items() if not v <= 1.0}
        if bad:
            failures.append((key, bad))
    for g, w in sorted(worst.items()):
        print(f"split_hp ORACLE WORST d in {SC.GROUPS[g]}: " + "  ".join(f"{k} {v:.3g}" for k, v in w.items()))
    assert not failures, f"the float64 oracle is outside a bound in {len(failures)} case(s): {failures[:6]}"


def test_checker_rejects_a_swapped_order_and_a_wrong_count(fix, canonical_oracle):
    key = "ring/3/513"
    pts, fx = SC.points(key), fix[0][key]
    got = _oracle_tree(pts, fx)
    wrong = dict(got, nnodes=got["nnodes"] + 2)
    with pytest.raises(AssertionError, match="nnodes"):
        S.check_tree(pts, wrong, fx, key, canonical=False)
    perm = np.arange(got["nells"])
    perm[[0, 1]] = [1, 0]
    swapped = dict(got, labels=perm[got["labels"]])
    with pytest.raises(AssertionError, match="ORDER only"):
        S.check_tree(pts, swapped, fx, key, canonical=False)
    # a leaf ellipsoid grown by 1e-9: the scale check sees it
    grown = dict(got, covs=got["covs"] * (1 + 1e-9), ams=got["ams"] / (1 + 1e-9))
    r = S.check_tree(pts, grown, fx, key, canonical=False)
    assert max(r.values()) > 1.0


# ---- bootstrap expansion ----
def test_bootstrap_cases_and_oracle(fix):
    from oracle import nested_ref as N
    above, exact_one = 0, 0
    worst = H.Ratios()
    for key, fam, d, n, multi in SC.BOOT_CASES:
        fx = fix[1][key]
        pts = S.boot_points(key)
        ent = SC.boot_entropy(key)
        masks = S.boot_masks(n, ent, SC.BOOT_B)
        np.testing.assert_array_equal([m.sum() for m in masks], fx["nin"], err_msg=key)
        assert np.all(fx["decid"] > 1), key
        i = int(np.argmax(fx["q2"]))
        q2, q2b = float(fx["q2"][i]), float(np.max(fx["q2b"]))
        assert abs(q2 - 1) > 10 * q2b, f"{key}: the expansion is within its bound of 1"
        want = max(1.0, math.sqrt(q2))
        bound = q2b / (2 * math.sqrt(q2)) + 2 * H.EPS * want if q2 > 1 else 0.0
        above += q2 > 1 and want - 1 > 10 * bound
        exact_one += q2 < 1
        # the oracle, end to end
        got = N.boot_expand(pts, ent, SC.BOOT_B, multi)
        worst.add("end_to_end", abs(got - want), bound)
        if q2 < 1:
            assert got == 1.0, key
        # ... and its own chain alone: the long-double form with the oracle's own ellipsoids
        vals = []
        for b, sel in enumerate(masks):
            pin, pout = pts[sel], pts[~sel]
            ell = B.bounding_ellipsoid(pin)
            ells = B.split_tree(pin, ell) if multi else [ell]
            assert len(ells) == fx["nells"][b], key
            vals.append(S.expand2_with_own_ellipsoids(pout, [e.ctr for e in ells], [e.am for e in ells]))
        val, vb = max(vals, key=lambda t: t[0])
        vb = max(t[1] for t in vals)
        own = max(1.0, math.sqrt(float(val)))
        worst.add("kernel_only", abs(got - own), vb / (2 * math.sqrt(float(val))) + 2 * H.EPS * own if val > 1 else 0.0)
        print(f"split_hp BOOT {key}: n_in {fx['nin']} expand {want:.6f} bound {bound:.2g} oracle error {abs(got - want):.2g}")
    print("split_hp BOOT ORACLE WORST: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert above >= len(SC.BOOT_CASES) / 2 and exact_one >= 1
    assert {d for _, _, d, _, _ in SC.BOOT_CASES} == {2, 5, 14, 25}
    assert all(130 <= n <= 300 for _, _, _, n, _ in SC.BOOT_CASES)
