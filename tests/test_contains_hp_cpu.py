"""Without a device: the membership tests' reference, bound and inputs (tests/contains_hp_ref.py, tests/contains_cases.py)
hold for the float64 NumPy oracle, the shells are what they claim to be, and the checkers reject wrong kernels -- NumPy
restatements of the membership kernels with one defect each.  The staging layout of dh_contains_runs is held with the
other layouts in tests/test_stage_plan_cpu.py (a stand-alone program under the address and undefined-behaviour sanitizers).
"""
import os
import re

import numpy as np
import pytest

import contains_cases as C
import contains_hp_ref as H
from oracle import bounding_ref as B



def dim_list():
    """DH_DIM_LIST as csrc/ctx.h defines it: the padded dimensions the narrow kernels are instantiated for."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "dynesty_amd", "csrc", "ctx.h")).read()
    line = re.search(r"^#define DH_DIM_LIST\(X\)(.*)$", src, flags=re.M).group(1)
    return tuple(int(n) for n in re.findall(r"X\((\d+)\)", line))


DIM_LIST = dim_list()


def oracle_quad(c):
    return np.array([B.multi_quadforms(p, c["ctrs"], c["ams"]) for p in c["x"]])


# ---- NumPy restatements of the kernels, with optional defects --------------------------------------------------------
def np_quad(x, ctrs, ams, dtype=np.float64, drop_last=False):
    """q (k, m) by rows, then the fold, in `dtype`; drop_last: the last column and row are left out (a padded
    instantiation that stops one short when d == N)."""
    x, ctrs, ams = (np.asarray(a, dtype=np.float64) for a in (x, ctrs, ams))
    n = x.shape[1] - (1 if drop_last else 0)
    out = np.empty((x.shape[0], ctrs.shape[0]))
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(ctrs.shape[0]):
            dl = (x - ctrs[a]).astype(dtype)[:, :n]
            out[:, a] = np.sum(dl * (dl @ ams[a].astype(dtype)[:n, :n].T), axis=1, dtype=dtype)
    return out


def np_inside(quad, mode, swap=False):
    with np.errstate(invalid="ignore"):
        if mode == 0:
            return quad <= 1 if swap else quad < 1
        return np.sqrt(quad) < 1 if swap else np.sqrt(quad) <= 1


def np_runs(c, all_slots=False, highest=False, serve_masked=False):
    """flag, first of a run-wise case from the float64 restatement."""
    R, wpr = len(c["flag"]), c["wpr"]
    flag, first = c["flag"].copy(), c["first"].copy()
    x = c["x"].reshape(R, wpr, -1)
    for r in range(R):
        if not (c["served"][r] or serve_masked):
            continue
        m = c["max_ells"] if all_slots else c["nells_eff"][r]
        ins = np_inside(np_quad(x[r], c["ctrs"][r, :m], c["ams"][r, :m]), 0 if c["strict"] else 1).any(axis=1)
        out = np.flatnonzero(~ins)
        if len(out):
            flag[r] |= 1
            first[r] = min(first[r], out[-1] if highest else out[0])
    return flag, first


# ---- the oracle keeps the bound; the shells are what they claim --------------------------------------------------------
@pytest.mark.parametrize("family,d", C.CONTAINS_NARROW + C.CONTAINS_WIDE)
def test_oracle_keeps_the_bound_and_shells_are_placed(family, d):
    c = C.case(family, d)
    q, bound, shell = c["q"], c["bound"], c["shell"]
    worst = max(H.check_quad(oracle_quad(c), q, bound), H.check_quad(np_quad(c["x"], c["ctrs"], c["ams"]), q, bound))
    dec = H.decidable(q, bound)
    # the decidable shells and the bulk: every pair of theirs, with every ellipsoid, is decidable -- nothing is exempt
    rows = np.isin(shell, C.DECIDABLE_SHELLS + C.BULK + ("ladder", "nan"))
    assert dec[rows].all(), f"{c['name']}: {int((~dec[rows]).sum())} pair(s) of the decidable shells are not decidable"
    # the +-B/8 shell: its own pairs lie within their bound, its pairs with other ellipsoids are decidable
    rows_u, cols_u = C.own_pairs(c, C.UNDECIDABLE_SHELLS)
    assert np.all(np.abs(q[rows_u, cols_u] - 1) <= bound[rows_u, cols_u])
    undecided = ~dec
    undecided[rows_u, cols_u] = False
    assert not undecided.any()
    if family != "late" and (family, d) != ("kappa", 1):  # (there the float64 grid has no point that near)
        assert len(rows_u) >= 2
    for s in C.DECIDABLE_SHELLS:
        r, a = C.own_pairs(c, (s,))
        assert len(r) and np.all((q[r, a] > 1) == (s[0] == "+")), s
    # both verdicts, in both modes, among the decidable pairs; every count from 0 to m in the multi cases
    for mode in (0, 1):
        v = H.hp_inside(q, mode)[dec]
        assert v.any() and not v.all()
        H.check_verdicts(np_inside(oracle_quad(c), mode) | ~dec, q, bound, mode)  # (undecided pairs: any answer passes)
    m = c["ctrs"].shape[0]
    if m > 1:
        ok = dec.all(axis=1)
        assert set(H.hp_inside(q, 0)[ok].sum(axis=1)) == set(range(m + 1))
    assert np.isnan(q[-1]).all() and shell[-1] == "nan"
    print(f"contains_hp cpu {c['name']}: k {len(shell)}  oracle error / bound {worst:.3g}  "
          f"largest bound {float(np.nanmax(bound)):.3g}")


@pytest.mark.parametrize("d", C.NARROW_D + C.WIDE_D)
def test_exact_cases_are_exact_in_any_order(d):
    e = C.exact_case(d)
    dl = e["x"] - e["ctrs"][0]
    am = e["ams"][0]
    fwd = np.array([sum(dl[p, i] * sum(am[i, j] * dl[p, j] for j in range(d)) for i in range(d)) for p in range(3)])
    rev = np.array([sum(dl[p, i] * sum(am[i, j] * dl[p, j] for j in reversed(range(d))) for i in reversed(range(d)))
                    for p in range(3)])
    ein = np.einsum("pi,ij,pj->p", dl, am, dl)
    for got in (fwd, rev, ein):
        assert got[0] == 1.0 and got[1] < 1.0 < got[2]
        np.testing.assert_array_equal(got, e["q"][:, 0].astype(np.float64))
    assert np.all(e["q"][:, 0].astype(np.float64).astype(H.LD) == e["q"][:, 0])  # the reference's values are float64s
    # one ulp outside is still outside after a correctly rounded square root
    assert np.sqrt(fwd[2]) > 1.0 and np.sqrt(fwd[1]) < 1.0 and np.sqrt(fwd[0]) == 1.0
    assert np.all(e["bound"] == 0)
    for mode in (0, 1):
        H.check_quad(fwd[:, None], e["q"], e["bound"])
        H.check_verdicts(np_inside(fwd[:, None], mode), e["q"], e["bound"], mode)


RUNS_CPU = [(1, 5), (5, 5), (5, 83), (13, 256), (32, 64), (33, 5), (65, 8)]


@pytest.mark.parametrize("d,wpr", RUNS_CPU)
@pytest.mark.parametrize("single", (False, True))
def test_run_cases_hold_what_they_claim(d, wpr, single):
    c = C.runs_case(d, wpr, single, d <= 32)
    st = c["states"]
    assert list(np.flatnonzero(st[0] == 1)) == [wpr - 1] and not (st[0] == 0).any()  # only the last entry is outside
    out1 = np.flatnonzero(st[1] == 1)
    assert out1[0] == 0 and (wpr == 1 or len(out1) == 2)  # the first and a later one
    assert np.all(st[2] == -1)  # entirely inside
    for r in (3, 4):
        assert not c["served"][r] and (st[r] == 1).any()  # masked, with entries outside
    und5 = np.flatnonzero(st[5] == 0)
    if d > 32 or single:
        assert list(np.flatnonzero(st[5] == 1)) == [wpr // 2]
    else:  # nothing of run 5 is decidably outside: its flag is the kernel's own verdict on the +-B/8 entries
        assert not (st[5] == 1).any()
    if d <= 32:  # undecided entries from entry 0 on: first depends on them (single: ahead of the +8B entry)
        assert len(und5) >= 2 and und5[0] == 0 and (wpr // 2 == 0 or und5[0] < wpr // 2)
        x5, m5 = c["x"].reshape(7, wpr, d)[5], c["nells_eff"][5]
        own = np.abs(c["q"][5][und5, :m5] - 1) <= c["bound"][5][und5, :m5]
        assert np.all(own.sum(axis=1) == 1)  # one undecidable pair each, decidably outside the run's other ellipsoids
    assert list(np.flatnonzero(st[6] == 1)) == [wpr // 3] and np.isnan(c["x"].reshape(7, wpr, d)[6, wpr // 3]).any()
    if d > 32:
        assert not (st == 0).any()  # the wide cases carry no undecided entry: nothing is exempt
    else:
        assert (st[[1, 5]] == 0).any() or wpr <= 2
    # the unused slots hold an ellipsoid that contains everything
    for r in range(7):
        assert not c["ams"][r, c["nells_eff"][r]:].any()
    # the float64 restatement passes the check; the reference determines the words of every served run but run 5 of
    # the narrow cases, whose words the undecided entries decide (5 served runs)
    flag, first = np_runs(c)
    share = 1.0 if d > 32 else 0.8
    assert H.check_runs(flag, first, c["flag"], c["first"], st, c["served"]) == share
    assert H.check_runs(flag, None, c["flag"], None, st, c["served"]) == (share if not single else 1.0)
    if d <= 32:  # there a kernel that calls every undecided entry inside, or every one outside, passes; its words differ
        words = []
        for verdict in (True, False):
            want = H.runs_from_inside((st == -1) | ((st == 0) & verdict), c["served"], c["flag"], c["first"])
            H.check_runs(want[0], want[1], c["flag"], c["first"], st, c["served"])
            words.append(want)
        assert words[0][1][5] != words[1][1][5] and (single or words[0][0][5] != words[1][0][5])
        ins5 = np.flatnonzero(st[5] == -1)
        if len(ins5):  # one whose first points at an entry that is inside does not pass
            bad = np.array(words[1][1])
            bad[5] = ins5[0]
            with pytest.raises(AssertionError):
                H.check_runs(words[1][0], bad, c["flag"], c["first"], st, c["served"])
    # and agrees with the words that follow from the entries' verdicts alone
    want = H.runs_from_inside(st == -1, c["served"], c["flag"], c["first"])
    if not (st[c["served"]] == 0).any():
        np.testing.assert_array_equal(flag, want[0])
        np.testing.assert_array_equal(first, want[1])


# ---- the checkers catch wrong kernels ------------------------------------------------------------------------------
def test_mutant_float32_accumulation_fails():
    for family, d in (("round", 5), ("kappa", 25), ("round", 200)):
        c = C.case(family, d)
        with pytest.raises(AssertionError):
            H.check_quad(np_quad(c["x"], c["ctrs"], c["ams"], dtype=np.float32), c["q"], c["bound"])


@pytest.mark.parametrize("d", DIM_LIST)
def test_mutant_last_column_dropped_fails(d):
    for c in (C.case("round", d), C.exact_case(d)):
        with pytest.raises(AssertionError):
            H.check_quad(np_quad(c["x"], c["ctrs"], c["ams"], drop_last=True), c["q"], c["bound"])


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("d", (1, 2, 3, 5, 25, 200))
def test_mutant_swapped_comparison_fails(d, mode):
    """`<=` for `<` in mode 0, `<` for `<=` in mode 1: only a point with q == 1 tells them apart."""
    e = C.exact_case(d)
    quad = np_quad(e["x"], e["ctrs"], e["ams"])
    H.check_verdicts(np_inside(quad, mode), e["q"], e["bound"], mode)
    with pytest.raises(AssertionError):
        H.check_verdicts(np_inside(quad, mode, swap=True), e["q"], e["bound"], mode)


@pytest.mark.parametrize("d,wpr", RUNS_CPU)
@pytest.mark.parametrize("defect", ("all_slots", "highest", "serve_masked"))
def test_mutant_run_wise_defects_fail(d, wpr, defect):
    """All max_ells slots read instead of nells[run]; first = the highest outside index; a masked run served."""
    c = C.runs_case(d, wpr, False, d <= 32)
    flag, first = np_runs(c, **{defect: True})
    with pytest.raises(AssertionError):
        H.check_runs(flag, first, c["flag"], c["first"], c["states"], c["served"])


def test_unpack_reports_the_bits_beyond_k():
    mask = np.array([[0b101, 0], [1 << 63, 1 << 5]], dtype=np.uint64)
    inside, beyond = H.unpack(mask, 66)
    assert inside.shape == (66, 2) and inside[0, 0] and inside[2, 0] and inside[63, 1] and inside.sum() == 3
    assert beyond[1].sum() == 1 and beyond[0].sum() == 0
