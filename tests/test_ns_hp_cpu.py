"""The run loop's evidence integration against a high-precision reference, the part that needs no device
(tests/ns_hp_ref.py, tests/ns_cases.py; the device's share: tests/test_gpu_ns_hp.py):

  * the long-double reference equals the mpmath golden file (tests/golden/ns_hp.npz) to long-double rounding
  * the oracle's float64 recurrence (oracle/nested_ref.consume_queue) is inside the bounds on every case: the bounds
    are not tighter than the reference itself (its worst error / bound per family is printed)
  * degraded restatements are outside them: the float64 scan form with its plateau correction unguarded (a non-finite
    var ln Z on every `floor` case), ln dX off by 1e-13, the constant step taken through a plateau
  * every `stop` case leaves the stopping index no choice: |dz - dlogz| exceeds dz's bound at every death
"""
import functools
import math
import os

import numpy as np
import pytest

import ns_cases as C
import ns_hp_ref as H

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ns_hp.npz")
KEYS = C.all_keys()
LD = H.LD


@functools.lru_cache(maxsize=None)
def evaluated(key, r, dlogz=None):
    case = C.build(key, dlogz)
    ch = C.chain_inputs(case, r)
    hp = H.integrate_hp(ch["dead"], ch["steps"], ch["state0"])
    b = {o: H.consume_bounds(hp, ch["dead"], ch["steps"], ch["state0"], ch["ends"], case.K, case.nlive, order=o,
                             plateau_pl=ch["pl"]) for o in ("device", "serial")}
    return case, ch, hp, b


@pytest.fixture(scope="module")
def golden():
    return np.load(G)


@pytest.mark.parametrize("key", KEYS)
def test_long_double_reference_equals_the_golden_file(golden, key):
    """np.longdouble carries 11 bits more than float64 and runs the recurrence in the serial order: its distance from
    the 50-digit values is held to 2^-11 of the serial order's float64 bound."""
    case = C.build(key)
    for r in range(case.runs):
        _, ch, hp, b = evaluated(key, r)
        ends = golden[f"{key}/r{r}/ends"]
        assert list(ends) == sorted(set(int(e) for e in ch["ends"] if e > 0))
        mp = H.join(golden[f"{key}/r{r}/state"])
        for q, name in enumerate(H.QUANT):
            err = np.asarray(hp[name][ends - 1] - mp[:, q], dtype=np.float64)
            rt = H.ratio(err, b["serial"][name][ends - 1] * 2.0 ** -11)
            assert rt.max() <= 1.0, (key, r, name, rt)


_worst = {}


@pytest.mark.parametrize("key", KEYS)
def test_the_oracle_is_inside_the_bounds(key):
    case = C.build(key)
    for r in range(case.runs):
        _, ch, hp, b = evaluated(key, r)
        recs = [x for x in case.ref[r] if x is not None]
        got = np.array([[x["state"].logvol, x["state"].logz, x["state"].h, x["state"].logzvar] for x in recs])
        ref, bd = H.fill_rows(hp, b["serial"], ch["ends"], ch["state0"])
        rt = H.ratio(np.asarray(got.astype(LD) - ref, dtype=np.float64), bd).max(axis=0)
        w = _worst.setdefault(case.family, np.zeros(5))
        w[:4] = np.maximum(w[:4], rt)
        for f, x in enumerate(recs):  # the plateau a fill leaves open
            s = x["state"]
            if s.plateau_mode:
                e = int(ch["ends"][f])
                j, lv_start = H.open_plateau(hp, ch["pl"], e, ch["state0"], s.plateau_logdvol)
                pl = H.plogdvol_hp(lv_start, case.nlive)
                bl = b["serial"]["logvol"][e - 1] if e else 0.0
                rp = float(H.ratio(float(LD(s.plateau_logdvol) - pl), H.plogdvol_bound(bl, j, case.nlive, float(pl))))
                w[4] = max(w[4], rp)
                assert rp <= 1.0, (key, r, f, rp)
        print(f"{key} run {r}: oracle error / bound (serial order) " + " ".join(f"{n} {x:.3g}" for n, x in zip(H.QUANT, rt)))
        assert rt.max() <= 1.0, (key, r, rt)


def test_the_oracles_worst_ratios_per_family():
    """(printed for DESIGN.md; runs after the cases above)"""
    for fam, w in sorted(_worst.items()):
        print(f"oracle worst error / bound, {fam}: " + " ".join(f"{n} {x:.3g}" for n, x in zip(H.QUANT + ("plateau_logdvol",), w)))
    assert all(w.max() <= 1.0 for w in _worst.values())


FLOOR = [k for k in KEYS if C.family(k) == "floor"]


@pytest.mark.parametrize("key", FLOOR)
def test_unguarded_scan_form_loses_var_on_the_floor_cases(key):
    """The float64 scan form of ns_consume's phase B -- weights summed relative to the fill's M, plateau deaths patched
    in through H_e = e^{lnZ_E - lnZ_e}(...) - lnZ_e -- gives a non-finite var ln Z as soon as a plateau lies more than
    745 below the values of the same fill (inf * 0 + inf); ln Z and H do not notice.  With such a fill's variance taken
    from the recurrence (csrc/ns.hip: kNsUnder) it is inside the bounds."""
    case = C.build(key)
    for r in range(case.runs):
        _, ch, hp, b = evaluated(key, r)
        ends = [int(e) for e in ch["ends"] if e > 0]
        ref, bd = H.fill_rows(hp, b["serial"], ends, ch["state0"])
        for guard in (False, True):
            got = H.scan_form_f64(ch["dead"], ch["steps"], ch["pl"], ends, ch["state0"], case.nlive, guard=guard)
            rt = H.ratio(np.asarray(got.astype(LD) - ref, dtype=np.float64), bd).max(axis=0)
            assert rt[1] <= 1.0 and rt[2] <= 1.0, (key, r, guard, rt)
            if guard:
                assert rt.max() <= 1.0, (key, r, rt)
            else:
                assert not np.isfinite(got[-1, 3]) and rt[3] > 1.0, (key, r, got[:, 3])


@pytest.mark.parametrize("key", ["base/50x17", "base/50x257", "base/4x5", "base/5x64"])
def test_ln_dx_off_by_1e_13_is_outside_the_bounds(key):
    """(Against the bounds the device is held to, where |ln Z| u is well below 1e-13: at |ln Z| = 800 an error of
    1e-13 is rounding.)"""
    case = C.build(key)
    for r in range(case.runs):
        _, ch, hp, b = evaluated(key, r)
        got = H.recurrence_f64(ch["dead"], ch["steps"], ch["state0"], ldv_err=1e-13)
        e = int(ch["ends"][0]) - 1  # the end of the first fill
        ok = H.recurrence_f64(ch["dead"], ch["steps"], ch["state0"])
        for o in ("device",):
            assert float(H.ratio(float(LD(got[e, 1]) - hp["logz"][e]), b[o]["logz"][e])) > 1.0, (key, r, o)
            assert float(H.ratio(float(LD(ok[e, 1]) - hp["logz"][e]), b[o]["logz"][e])) <= 1.0, (key, r, o)


@pytest.mark.parametrize("key", [k for k in KEYS if C.family(k) in ("floor", "ties")])
def test_constant_step_through_a_plateau_is_outside_the_bounds(key):
    case = C.build(key)
    for r in range(case.runs):
        _, ch, hp, b = evaluated(key, r)
        if not np.isfinite(ch["pl"]).any():
            continue
        dlv = math.log((case.nlive + 1.0) / case.nlive)
        got = H.recurrence_f64(ch["dead"], np.full(len(ch["dead"]), dlv), ch["state0"])
        rt = H.ratio(np.asarray(LD(got[-1, 0]) - hp["logvol"][-1], dtype=np.float64), b["serial"]["logvol"][-1])
        assert rt > 1.0, (key, r, rt)


@pytest.mark.parametrize("key", [k for k in KEYS if C.family(k) in ("range", "floor")])
def test_range_and_floor_shapes_do_what_they_are_for(key):
    """range: the whole initial set dies in the first fill and spans more than 745.  floor: the floor points are a
    plateau; where K allows it ends inside a fill that goes on to the top values, elsewhere it is carried."""
    case = C.build(key)
    for r in range(case.runs):
        rec = case.ref[r][0]
        if case.family == "range":
            assert (rec["dead_src"] >= 0).all() and len(rec["dead_logl"]) >= case.nlive
            assert np.ptp(rec["dead_logl"]) > 745
        else:
            assert np.isfinite(rec["dead_pl"][0])
    if key in ("floor-10000/50x257", "floor-800/50x257", "floor-1e+30/50x257"):
        rec = case.ref[0][0]
        assert not rec["state"].plateau_mode and rec["dead_logl"][-1] > -10 and rec["dead_logl"][0] < -745
    if key in ("floor-800/50x17", "floor-10000/9000x700"):
        assert case.ref[0][0]["state"].plateau_mode and case.ref[0][0]["state"].plateau_counter > 0


@pytest.mark.parametrize("key", [k for k in KEYS if C.family(k) == "stop"])
def test_stop_cases_leave_the_stopping_index_no_choice(golden, key):
    case = C.build(key)
    free = C.build(key, C.NEVER)  # the same chain, never stopped
    nstop = 0
    for r in range(case.runs):
        recs = [x for x in case.ref[r] if x is not None]
        n0 = len(recs[0]["dead_logl"])
        if not (len(recs) == 2 and recs[1]["stopped"]):
            continue
        nstop += 1
        ndead = n0 + len(recs[1]["dead_logl"])
        assert 0 < len(recs[1]["dead_logl"]) < len(free.ref[r][1]["dead_logl"])  # inside the second fill
        assert int(golden[f"{key}/r{r}/ndead"]) == ndead and bool(golden[f"{key}/r{r}/stopped"])
        _, ch, hp, b = evaluated(key, r, C.NEVER)
        lmax = C.chain_lmax(free, r)
        n1 = n0 + len(free.ref[r][1]["dead_logl"])
        dz = np.array([float(H._lae(LD(0), LD(lmax[k]) + hp["logvol"][k] - hp["logz"][k])) for k in range(n1)])
        bd = np.array([H.dz_bound(b["device"], k, lmax[k], float(hp["logvol"][k]), float(hp["logz"][k])) for k in range(n1)])
        assert (np.abs(dz - case.dlogz) > bd).all(), (key, r, np.min(np.abs(dz - case.dlogz) / bd))
        # the rule is tested with the state a death leaves behind: the first death after which dz < dlogz is the last
        assert int(np.flatnonzero(dz < case.dlogz)[0]) + 1 == ndead
    assert nstop > 0
