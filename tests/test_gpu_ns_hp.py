"""ln Z, H and var ln Z of the device-resident run loop (csrc/ns.hip: ns_consume phase B, ns_finish) held to a
long-double restatement of the reference's recurrence with derived bounds (tests/ns_hp_ref.py) at the value scales
tests/test_gpu_ns_consume.py does not reach (tests/ns_cases.py): offsets of +-800 and +-1e6, live sets that span more
than 745, penalty floors down to -1e30 under a likelihood of order 1, ties at +-1e6, fills late in a run
(ln X = -5000), and the stopping rule firing inside a fill.  Which point dies where is the oracle's and exact.
Every case prints error / bound per quantity; a ratio above 1 fails.  No tolerance is set by hand."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ns_cases as C
import ns_hp_device as D
import ns_hp_ref as H
from oracle import nested_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LD = H.LD


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


@pytest.mark.parametrize("key", C.all_keys())
def test_consume_chain_is_inside_the_bounds(ctx, key):
    worst = D.run_case(ctx, key)
    print(D.report(key, worst))
    assert max(worst[n] for n in D.NAMES) <= 1.0, D.report(key, worst)
    if key in ("floor-800/50x17", "floor-10000/9000x700", "floor-1e+30/40000x300"):
        assert worst["plateaus_carried"] > 0  # K < the floor's multiplicity: the plateau crosses fills


def test_compact_and_full_path_integrate_the_same_values(ctx):
    """ns_consume_compact works on the K + 1 smallest live points.  nlive = 9000 has no other route, nlive = 5000 has
    both: K = 700 selects, K = 1300 (the same 700 entries and 600 stale ones behind them) holds the whole set in LDS.
    The same deaths, and each route inside its own bounds of the same reference."""
    for key in ("base/5000x700", "ties40-1e6/5000x700", "floor-10000/5000x700"):
        for pad in (None, 1300):
            worst = D.run_case(ctx, key, pad_to=pad)
            print(("full path    " if pad else "compact path ") + D.report(key, worst))
            assert max(worst[n] for n in D.NAMES) <= 1.0, (key, pad, worst)


SERIAL_KEYS = ["base/50x257", "floor-10000/50x257", "ties40+1e6/50x257", "offset+1e+06/300x600", "range/300x600",
               "ties40-1e6/300x600", "ties400+1e6/300x2048", "stop/300x600", "floor-10000/9000x700"]


def test_serial_walk_integrates_the_same():
    """DH_NS_SERIAL=1 (a fresh process: the switch is read from the environment) takes every fill through the serial
    walk: the walk changes, the deaths and the integration must not."""
    env = dict(os.environ, DH_NS_SERIAL="1")
    out = subprocess.run([sys.executable, os.path.join(HERE, "ns_hp_device.py")] + SERIAL_KEYS, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    for key in SERIAL_KEYS:
        print("DH_NS_SERIAL=1 " + D.report(key, res[key]))
        assert max(res[key][n] for n in D.NAMES) <= 1.0, D.report(key, res[key])


# ---------------------------------------------------------------------------------------------------------------------
# ns_finish through whole runs of dh_ns_ensemble
# ---------------------------------------------------------------------------------------------------------------------
NLIVE, QUEUE = 50, 16
OFFS, WIDTHS = (0.0, 800.0, -1.0e6), (5.0, 40.0)


def problem(c, a):
    """DH_LIKE_GAUSS_IID in 2-D, logl = -|v|^2 / 2 + c, under the affine prior of half-width a."""
    from dynesty_amd import problems as PR
    return PR.Problem(2, PR.LIKE_GAUSS_IID, [c], PR.PRIOR_AFFINE, [a, 0.0], name=f"gauss2_c{c:g}_a{a:g}")


def check_record(r, i, nlive, K, what, open_plateau=False):
    """Run i of the ensemble result r against the long-double compute_integrals over its own dead and live values with
    the volumes replayed from its record.  Returns (values, bounds) of logz, logzerr, h."""
    n = int(r["niter"][i])
    dead, ids, live = r["dead_logl"][i, :n], r["dead_id"][i, :n], r["live_logl"][i]
    lv = R.logvol_from_record(dead, ids, live, nlive)
    fin = H.integrals_hp(np.concatenate([dead, np.sort(live)]), lv)
    b = H.finish_bounds(fin, n, nlive, K, int(r["nfills"]), open_plateau=open_plateau)
    ref = dict(logz=fin["logz"], logzerr=np.sqrt(fin["logzvar"]), h=fin["h"])
    rt = {k: float(H.ratio(float(LD(r[k][i]) - ref[k]), b[k])) for k in ("logz", "logzerr", "h")}
    print(f"{what} run {i} ({n} deaths, {int(r['nfills'])} fills): error / bound " + " ".join(f"{k} {v:.3g}" for k, v in rt.items())
          + " | bounds " + " ".join(f"{k} {b[k]:.2g}" for k in ("logz", "logzerr", "h")))
    assert max(rt.values()) <= 1.0, (what, i, rt)
    return {k: float(r[k][i]) for k in ref}, b


@pytest.fixture(scope="module")
def whole_runs(ctx):
    out = {}
    for a in WIDTHS:
        for c in OFFS:
            out[c, a] = ctx.ns_ensemble(problem(c, a), 2, NLIVE, QUEUE, walks=25, bound="multi", entropy=[77], dlogz=0.5,
                                        max_iter=5000, want_samples=True)
    return out


@pytest.mark.parametrize("a", WIDTHS)
@pytest.mark.parametrize("c", OFFS)
def test_whole_run_record_is_inside_the_bounds(whole_runs, c, a):
    r = whole_runs[c, a]
    assert np.all(r["status"] == 0) and 100 < int(r["niter"].max()) < 3000
    if a == 40.0:  # the initial live set spans more than exp can hold
        assert r["dead_logl"][0, int(r["niter"][0]) - 1] - r["dead_logl"][0, 0] > 745
    for i in range(2):
        check_record(r, i, NLIVE, QUEUE, f"c = {c:g}, a = {a:g}")


@pytest.mark.parametrize("a", WIDTHS)
def test_shift_invariance_across_the_offsets(whole_runs, a):
    """PCG64 streams: the walks of the runs at different c are the same, and values shifted by c order alike as long as
    the sum does not round two of them together.  Where the death order IS the same, ln Z - c, H and the error agree
    within the sum of the two bounds; where it is not, every run has been held to its own reference above."""
    base = whole_runs[0.0, a]
    for c in OFFS[1:]:
        r = whole_runs[c, a]
        for i in range(2):
            n = int(base["niter"][i])
            same = int(r["niter"][i]) == n and np.array_equal(r["dead_id"][i, :n], base["dead_id"][i, :n])
            print(f"a = {a:g}, c = {c:g}, run {i}: death order {'identical' if same else 'differs'} from c = 0")
            if not same:
                continue
            v0, b0 = check_record(base, i, NLIVE, QUEUE, f"c = 0, a = {a:g}")
            v1, b1 = check_record(r, i, NLIVE, QUEUE, f"c = {c:g}, a = {a:g}")
            # (the values themselves differ by the rounding of logl + c: u |c| each, which moves ln Z by as much)
            assert abs((v1["logz"] - c) - v0["logz"]) <= b0["logz"] + b1["logz"] + 2 * H.U * abs(c)
            assert abs(v1["h"] - v0["h"]) <= b0["h"] + b1["h"]
            assert abs(v1["logzerr"] - v0["logzerr"]) <= b0["logzerr"] + b1["logzerr"]


def test_whole_run_with_open_plateaus(ctx):
    """walks = 2 with the bound in use from the start: rwalk hands back its start point about a quarter of the time, so
    there are plateaus all along the run.  A first ensemble runs free; `maxiter` then ends the same runs (PCG64 streams:
    the same deaths) after the death count at which most of them stand inside a plateau -- pcount > 0 in ns_finish,
    whose remaining plateau steps come before the rest of the live points."""
    for c in (0.0, 800.0):
        kw = dict(walks=2, bound="multi", entropy=[78], dlogz=0.5, max_iter=5000, want_samples=True,
                  first_update=dict(min_ncall=1, min_eff=100.0))
        free = ctx.ns_ensemble(problem(c, 5.0), 6, NLIVE, QUEUE, **kw)
        assert np.all(free["status"] == 0)
        d = free["dead_logl"]
        nmin = int(free["niter"].min())
        inside = np.array([[d[i, m - 1] == d[i, m] for i in range(6)] for m in range(60, nmin)])  # open after m deaths
        m = 60 + int(np.argmax(inside.sum(axis=1)))
        assert inside[m - 60].sum() > 0
        for i in range(6):
            check_record(free, i, NLIVE, QUEUE, f"walks = 2, c = {c:g}", open_plateau=True)
        r = ctx.ns_ensemble(problem(c, 5.0), 6, NLIVE, QUEUE, maxiter=m - 1, **kw)
        assert np.all(r["status"] == 0) and np.all(r["niter"] == m)
        np.testing.assert_array_equal(r["dead_logl"][:, :m], d[:, :m])
        nopen = sum(int(r["dead_logl"][i, m - 1] == r["live_logl"][i].min()) for i in range(6))
        print(f"c = {c:g}: {nopen} of 6 runs end inside a plateau after {m} deaths")
        assert nopen == inside[m - 60].sum()
        for i in range(6):
            check_record(r, i, NLIVE, QUEUE, f"walks = 2, c = {c:g}, maxiter = {m - 1}", open_plateau=True)


@pytest.mark.parametrize("c,a", [(0.0, 40.0), (800.0, 5.0), (-1.0e6, 5.0)])
def test_whole_run_without_the_live_points(ctx, c, a):
    """add_live = False (DH_NS_OPT_ADD_LIVE = 0): the record is the recurrence's state after the last death."""
    r = ctx.ns_ensemble(problem(c, a), 2, NLIVE, QUEUE, walks=25, bound="multi", entropy=[77], dlogz=0.5,
                        max_iter=5000, want_samples=True, add_live=False)
    assert np.all(r["status"] == 0)
    dlv = np.log((NLIVE + 1.0) / NLIVE)
    for i in range(2):
        n = int(r["niter"][i])
        dead, ids, live = r["dead_logl"][i, :n], r["dead_id"][i, :n], r["live_logl"][i]
        lv = R.logvol_from_record(dead, ids, live, NLIVE)[:n]
        lvp = np.concatenate([[0.0], lv[:-1]])
        steps = lvp - lv
        const = np.abs(steps - dlv) <= 8 * H.U * (np.abs(lv) + 1.0)
        steps = np.where(const, dlv, steps)
        pl = np.where(const, np.nan, lvp - np.log(NLIVE + 1.0))
        st0 = (0.0, -1.e300, 0.0, 0.0, -1.e300)
        hp = H.integrate_hp(dead, steps, st0)
        # every death counted as a fill of its own: no partition of the run into fills has a longer chain
        b = H.consume_bounds(hp, dead, steps, st0, np.arange(1, n + 1), QUEUE, NLIVE, plateau_pl=pl)
        var, bv = float(hp["logzvar"][-1]), float(b["logzvar"][-1])
        lin = bv / (2 * np.sqrt(abs(var) - bv)) if abs(var) > bv else np.inf
        got = dict(logz=r["logz"][i], h=r["h"][i], logzerr=r["logzerr"][i])
        ref = dict(logz=hp["logz"][-1], h=hp["h"][-1], logzerr=np.sqrt(abs(hp["logzvar"][-1])))
        bd = dict(logz=b["logz"][-1], h=b["h"][-1], logzerr=min(lin, np.sqrt(bv)) + 2 * H.U * np.sqrt(abs(var)))
        rt = {k: float(H.ratio(float(LD(got[k]) - ref[k]), bd[k])) for k in got}
        print(f"add_live = False, c = {c:g}, a = {a:g}, run {i} ({n} deaths): error / bound "
              + " ".join(f"{k} {v:.3g}" for k, v in rt.items()))
        assert max(rt.values()) <= 1.0, (c, a, i, rt)


def test_whole_run_through_the_global_memory_sort(ctx):
    """nlive = 9000: beyond the register sort's reach, ns_finish orders the final live points by its bitonic network in
    global memory (ns_finish_big); maxiter ends the run normally after 2000 deaths."""
    N, K = 9000, 64
    for c in (0.0, -1.0e6):
        r = ctx.ns_ensemble(problem(c, 5.0), 1, N, K, walks=25, bound="multi", entropy=[79], dlogz=0.01, max_iter=4000,
                            maxiter=2000, want_samples=True)
        assert np.all(r["status"] == 0) and 1900 <= int(r["niter"][0]) <= 2100
        check_record(r, 0, N, K, f"nlive = {N}, c = {c:g}")
