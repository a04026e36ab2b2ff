"""Runs the cases of tests/ns_cases.py through dh_ns_consume and holds the outcome to the oracle (integer work: exact)
and to the long-double reference (tests/ns_hp_ref.py: error / bound per quantity).  Shared by tests/test_gpu_ns_hp.py
and by the child process it starts with DH_NS_SERIAL=1 (`python ns_hp_device.py key ...` prints one JSON line)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as a script: the oracle lives at the repository's root)
    sys.path.insert(0, ROOT)

import ns_cases as C  # noqa: E402
import ns_hp_ref as H  # noqa: E402

LD = H.LD
NAMES = H.QUANT + ("plateau_logdvol",)


def pack(states):
    return np.array([[s.logvol, s.logz, s.h, s.logzvar, s.loglstar, s.it, s.ncall, 0.0] for s in states])


def run_case(ctx, key, pad_to=None):
    """The chain of fills of a case on the device.  Returns {name: worst error / bound}; the exact part is asserted
    here.  A run that has stopped leaves the ensemble, as MODE_DONE runs do.  pad_to: every queue is lengthened to
    pad_to entries by stale ones of one call each behind the case's own (the same deaths at another shape: the pads
    are popped after the fill's last death and only count into the run's calls)."""
    case = C.build(key)
    runs, N = case.runs, case.nlive
    K = pad_to or case.K
    npad = K - case.K
    live = case.live0.copy()
    state = pack(case.state0)
    live_it = np.zeros((runs, N), dtype=np.int32)
    plat = np.zeros((runs, 2))
    evald = []
    for r in range(runs):
        ch = C.chain_inputs(case, r)
        hp = H.integrate_hp(ch["dead"], ch["steps"], ch["state0"])
        b = H.consume_bounds(hp, ch["dead"], ch["steps"], ch["state0"], ch["ends"], K, N, plateau_pl=ch["pl"])
        evald.append((ch, hp, b, H.fill_rows(hp, b, ch["ends"], ch["state0"])))
    worst = dict.fromkeys(NAMES, 0.0)
    nplateau = 0
    for f, (ql, qn) in enumerate(case.fills):
        act = np.array([case.ref[r][f] is not None for r in range(runs)])
        if not act.any():
            break
        if npad:
            ql = np.concatenate([ql, np.repeat(live.min(axis=1)[:, None] - 1.0, npad, axis=1)], axis=1)
            qn = np.concatenate([qn, np.ones((runs, npad), dtype=np.int32)], axis=1)
        la, sa = np.ascontiguousarray(live[act]), np.ascontiguousarray(state[act])
        ia, pa = np.ascontiguousarray(live_it[act]), np.ascontiguousarray(plat[act])
        out = ctx.ns_consume(la, np.ascontiguousarray(ql[act]), np.ascontiguousarray(qn[act]), sa, case.dlogz,
                             live_it=ia, plateau=pa)
        live[act], state[act], live_it[act], plat[act] = la, sa, ia, pa
        for i, r in enumerate(np.flatnonzero(act)):
            ref = case.ref[r][f]
            s = ref["state"]
            for k in ("dead_logl", "dead_slot", "dead_src", "dead_it", "dead_nc"):
                np.testing.assert_array_equal(out[k][i], ref[k], err_msg=f"{key} run {r} fill {f} {k}")
            np.testing.assert_array_equal(live[r], ref["live"], err_msg=f"{key} run {r} fill {f} live set")
            np.testing.assert_array_equal(live_it[r], ref["live_it"], err_msg=f"{key} run {r} fill {f} live_it")
            assert bool(out["stopped"][i]) == ref["stopped"], (key, r, f)
            assert int(state[r, 5]) == s.it and int(state[r, 6]) == s.ncall + (f + 1) * npad and state[r, 7] == ref["live"].min()
            assert state[r, 4] == s.loglstar
            ch, hp, b, (rows, bd) = evald[r]
            rt = H.ratio(np.asarray(state[r, :4].astype(LD) - rows[f], dtype=np.float64), bd[f])
            for q, name in enumerate(H.QUANT):
                worst[name] = max(worst[name], float(rt[q]))
            assert int(plat[r, 0]) == (s.plateau_counter if s.plateau_mode else 0), (key, r, f)
            if s.plateau_mode:
                nplateau += 1
                e = int(ch["ends"][f])
                j, lv_start = H.open_plateau(hp, ch["pl"], e, ch["state0"], s.plateau_logdvol)
                pl = H.plogdvol_hp(lv_start, N)
                bl = b["logvol"][e - 1] if e else 0.0
                rp = float(H.ratio(float(LD(plat[r, 1]) - pl), H.plogdvol_bound(bl, j, N, float(pl))))
                worst["plateau_logdvol"] = max(worst["plateau_logdvol"], rp)
    worst["plateaus_carried"] = nplateau
    return worst


def report(key, worst):
    return f"{key}: error / bound " + " ".join(f"{n} {worst[n]:.3g}" for n in NAMES)


if __name__ == "__main__":
    from dynesty_amd import _lib
    ctx = _lib.Context(0)
    print(json.dumps({k: run_case(ctx, k) for k in sys.argv[1:]}))
