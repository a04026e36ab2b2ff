"""Test infrastructure: one run of the device-resident loop with a RadFriends / SupFriends bound and the uniform
sampler (dh_ns_ensemble, bound code 2 / 3, sampler 6) restated on the host, event for event.

As tests/resident_mirror.py does for the ellipsoids, the loop's CONTROL is restated here in its own random-choice
protocol (ns_init / ns_prepare / ns_select); the numerical steps are the library's single-call entry points:
dh_friends_update (the bound update, clustering in the run's previous metric -- the identity before the first one),
dh_unif_friends_batch (the queue's proposals, the shapes on the run's live points of the fill), dh_unif_batch (the
unit-cube phase) and dh_ns_consume.  The bootstrap replicas' in-sample masks are restated from their streams
(boot_mask: _bootstrap_points, bounding.py:1593-1616, on oracle.nested_ref.boot_generator); the enlargement is
scale_to_logvol (bounding.py:765-774) in NumPy.  The uniform sampler has no start points, hence no membership test and
no forced update: with friends bounds a live point is always the centre of its own shape, so the reference's forced
update (sampler.py:484-489) could not fire either.
"""
import math

import numpy as np

from resident_mirror import Pcg, child_words, M64


def boot_mask(n, ent, b):
    """The in-sample mask of replica b (bounding.py:1593-1616): integers(n, size=n) from boot_generator(ent, b),
    sel[unique(idxs)] = True; fewer than two in the sample -> the first two join; all in -> the first leaves (both
    decided on the count before either is applied)."""
    from oracle.nested_ref import boot_generator
    g = boot_generator(ent, b)
    idxs = g.integers(n, size=n)
    sel = np.zeros(n, dtype=bool)
    sel[np.unique(idxs)] = True
    n_in = int(sel.sum())
    if n_in < 2:
        sel[:2] = True
    if n_in > n - 1:
        sel[0] = False
    return sel


def scale_to_logvol(b, logvol):
    """RadFriends / SupFriends.scale_to_logvol (bounding.py:765-774)."""
    f = np.exp((logvol - b["logvol"]) * (1.0 / b["cov"].shape[0]))
    b["cov"] = b["cov"] * f**2
    b["am"] = b["am"] / f**2
    b["axes"] = b["axes"] * f
    b["axes_inv"] = b["axes_inv"] / f
    b["logvol"] = logvol


def mirror_friends_run(ctx, prob, nlive, K, kind, entropy, run, dlogz, enlarge=1.0, bootstrap=5, first_run=0,
                       max_fills=100000, forced="exact"):
    """The run with global index first_run + run of ns_ensemble(prob, ..., bound=kind, sample='unif',
    rebuild_every=1, enlarge=enlarge, bootstrap=bootstrap)."""
    N, D, grun = nlive, prob.ndim, first_run + run
    live_u = np.empty((N, D))
    for i in range(N):
        g = Pcg(child_words(entropy, grun * N + i))
        live_u[i] = [g.next_double() for _ in range(D)]
    rg = Pcg(child_words(entropy, 0x80000000 + grun))
    live_v, live_logl = ctx.problem_eval(prob, live_u)
    live_l2 = np.ascontiguousarray(live_logl, dtype=np.float64)[None, :]
    live_logl = live_l2[0]
    state = np.array([[0., -1.e300, 0., 0., -1.e300, 0., float(N), 0.]])
    plateau = np.zeros((1, 2))
    live_it2 = np.zeros((1, N), dtype=np.int32)
    loglstar = float(live_logl.min())
    update_interval = N  # UniformBoundSampler: ratio 1 (internal_samplers.py:88-94)
    first_ncall, first_eff = 2 * N, 10.0
    cube, nbound, ncall_last = True, 0, 0
    undo = None
    bnd = dict(am=np.eye(D))  # RadFriends(ndim) / SupFriends(ndim) with cov=None
    ev = dict(dead_logl=[], dead_slot=[], dead_src=[], fill_of_death=[], rebuild_fills=[], nclusters=[])

    def rebuild():
        nonlocal nbound
        masks = None
        if bootstrap > 0:
            # the words ns_prepare draws from the run's generator when the rebuild is decided
            bent = [rg.next64() for _ in range(4)]
            masks = np.array([boot_mask(N, bent, b) for b in range(bootstrap)])
        res = ctx.friends_update(live_u, kind, am_prev=bnd["am"], in_masks=masks)
        bnd.update(cov=res["cov"], am=res["am"], axes=res["axes"], axes_inv=res["axes_inv"], logvol=res["logvol"])
        ev["nclusters"].append(res["nclusters"])
        if enlarge != 1.0:
            scale_to_logvol(bnd, bnd["logvol"] + math.log(enlarge))
        nbound += 1

    fill = 0
    done = False
    while not done and fill < max_fills:
        it, ncall = int(state[0, 5]), int(state[0, 6])
        eff = 100.0 * max(it, 1) / ncall
        want = (ncall >= first_ncall and eff < first_eff) if cube else (ncall >= ncall_last + update_interval)
        if want:
            cube = False
            if forced == "exact" and undo is not None:
                # the regular update is built from the live set without the newest point (sampler.py:771-772)
                keep = live_u[undo[0]].copy()
                live_u[undo[0]] = undo[1]
                rebuild()
                live_u[undo[0]] = keep
            else:
                rebuild()
            ncall_last = ncall
            ev["rebuild_fills"].append(fill)
        ent = [rg.next64() for _ in range(4)]
        states = np.empty((K, 4), dtype=np.uint64)
        for w in range(K):
            g = Pcg()
            g.seed((ent[0] << 64) | ((ent[1] + w) & M64), (ent[2] << 64) | ((ent[3] + 2 * w) & M64))
            states[w] = g.words()
        if cube:
            out = ctx.unif_batch(prob, loglstar, states)
        else:
            # the shapes sit on the live points of this fill (internal_samplers.py:232-233)
            out = ctx.unif_friends_batch(prob, loglstar, states, live_u.copy(), kind, bnd["axes"], bnd["axes_inv"])
        q_nc = out["ncalls"].astype(np.int32)
        q_logl = np.ascontiguousarray(out["logl"], dtype=np.float64)
        res = ctx.ns_consume(live_l2, q_logl[None], q_nc[None], state, dlogz, live_it=live_it2, plateau=plateau)
        slots, srcs = res["dead_slot"][0].astype(np.int64), res["dead_src"][0].astype(np.int64)
        ev["dead_logl"].extend(res["dead_logl"][0].tolist())
        ev["dead_slot"].extend(slots.tolist())
        ev["dead_src"].extend(srcs.tolist())
        ev["fill_of_death"].extend([fill] * len(slots))
        undo = None
        if len(slots) and srcs[-1] == K - 1:
            sl = int(slots[-1])
            prev = [e for e in range(len(slots) - 1) if slots[e] == sl]
            undo = (sl, (out["u"][srcs[prev[-1]]] if prev else live_u[sl]).copy())
        if len(slots):
            order = np.argsort(slots, kind="stable")
            same = slots[order][1:] == slots[order][:-1]
            last = np.ones(len(slots), dtype=bool)
            last[order[:-1][same]] = False
            live_u[slots[last]] = out["u"][srcs[last]]
            live_v[slots[last]] = out["v"][srcs[last]]
        loglstar = float(state[0, 7])
        fill += 1
        if res["stopped"][0] or np.ptp(live_logl) == 0:
            done = True
    from oracle import nested_ref as R
    dead, ids = np.array(ev["dead_logl"]), np.array(ev["dead_slot"], dtype=np.int64)
    lv = R.logvol_from_record(dead, ids, live_logl.copy(), N)
    _, logz, _, _ = R.compute_integrals(np.concatenate([dead, np.sort(live_logl)]), lv)
    ev.update(niter=int(state[0, 5]), ncall=int(state[0, 6]), nbound=nbound, nfills=fill, logz=float(logz[-1]),
              live_logl=live_logl.copy(), live_u=live_u.copy(), done=done)
    return ev
