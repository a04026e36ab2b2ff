"""Test infrastructure: one strand of a dynamic batch (csrc/ns.hip, dh_ns_batch) restated on the host, event for event,
in the way tests/resident_mirror.py restates a run of the resident loop (whose generator and child-stream helpers are
used as they are).

Restated here is the CONTROL of the seeding phase and the hand-over -- ns_batch_init (the strand's generator, the
bootstrap words of the one bound update), the seed fills at the fixed threshold logl_min with start points among the
seeds (ns_select's protocol: four words of the strand's generator seed the fill's K selection streams), ns_seed_consume
(queue order, nc with the rejected entries' calls, every call charged, one tuning step per fill, nothing replaced),
ns_batch_start -- and then the ordinary loop in its forced-exact form with rebuild_every = 1 (copied from
resident_mirror._mirror, bound mode only) for as many deaths as asked.  The numerical steps are the library's own entry
points, called one at a time (bound.update -> dh_rebuild, scale_to_logvol, contains_many, dh_rwalk_batch,
dh_unif_batch, dh_ns_consume), so a mirrored strand and the strand inside dh_ns_batch take the same proposals."""
import math

import numpy as np

from resident_mirror import M64, Pcg, child_words


def mirror_strand(ctx, prob, seed_u, seed_logl, logl_min, start, K, walks, bound, entropy, grun, dlogz, ndeaths,
                  sample="rwalk", enlarge=1.25, bootstrap=0):
    """Strand with global index `grun` of ns_batch(prob, seed_u[None], ..., rebuild_every=1, forced_exact=True):
    sample = 'rwalk' | 'unif'.  Returns the start set, seed_ncall, the generator at the hand-over and the first deaths
    (at least ndeaths, whole fills) with their slot, it and nc."""
    from dynesty_amd import backend
    backend.set_backend(ctx)
    try:
        return _mirror(ctx, prob, np.array(seed_u, dtype=np.float64), np.array(seed_logl, dtype=np.float64),
                       float(logl_min), [float(x) for x in start], K, walks, bound, entropy, grun, dlogz, ndeaths, sample,
                       enlarge, bootstrap)
    finally:
        backend.set_backend(None)


def _mirror(ctx, prob, live_u, live_logl, logl_min, start, K, walks, bound, entropy, grun, dlogz, ndeaths, sample, enlarge,
            bootstrap):
    from dynesty_amd import bounding
    N, D = live_u.shape
    # ---- ns_batch_init ----
    rg = Pcg(child_words(entropy, 0x80000000 + grun))
    scale, nbound, ncall, ncall_last = start[5], 0, 0, 0
    facc = min(1.0, max(1.0 / max(walks, 2), 0.5))
    update_interval = N if sample == "unif" else walks * N
    bnd = None

    def rebuild(bent=None):
        nonlocal bnd, nbound
        if bnd is None:
            bnd = (bounding.HipMultiEllipsoid if bound == "multi" else bounding.HipEllipsoid)(D)
        bnd.update(live_u)
        if bootstrap > 0:
            if bent is None:  # four words of the strand's generator, drawn when the rebuild is decided
                bent = np.array([[rg.next64() for _ in range(4)]], dtype=np.uint64)
            f = float(ctx.bootstrap_expand(live_u[None], bent, bootstrap, bound == "multi")[0])
            if f > 1.0:
                bnd.scale_to_logvol(bnd.logvol + D * math.log(f))
        if enlarge != 1.0:
            bnd.scale_to_logvol(bnd.logvol + math.log(enlarge))
        nbound += 1

    def frames_of():
        if bound == "multi":
            return np.array(bnd.axes_ells, dtype=np.float64).copy(), np.array(bnd.logvol_ells, dtype=np.float64).copy()
        return np.array(bnd.axes, dtype=np.float64)[None].copy(), np.zeros(1)

    def cum_of(lv):  # ns_select: cumsum(exp(lv - max)) / total
        e = np.exp(lv - lv.max())
        c, out = 0.0, np.empty(len(lv))
        for j, x in enumerate(e):
            c += x
            out[j] = c
        return out * (1.0 / c)

    def pick(cum, xr):  # first index with cum >= xr, capped
        lo, hi = 0, len(cum) - 1
        while lo < hi:
            mid = (lo + hi) >> 1
            if cum[mid] < xr:
                lo = mid + 1
            else:
                hi = mid
        return lo

    def select(loglstar):
        """ns_select: the fill's four words, then per entry its selection stream: start point, frame variate"""
        ent = [rg.next64() for _ in range(4)]
        states = np.empty((K, 4), dtype=np.uint64)
        st = np.zeros(K, dtype=np.int64)
        xr = np.zeros(K)
        multi = bound == "multi" and bnd.nells > 1
        for w in range(K):
            g = Pcg()
            g.seed((ent[0] << 64) | ((ent[1] + w) & M64), (ent[2] << 64) | ((ent[3] + 2 * w) & M64))
            if sample != "unif":
                while True:
                    i = g.interval(N - 1)
                    if live_logl[i] > loglstar:
                        break
                st[w] = i
                if multi:
                    xr[w] = g.next_double()
            states[w] = g.words()
        return ent, states, st, xr, multi

    def unif_fill(loglstar, states):
        if bound == "multi":
            out = ctx.unif_batch(prob, loglstar, states, ctrs=bnd.ctrs, axes=bnd.axes_ells, ams=bnd.ams,
                                 logvol_ells=bnd.logvol_ells)
        else:
            out = ctx.unif_batch(prob, loglstar, states, ctrs=bnd.ctr, axes=bnd.axes)
        return out, out["ncalls"].astype(np.int32)

    def tune(ta, tr):
        nonlocal scale
        if sample == "rwalk" and ta + tr > 0:  # RWalkSampler.tune, once per fill
            scale *= math.exp((ta / (ta + tr) - facc) / D / facc)

    # the one bound of the seeding phase: built on the seeds at call count 0, its bootstrap words drawn first
    rebuild(np.array([[rg.next64() for _ in range(4)]], dtype=np.uint64) if bootstrap > 0 else None)
    # ---- the seed fills and ns_seed_consume ----
    su, sv, sl, snc = [], [], [], []
    pend, seed_fills = 0, 0
    while len(sl) < N:
        _, states, st, xr, multi = select(logl_min)
        if sample == "unif":
            out, q_nc = unif_fill(logl_min, states)
            ta = tr = 0
        else:
            axes, lv = frames_of()
            cum = cum_of(lv) if multi else None
            fidx = np.array([pick(cum, xr[w]) if multi else 0 for w in range(K)], dtype=np.int32)
            out = ctx.rwalk_batch(prob, live_u[st], axes, scale, logl_min, walks, states, axes_idx=fidx)
            q_nc = np.full(K, walks, dtype=np.int32)
            ta, tr = int(out["accept"].sum()), int(out["reject"].sum())
            out["logl"] = np.where(out["accept"] == 0, live_logl[st], out["logl"])
        for j in range(K):
            c = int(q_nc[j])
            if len(sl) < N and out["logl"][j] > logl_min:
                su.append(out["u"][j].copy())
                sv.append(out["v"][j].copy())
                sl.append(float(out["logl"][j]))
                snc.append(pend + c)
                pend = 0
            else:
                pend += c
        ncall += int(q_nc.sum())
        tune(ta, tr)
        seed_fills += 1
    # ---- ns_batch_start ----
    live_u, live_v = np.array(su), np.array(sv)
    live_l2 = np.array(sl)[None, :].copy()
    live_logl = live_l2[0]
    ev = dict(start_u=live_u.copy(), start_logl=live_logl.copy(), start_nc=np.array(snc), seed_ncall=ncall,
              seed_rng=rg.words(), seed_fills=seed_fills, scale_at_start=scale,
              dead_logl=[], dead_slot=[], dead_it=[], dead_nc=[])
    state = np.array([[start[0], start[1], start[2], start[3], start[4], 0., float(ncall), 0.]])
    plateau = np.zeros((1, 2))
    live_it2 = np.zeros((1, N), dtype=np.int32)
    loglstar = float(live_logl.min())
    carry, undo = 0, None
    # ---- the loop (resident_mirror._mirror, bound mode, forced = 'exact', rebuild_every = 1) ----
    done = False
    while not done and len(ev["dead_logl"]) < ndeaths:
        ncall = int(state[0, 6])
        if ncall >= ncall_last + update_interval:
            if undo is not None:
                keep = live_u[undo[0]].copy()
                live_u[undo[0]] = undo[1]
                rebuild()
                live_u[undo[0]] = keep
            else:
                rebuild()
            ncall_last = ncall
        ent, states, st, xr, multi = select(loglstar)
        if sample == "unif":
            out, q_nc = unif_fill(loglstar, states)
            ta = tr = 0
        else:
            axes, lv = frames_of()
            cum = cum_of(lv) if multi else None
            fidx = np.array([pick(cum, xr[w]) if multi else 0 for w in range(K)], dtype=np.int32)
            u0 = live_u[st]
            inside = np.asarray(bnd.contains_many(u0)) if bound == "multi" else np.array([bnd.contains(x) for x in u0])
            if not inside.all():
                # sampler.py:484-489 inside the fill: entries up to the first one outside keep the old frames
                jstar = int(np.argmin(inside))
                rebuild()
                ncall_last = ncall - carry
                new_axes, new_lv = frames_of()
                multi2 = bound == "multi" and bnd.nells > 1
                cum2 = cum_of(new_lv) if multi2 else None
                nold = len(axes)
                for w in range(jstar + 1, K):
                    if multi2:
                        g = Pcg()
                        g.seed((ent[0] << 64) | ((ent[1] + w) & M64), (ent[2] << 64) | ((ent[3] + 2 * w) & M64))
                        while True:
                            i = g.interval(N - 1)
                            if live_logl[i] > loglstar:
                                break
                        fidx[w] = nold + pick(cum2, g.next_double())
                    else:
                        fidx[w] = nold
                axes = np.concatenate([axes, new_axes])
            out = ctx.rwalk_batch(prob, u0, axes, scale, loglstar, walks, states, axes_idx=fidx)
            q_nc = np.full(K, walks, dtype=np.int32)
            ta, tr = int(out["accept"].sum()), int(out["reject"].sum())
            out["logl"] = np.where(out["accept"] == 0, live_logl[st], out["logl"])
        q_logl = np.ascontiguousarray(out["logl"], dtype=np.float64)
        res = ctx.ns_consume(live_l2, q_logl[None], q_nc[None], state, dlogz, live_it=live_it2, plateau=plateau)
        slots, srcs = res["dead_slot"][0].astype(np.int64), res["dead_src"][0].astype(np.int64)
        nc = res["dead_nc"][0].astype(np.int64)
        if len(nc):
            nc[0] += carry  # (the operator starts every call without a carry: the loop's is kept here)
        ev["dead_logl"].extend(res["dead_logl"][0].tolist())
        ev["dead_slot"].extend(slots.tolist())
        ev["dead_it"].extend(res["dead_it"][0].tolist())
        ev["dead_nc"].extend(nc.tolist())
        carry = int(q_nc[srcs[-1] + 1:].sum()) if len(slots) else carry + int(q_nc.sum())
        undo = None
        if len(slots) and srcs[-1] == K - 1:
            s_ = int(slots[-1])
            prev = [e for e in range(len(slots) - 1) if slots[e] == s_]
            undo = (s_, (out["u"][srcs[prev[-1]]] if prev else live_u[s_]).copy())
        if len(slots):
            order = np.argsort(slots, kind="stable")
            same = slots[order][1:] == slots[order][:-1]
            last = np.ones(len(slots), dtype=bool)
            last[order[:-1][same]] = False
            live_u[slots[last]] = out["u"][srcs[last]]
            live_v[slots[last]] = out["v"][srcs[last]]
        tune(ta, tr)
        loglstar = float(state[0, 7])
        if res["stopped"][0] or np.ptp(live_logl) == 0:
            done = True
    ev.update(nbound=nbound, done=done)
    return ev
