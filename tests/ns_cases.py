"""Seeded inputs of the run loop's evidence integration at the value scales tests/test_gpu_ns_consume.py does not
reach (tests/test_ns_hp_cpu.py, tests/test_gpu_ns_hp.py; reference and bounds: tests/ns_hp_ref.py).

A case is a chain of queue fills over `runs` independent runs: the initial live set, the incoming state, and per fill
a queue of proposals with their call counts.  Everything is regenerated from the seed; the queue of a fill is drawn
against the live set the oracle (oracle/nested_ref.consume_queue, float64) leaves behind, so building a case runs the
oracle, whose record of every fill -- deaths, slots, sources, every death's -d ln X, the state -- rides along.

Shape axis (nlive, K): the smallest shapes at which each route of csrc/ns.hip is still taken --
  (50, 17) kEPT = 1; (50, 257) kEPT = 2; (300, 600) EPT = 3 in the kEPT = 4 instance; (300, 1300) EPT = 6 in kEPT = 8;
  (300, 2048) the largest queue; (4, 5), (5, 64) the largest -d ln X (dh_ns_consume takes nlive >= 4);
  (9000, 700) ns_consume_compact; (40000, 300) the smallest step under expm1.
Value axis: base, offsets, range, floor, ties at offset, late, stop (see `build`).
Every value family at (50, 257) and (300, 600); base, floor and ties at every shape."""
import functools

import numpy as np

from oracle import nested_ref as R

SHAPES = [(50, 17), (50, 257), (300, 600), (300, 1300), (300, 2048), (4, 5), (5, 64), (9000, 700), (40000, 300)]
FULL = [(50, 257), (300, 600)]  # every value family
OFFSETS = [800.0, -800.0, 1.0e6, -1.0e6]
FLOORS = [-800.0, -1.0e4, -1.0e30]
NEVER = 1e-300  # a dlogz the stopping rule cannot reach


def _runs(nlive):
    return 2 if nlive <= 300 else 1


def _nfills(nlive, K):
    return 5 if K <= 64 else 3


def all_keys():
    keys = []
    for i, (n, k) in enumerate(SHAPES):
        keys.append(f"base/{n}x{k}")
        keys.append(f"floor{FLOORS[i % 3]:g}/{n}x{k}")
        keys.append(f"ties400{'+' if i % 2 == 0 else '-'}1e6/{n}x{k}")
        keys.append(f"ties40{'-' if i % 2 == 0 else '+'}1e6/{n}x{k}")
    for n, k in FULL:
        for c in OFFSETS:
            keys.append(f"offset{c:+g}/{n}x{k}")
        keys.append(f"range/{n}x{k}")
        for f in FLOORS:
            kk = f"floor{f:g}/{n}x{k}"
            if kk not in keys:
                keys.append(kk)
        for t in ("ties400-1e6", "ties400+1e6", "ties40+1e6", "ties40-1e6"):
            if f"{t}/{n}x{k}" not in keys:
                keys.append(f"{t}/{n}x{k}")
        keys.append(f"late-700/{n}x{k}")
        keys.append(f"late-5000/{n}x{k}")
        keys.append(f"stop/{n}x{k}")
    return keys


def family(key):
    f = key.split("/")[0]
    for name in ("base", "offset", "range", "floor", "ties", "late", "stop"):
        if f.startswith(name):
            return name
    raise KeyError(key)


def _shape(key):
    n, k = key.split("/")[1].split("x")
    return int(n), int(k)


def _seed(key):
    return int.from_bytes(key.encode(), "little") % (2**63)


def _ball(rng, n, rad):
    """-r^2 / 2 of points uniform in a 6-D ball: the draw of tests/test_gpu_ns_consume.py."""
    return -0.5 * (rad * rng.random(n) ** (1 / 6.0)) ** 2


# how many of the nlive initial points sit on the floor: the plateau ends inside the first fill where K allows it
# ((50, 257): the fill that goes on to the top values -- the case whose var ln Z the float64 scan form loses), and is
# carried across fills through `plateau` where K < m ((50, 17), (300, 2048) with m = 280 of which the stale queue
# entries leave some for the next fill, (9000, 700), (40000, 300))
def _nfloor(nlive, K):
    return {(50, 17): 20, (50, 257): 20, (300, 600): 120, (300, 1300): 40, (300, 2048): 280, (4, 5): 2, (5, 64): 3,
            (9000, 700): 1000, (40000, 300): 400, (5000, 700): 1000}[(nlive, K)]


class Case:
    """live0 (runs, N); state0: list of RunState; fills: list of (q_logl (runs, K), q_ncalls (runs, K));
    ref[r][f]: the oracle's record of fill f of run r (consume_queue's dict plus `state`: a copy of the RunState after
    the fill, `live`: the live set after it, `live_it`)."""


@functools.lru_cache(maxsize=None)
def build(key, dlogz=None):
    fam, (N, K) = family(key), _shape(key)
    rng = np.random.default_rng(_seed(key))
    runs, nf = _runs(N), _nfills(N, K)
    c = Case()
    c.key, c.family, c.nlive, c.K, c.runs = key, fam, N, K, runs
    c.dlogz = NEVER if dlogz is None else dlogz
    off = 0.0
    vals = None
    states = [R.RunState(N) for _ in range(runs)]
    tag = key.split("/")[0]
    if fam in ("base", "stop"):
        live = np.stack([_ball(rng, N, 6.0) for _ in range(runs)])
    elif fam == "offset":
        off = float(tag[len("offset"):])
        live = np.stack([_ball(rng, N, 6.0) for _ in range(runs)]) + off
    elif fam == "range":
        assert K >= N
        live = np.where(rng.random((runs, N)) < 0.5, -2000.0 + 100.0 * rng.random((runs, N)), -10.0 * rng.random((runs, N)))
    elif fam == "floor":
        F, m = float(tag[len("floor"):]), _nfloor(N, K)
        live = -10.0 * rng.random((runs, N))
        for r in range(runs):
            live[r, rng.permutation(N)[:m]] = F
    elif fam == "ties":
        nlev = 400 if tag.startswith("ties400") else 40
        off = float(tag[-4:])
        vals = -np.sort(rng.random(nlev) * 20) + off
        live = vals[rng.integers(0, nlev, size=(runs, N))].copy()
    elif fam == "late":
        lx0 = float(tag[len("late"):])
        live = -2.0 * rng.random((runs, N))
        for r, s in enumerate(states):
            s.logvol = lx0 - 0.25 * r
            s.logz = lx0 - 1.0 + live[r].min()
            s.h, s.logzvar = 2.0 + r, 0.01
            s.loglstar = live[r].min() - 0.125
            s.it = int(round(-lx0 / s.dlv))
    if fam == "stop" and dlogz is None:
        c.dlogz = stop_dlogz(key)
    c.live0 = live.copy()
    c.state0 = [s.copy() for s in states]
    c.fills = []
    c.ref = [[] for _ in range(runs)]
    cur = live.copy()
    live_it = np.zeros((runs, N), dtype=np.int64)
    done = np.zeros(runs, bool)
    for f in range(nf):
        ql = np.empty((runs, K))
        for r in range(runs):
            lo, hi = cur[r].min(), cur[r].max()
            if fam in ("base", "stop", "offset"):
                ql[r] = _ball(rng, K, np.sqrt(-2 * (lo - off)) * 1.05) + off  # about a quarter stale at birth
            elif fam == "ties":
                ql[r] = vals[rng.integers(0, len(vals), size=K)]
                ql[r, ::3] += 0.5  # some entries off the grid
            else:
                top = max(hi, -10.0 if fam != "late" else -2.0)
                base = max(lo, top - 10.0)
                ql[r] = base - 0.05 * (top - base + 1.0) + (1.05 * (top - base) + 0.05) * rng.random(K) ** 0.5
                ql[r] = np.minimum(ql[r], 0.0)
        qn = rng.integers(1, 60, size=(runs, K)).astype(np.int32)
        c.fills.append((ql, qn))
        for r in range(runs):
            if done[r]:
                c.ref[r].append(None)
                continue
            rec = R.consume_queue(cur[r], ql[r], qn[r], states[r], c.dlogz, plateau=True, live_it=live_it[r])
            rec["state"], rec["live"], rec["live_it"] = states[r].copy(), cur[r].copy(), live_it[r].copy()
            c.ref[r].append(rec)
            done[r] = rec["stopped"]
    return c


@functools.lru_cache(maxsize=None)
def stop_dlogz(key):
    """A dlogz that the rule meets inside the SECOND fill: half way between the dz of two consecutive deaths in the
    middle of that fill (dz as the float64 oracle sees it on an unstopped chain; the margin against the long-double dz
    and its bound is asserted by tests/test_ns_hp_cpu.py)."""
    free = build(key, NEVER)
    dzs = []
    for r in range(free.runs):
        rec0, rec1 = free.ref[r][0], free.ref[r][1]
        dz = chain_dz(free, r)
        n0, n1 = len(rec0["dead_logl"]), len(rec1["dead_logl"])
        e = n0 + n1 // 2
        dzs.append(0.5 * (dz[e] + dz[e + 1]))
    return float(min(dzs))  # run with the smaller value stops in its second fill; the other at or after it


def chain_lmax(case, r):
    """The largest live value after every death of run r's chain (the stopping rule's L_max)."""
    live = case.live0[r].copy()
    out = []
    for f, rec in enumerate(case.ref[r]):
        if rec is None:
            break
        ql = case.fills[f][0][r]
        m = live.max()
        for e in range(len(rec["dead_logl"])):
            live[rec["dead_slot"][e]] = ql[rec["dead_src"][e]]
            m = max(m, ql[rec["dead_src"][e]])  # (the largest value is the last to die)
            out.append(m)
    return np.array(out)


def chain_dz(case, r):
    """The stopping rule's delta ln Z after every death of run r's chain (float64, the oracle's recurrence)."""
    ch = chain_inputs(case, r)
    s = case.state0[r].copy()
    lmax = chain_lmax(case, r)
    out = []
    for k in range(len(ch["dead"])):
        lnew, step = ch["dead"][k], ch["steps"][k]
        s.logvol -= step
        _, s.logz, s.logzvar, s.h = R.progress_integration(s.loglstar, lnew, s.logz, s.logzvar, s.logvol, step, s.h)
        s.loglstar = lnew
        out.append(np.logaddexp(0, lmax[k] + s.logvol - s.logz))
    return np.array(out)


def chain_inputs(case, r):
    """Run r's whole chain as the integration sees it: dead values, every death's -d ln X, the plateau's ln volume
    step (nan outside plateaus), the 1-based death counts at which the fills end, and the incoming state
    (logvol, logz, h, logzvar, last dead value)."""
    recs = [x for x in case.ref[r] if x is not None]
    s = case.state0[r]
    ends = np.cumsum([len(x["dead_logl"]) for x in recs])
    return dict(dead=np.concatenate([x["dead_logl"] for x in recs]), steps=np.concatenate([x["dead_dlv"] for x in recs]),
                pl=np.concatenate([x["dead_pl"] for x in recs]), ends=ends,
                state0=(s.logvol, s.logz, s.h, s.logzvar, s.loglstar))
