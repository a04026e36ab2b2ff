"""Synthetic run ensembles for the combiner tests (tests/test_merge_hp_cpu.py, tests/test_gpu_merge.py): sorted
log-likelihoods that are drawn, not sampled -- the combiner only needs each run's dead values non-decreasing and its
final live values above them."""
import numpy as np


def make(rng, niters, N, D, span=30.0):
    """Runs with niters[r] dead points and N live ones; unit-cube rows random.  Returns the keyword arguments of
    ensemble.merge_static_runs / Context.merge_runs (lists per run for the dead arrays)."""
    R = len(niters)
    out = dict(niter=np.array(niters, dtype=np.int64), dead_logl=[], live_logl=np.empty((R, N)), dead_u=[],
               live_u=rng.random((R, N, D)), dead_id=[], dead_it=[], dead_nc=[],
               live_it=rng.integers(0, 1000, size=(R, N)))
    for r, k in enumerate(niters):
        # ln L ~ -span * X^(2/D)-like ladder: increasing, flattening towards the top
        all_l = np.sort(-span * rng.random(k + N) ** 2)
        out["dead_logl"].append(all_l[:k])
        out["live_logl"][r] = rng.permutation(all_l[k:])
        out["dead_u"].append(rng.random((k, D)))
        out["dead_id"].append(rng.integers(0, N, size=k))
        out["dead_it"].append(rng.integers(0, 1000, size=k))
        out["dead_nc"].append(rng.integers(1, 50, size=k))
    return out


def cases():
    """name -> (problem name of tests/inputs.py or (kind, D), arguments).  See tests/test_gpu_merge.py."""
    out = {}
    rng = np.random.default_rng(7)
    # (a) run 2 is a copy of run 0: every value tied across two runs
    a = make(rng, [150, 170, 150, 140], 40, 3)
    for k in ("dead_logl", "dead_u", "dead_id", "dead_it", "dead_nc"):
        a[k][2] = a[k][0].copy()
    a["live_logl"][2], a["live_u"][2], a["live_it"][2] = a["live_logl"][0], a["live_u"][0], a["live_it"][0]
    out["a_copy"] = a
    # (b) a plateau of 7 equal dead values, equal values among the final live points
    b = make(rng, [120, 130, 110], 40, 3)
    b["dead_logl"][1][50:57] = b["dead_logl"][1][50]
    top = np.sort(b["live_logl"][1])
    b["live_logl"][1][[3, 17, 29]] = top[5]
    b["live_logl"][1][[8, 11]] = top[-1]
    b["dead_logl"][1] = np.minimum(b["dead_logl"][1], b["live_logl"][1].min())
    out["b_plateau"] = b
    # (c) unequal niter, one run with none
    out["c_ragged"] = make(rng, [300, 0, 45, 210], 40, 3)
    # (d) one run: the order is the identity
    out["d_single"] = make(rng, [200], 40, 3)
    # (e) scan carries and merge rounds across workgroups: M = 13 943 (not a multiple of 64 or 256)
    out["e_large"] = make(rng, [2000, 2917, 2411, 2650, 2465], 300, 7)
    # (f) rows wider than the register path
    out["f_wide"] = make(rng, [130, 120, 143], 90, 40)
    # (g) 2000 nats between the first and the last point
    out["g_span"] = make(rng, [400, 380, 391], 60, 3, span=2000.0)
    return out


def padded(rows, tail=(), dtype=np.float64):
    """Per-run lists as one (R, max niter, ...) array."""
    out = np.zeros((len(rows), max(1, max(len(r) for r in rows))) + tail, dtype=dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def host_merge(args, prior_transform=None):
    from dynesty_amd import ensemble
    D = args["live_u"].shape[2]
    return ensemble.merge_static_runs(padded(args["dead_logl"]), args["niter"], args["live_logl"],
                                      padded(args["dead_u"], (D,)), args["live_u"], prior_transform=prior_transform,
                                      dead_id=padded(args["dead_id"], dtype=np.int64),
                                      dead_it=padded(args["dead_it"], dtype=np.int64),
                                      dead_nc=padded(args["dead_nc"], dtype=np.int64), live_it=args["live_it"])
