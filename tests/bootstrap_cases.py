"""Run ensembles for the strand bootstrap's tests (tests/test_merge_bootstrap_cpu.py, tests/test_gpu_merge_bootstrap.py)
beyond those of tests/merge_cases.py, and what both tests share: the strands of a merged run and the golden one."""
import os

import numpy as np

import merge_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("golden", "a_copy", "b_plateau", "c_ragged", "d_single", "g_span", "h_bigplateau", "i_endties")
TIE_FREE = ("golden", "c_ragged", "d_single", "g_span")  # no two merged points of equal ln L
NCALLS = 4  # reference calls per case in tests/golden/merge_bootstrap.npz


def extra_cases():
    out = {}
    rng = np.random.default_rng(17)
    # (h) a tie group of more than a chunk: 2100 equal dead values of run 0 at a level L, and eleven of run 1's final
    # live points at L too (endpoints inside the group).  1500 points lie below L (200 of run 0, run 1's 350 dead ones,
    # 950 of run 2), so the group's expanded positions begin near 1500 +- 150 and straddle position 2048.
    h = merge_cases.make(rng, [2320, 350, 1000], 40, 3)
    L = h["dead_logl"][0][200]
    h["dead_logl"][0][200:2300] = L
    d1 = h["dead_logl"][1]
    h["dead_logl"][1] = L - 1e-3 - (d1.max() - d1)
    d2 = h["dead_logl"][2]
    d2[:950] -= max(0.0, d2[949] - (L - 1e-3))
    l1 = h["live_logl"][1]
    l1 = L + 0.01 + (l1 - l1.min())
    l1[[0, 3, 4, 9, 13, 20, 21, 22, 30, 35, 39]] = L
    h["live_logl"][1] = l1
    out["h_bigplateau"] = h
    # (i) all 40 final live points of one run equal
    i = merge_cases.make(rng, [150, 160, 140], 40, 3)
    i["live_logl"][1][:] = i["live_logl"][1].min()
    out["i_endties"] = i
    return out


def cases():
    out = {k: v for k, v in merge_cases.cases().items() if k in NAMES or k == "e_large"}
    out.update(extra_cases())
    return out


def golden_args(g):
    """The golden merged run's arguments with its per-point bookkeeping (tests/golden/merge.npz)."""
    return dict(niter=g["static/nit"], dead_logl=g["static/dead_l"], live_logl=g["static/live_l"], dead_u=g["static/dead_u"],
                live_u=g["static/live_u"], dead_id=g["static/dead_i"][0], dead_it=g["static/dead_i"][1],
                dead_nc=g["static/dead_i"][2], live_it=g["static/live_it"])


def host_run(name, g=None):
    """The host's merged run of a case, parameters included."""
    from dynesty_amd import ensemble
    if name != "golden":
        return merge_cases.host_merge(cases()[name], prior_transform=lambda u: 20.0 * u - 10.0)
    g = np.load(os.path.join(GOLD, "merge.npz")) if g is None else g
    a = golden_args(g)
    m = ensemble.merge_static_runs(a["dead_logl"], a["niter"], a["live_logl"], a["dead_u"], a["live_u"], dead_id=a["dead_id"],
                                   dead_it=a["dead_it"], dead_nc=a["dead_nc"], live_it=a["live_it"])
    np.testing.assert_array_equal(m.logl, g["ref/logl"])
    np.testing.assert_array_equal(m.samples_id, g["ref/samples_id"])
    m["samples"] = g["ref/samples"]
    return m


def strands(m):
    """(key run * nlive + slot per point, number of strands) of a merged run (host or downloaded)."""
    S = int(m["samples_n"][0])
    R = int(np.max(m["samples_run"])) + 1
    return np.asarray(m["samples_run"], dtype=np.int64) * (S // R) + np.asarray(m["samples_id"], dtype=np.int64), S


def multiplicities(draws, S):
    return np.bincount(np.asarray(draws, dtype=np.int64), minlength=S).astype(np.int32)
