"""Synthetic bases and batches for the fold's tests (tests/test_fold_cpu.py, tests/test_gpu_merged_fold.py): a base that
is a merge of static runs (tests/merge_cases.py's drawn ladders) and R strands above a lower bound, at the smallest sizes
where the device's kernels can go wrong -- M + W beyond one scan chunk of 2048 points, plateaus of equal ln L laid
across merged positions 2047 / 2048 and across a multiple of 256, base and strand points mixed in them, base values
equal to logl_min, a strand wholly above the base."""
import numpy as np

import merge_cases


def _flat(parts):
    """Every value of every sequence with where it lives: (values, [(part, 'dead' | 'live', run, index), ..])."""
    vals, where = [], []
    for pi, a in enumerate(parts):
        for r in range(len(a["niter"])):
            for i, x in enumerate(a["dead_logl"][r]):
                vals.append(x)
                where.append((pi, "dead_logl", r, i))
            for i, x in enumerate(a["live_logl"][r]):
                vals.append(x)
                where.append((pi, "live_logl", r, i))
    return np.array(vals), where


def _plateau(parts, lo, hi, need_mixed):
    """Merged positions [lo, hi) all take the value at `lo` (lowering a value to one that its run's earlier points do
    not exceed keeps every sequence non-decreasing and every final live value above its run's dead ones)."""
    vals, where = _flat(parts)
    order = np.argsort(vals, kind="stable")
    x = vals[order[lo]]
    kinds = set()
    for f in order[lo:hi]:
        pi, key, r, i = where[f]
        parts[pi][key][r][i] = x
        kinds.add(pi)
    assert not need_mixed or kinds == {0, 1}, (lo, hi, kinds)
    return x


def make(seed, D, R, base_niters, base_nlive, strand_niters, strand_nlive, above=False, plateaus=(), min_pos=None, pt=True):
    """Returns (base arguments of Context.merge_runs, strand arguments of Context.merged_fold as one dict, logl_min,
    logl_max).  min_pos: the merged position (all base points below it) whose value becomes logl_min, with the two base
    points before it set equal to it.  plateaus: (lo, hi) merged positions to make equal, base and strand points both
    inside.  above: the last strand lies wholly above the base's last point."""
    rng = np.random.default_rng(seed)
    base = merge_cases.make(rng, base_niters, base_nlive, D)
    new = merge_cases.make(rng, strand_niters, strand_nlive, D)
    allb = np.sort(np.concatenate([np.concatenate(base["dead_logl"]), base["live_logl"].ravel()]))
    logl_min = float(allb[min_pos])
    for r in range(R):  # the ladder on (-30, 0] squeezed into (logl_min, 0]; the strand above onto (1, 31]
        up = above and r == R - 1
        f = (lambda x: x + 31.0) if up else (lambda x: logl_min + (x + 30.0) / 30.0 * (0.0 - logl_min) * 0.999 + 1e-3)
        new["dead_logl"][r] = f(new["dead_logl"][r])
        new["live_logl"][r] = f(new["live_logl"][r])
    parts = [base, new]
    # base values equal to logl_min: positions min_pos - 2 .. min_pos hold base points only (the strands lie above)
    assert _plateau(parts, min_pos - 2, min_pos + 1, False) <= logl_min
    logl_min = float(np.sort(np.concatenate([np.concatenate(base["dead_logl"]), base["live_logl"].ravel()]))[min_pos])
    for lo, hi in plateaus:
        assert lo > min_pos + 1
        assert _plateau(parts, lo, hi, True) > logl_min
    if not pt:
        for a in parts:
            for k in ("dead_id", "dead_it", "dead_nc", "live_it"):
                a.pop(k)
    return base, new, logl_min, 40.0


def host_strands(new, nlive, prior_transform):
    """The strands as dynamic.merge_strands takes them (dynamic.strand_of of the padded arrays)."""
    from dynesty_amd import dynamic
    D = new["live_u"].shape[2]
    out = dict(niter=new["niter"], dead_logl=merge_cases.padded(new["dead_logl"]), live_logl=new["live_logl"],
               dead_u=merge_cases.padded(new["dead_u"], (D,)), live_u=new["live_u"])
    R = len(new["niter"])
    if "dead_id" in new:
        out.update(dead_id=merge_cases.padded(new["dead_id"], dtype=np.int64), dead_it=merge_cases.padded(new["dead_it"], dtype=np.int64),
                   dead_nc=merge_cases.padded(new["dead_nc"], dtype=np.int64), live_it=new["live_it"])
    else:  # (strand_of wants the bookkeeping: zeros, dropped again by the caller's comparison)
        z = np.zeros(out["dead_logl"].shape, dtype=np.int64)
        out.update(dead_id=z, dead_it=z, dead_nc=z, live_it=np.zeros((R, nlive), dtype=np.int64))
    return [dynamic.strand_of(out, r, nlive, prior_transform=prior_transform) for r in range(R)]


# name -> arguments of make(): the device test's cases (the CPU test holds the generator to what it promises)
CASES = dict(
    one_strand_d1=dict(seed=1, D=1, R=1, base_niters=[940, 950, 930], base_nlive=60, strand_niters=[1440], strand_nlive=60,
                       plateaus=((2044, 2051), (2300, 2308)), min_pos=900),
    three_strands_d33=dict(seed=2, D=33, R=3, base_niters=[940, 950, 930], base_nlive=60, strand_niters=[500, 410, 380],
                           strand_nlive=70, above=True, plateaus=((2045, 2050), (2555, 2563)), min_pos=1000),
    five_strands_no_pt=dict(seed=3, D=1, R=5, base_niters=[940, 950, 930], base_nlive=60, strand_niters=[300, 0, 280, 310, 260],
                            strand_nlive=70, plateaus=((2040, 2052), (2810, 2820)), min_pos=700, pt=False),
    more_new_than_base=dict(seed=4, D=33, R=3, base_niters=[100, 110, 90], base_nlive=20, strand_niters=[700, 720, 690],
                            strand_nlive=60, plateaus=((2046, 2050), (1020, 1030)), min_pos=60),
)
