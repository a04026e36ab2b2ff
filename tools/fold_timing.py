"""Times the fold leg of one dynamic batch: the strands of a finished `ns_batch` folded into the saved run.

Workload: a C2-shaped base (D = 25) of `--runs` drawn static runs of `--nlive` live points and `--dead` dead points each
(sorted ladders with slot ids, as tools/merged_errors.py --synthetic draws them: the fold reads values and rows, not how
they were sampled), merged on the device; one batch of `--strands` strands of `--nlive` live points and `--strand-dead`
dead points each, all above the base's value at a third of its length (logl_min), as a Context.ns_batch result dict.

  host    what run_dynamic(merge='host') spends between ns_batch and the stopping function: per strand strand_of (with the
          parameters of its points through problem_eval) and dynamic.merge_batch on the saved run held in NumPy.  This leg
          needs nothing of the fold and runs on a build without it.
  device  dynamic.fold_batch on the DeviceMergedRun: the strands' upload, dh_merged_fold, the summary's read-back.  The
          base is merged again before every repeat (a fold replaces it); that merge is timed apart.
  mirror  dynamic.merge_strands, the host's one-pass form (one sort, one integration), for the same batch.

Every leg runs once untimed, then `--reps` times; median and range per leg, one JSON line at the end.

    python tools/fold_timing.py [--form host|device|both] [--runs 16] [--nlive 2000] [--dead 83438] [--strands 16]
                                [--strand-dead 20000] [--reps 5] [--host-reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def drawn(rng, R, N, K, D, lo, hi):
    """R sequences of K dead and N live values on (lo, hi], flattening towards the top; rows random; slot ids."""
    all_l = np.sort(hi - (hi - lo) * rng.random((R, K + N)) ** 2, axis=1)
    live = np.stack([rng.permutation(all_l[r, K:]) for r in range(R)])
    return dict(niter=np.full(R, K, dtype=np.int64), dead_logl=np.ascontiguousarray(all_l[:, :K]), live_logl=live,
                dead_u=rng.random((R, K, D)), live_u=rng.random((R, N, D)),
                dead_id=rng.integers(0, N, size=(R, K)).astype(np.int32), dead_it=rng.integers(0, 1000, size=(R, K)).astype(np.int32),
                dead_nc=rng.integers(1, 50, size=(R, K)).astype(np.int32), live_it=rng.integers(0, 1000, size=(R, N)).astype(np.int32))


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="both", choices=("host", "device", "both"))
    ap.add_argument("--runs", type=int, default=16)
    ap.add_argument("--nlive", type=int, default=2000)
    ap.add_argument("--dead", type=int, default=83438)
    ap.add_argument("--strands", type=int, default=16)
    ap.add_argument("--strand-dead", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    import inputs
    from dynesty_amd import _lib, dynamic
    prob = inputs.problem("C2")
    D, N = prob.ndim, a.nlive
    ctx = _lib.Context(0)
    rng = np.random.default_rng(5)
    base = drawn(rng, a.runs, N, a.dead, D, -60.0, 0.0)
    allb = np.sort(np.concatenate([base["dead_logl"].ravel(), base["live_logl"].ravel()]))
    lmin, lmax = float(allb[len(allb) // 3]), 1.0
    out = drawn(rng, a.strands, N, a.strand_dead, D, lmin, 0.5)
    M, W = len(allb), a.strands * (a.strand_dead + N)
    res = dict(runs=a.runs, nlive=N, strands=a.strands, ndim=D, base_points=M, new_points=W, reps=a.reps, host_reps=a.host_reps)

    def merge_base():
        t = time.perf_counter()
        d = ctx.merge_runs(prob, **base)
        return d, time.perf_counter() - t
    if a.form in ("host", "both"):
        d, _ = merge_base()
        m = d.to_merged_run()
        d.release()
        # one run from here on, as run_dynamic makes it
        m["samples_id"] = np.asarray(m["samples_run"], dtype=np.int64) * N + np.asarray(m["samples_id"])
        m["samples_run"] = np.zeros(len(m["logl"]), dtype=np.int64)

        def ptform(u):
            return ctx.problem_eval(prob, u)[0]
        t_host, last = [], None
        for rep in range(a.host_reps + 1):
            t = time.perf_counter()
            cur = m
            for r in range(a.strands):
                cur = dynamic.merge_batch(cur, dynamic.strand_of(out, r, N, prior_transform=ptform), lmin, lmax)
            dt = time.perf_counter() - t
            if rep:
                t_host.append(dt)
            last = cur
        res["host_fold_s"] = stat(t_host)
        res["host_logz"] = float(last["logz"][-1])
        if hasattr(dynamic, "merge_strands"):
            t_mirror = []
            for rep in range(a.host_reps + 1):
                t = time.perf_counter()
                one = dynamic.merge_strands(m, [dynamic.strand_of(out, r, N, prior_transform=ptform) for r in range(a.strands)],
                                            lmin, lmax)
                dt = time.perf_counter() - t
                if rep:
                    t_mirror.append(dt)
            res["mirror_fold_s"] = stat(t_mirror)
            res["mirror_logz_minus_host"] = float(one["logz"][-1] - last["logz"][-1])
    if a.form in ("device", "both"):
        if not hasattr(dynamic, "fold_batch"):
            raise SystemExit("this build has no device fold (dynamic.fold_batch): --form host")
        t_fold, t_merge = [], []
        for rep in range(a.reps + 1):
            d, dt_merge = merge_base()
            t = time.perf_counter()
            f = dynamic.fold_batch(d, out, N, lmin, lmax)
            dt = time.perf_counter() - t
            if rep:
                t_fold.append(dt)
                t_merge.append(dt_merge)
            res["device_logz"] = f.summary["logz"]
            assert f.niter == M + W
            f.release()
        res["device_fold_s"] = stat(t_fold)
        res["device_merge_runs_s"] = stat(t_merge)  # the static merge of the base, upload included
        res["fold_ns_per_point"] = 1e9 * res["device_fold_s"]["median"] / (M + W)
        res["row_move_bytes"] = (M + W) * 2 * 16 * D  # mf_rows: u and v of every point read and written
        if "host_fold_s" in res:
            res["host_over_device"] = res["host_fold_s"]["median"] / res["device_fold_s"]["median"]
            res["device_logz_minus_host"] = res["device_logz"] - res["host_logz"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
