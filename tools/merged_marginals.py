"""Times credible intervals and corner-plot histograms of a merged run: on the device against download + NumPy.

Workload: 64 C2 runs (nlive 2000, K 512), merged on the device (`run_ensemble_merged(merge='device')`), once.  Then,
alternating the two sides in one process, `--reps` of each after one untimed round of both:
  (a) quantile([0.025, 0.5, 0.975]) over all 25 columns;
  (b) histogram of all columns at 50 bins (range: the column's [min, max]);
  (c) histogram2d of all 300 pairs at 50 x 50 bins.
Device side: the DeviceMergedRun methods (each ends in a stream synchronisation and a read-back of the results).
Host side: what there was before them: field("samples") + importance_weights() (the download, timed apart), then
the same three methods of ensemble.MergedRun in NumPy (timed apart; --host-reps of them, they take seconds).
One JSON line at the end, with the bytes per second of the quantile call against what its passes must read:
passes x M x (8 D + 8), passes = 2 (extremes, last point) + 12 (digits) + 1 (successor).

    python tools/merged_marginals.py [--runs 64] [--reps 5] [--host-reps 1] [--host-pairs 300] [--device-only]
(--device-only: for a kernel trace)
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

Q = [0.025, 0.5, 0.975]
PASSES = 15


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=64)
    ap.add_argument("--nlive", type=int, default=2000)
    ap.add_argument("--queue", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-pairs", type=int, default=300, help="pairs of the NumPy histogram2d (about 0.5 s each)")
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    import inputs
    from dynesty_amd import _lib, backend, ensemble
    prob = inputs.problem("C2")
    ctx = _lib.Context(0)
    backend.set_backend(ctx)
    d = ensemble.run_ensemble_merged(prob, a.runs, merge='device', nlive=a.nlive, queue_size=a.queue, entropy=(21,))
    D = prob.ndim
    pairs = [(i, j) for i in range(D) for j in range(i + 1, D)]
    dev = dict(quantile=lambda: d.quantile(Q), histogram=lambda: d.histogram(bins=a.bins),
               histogram2d=lambda: d.histogram2d(pairs, bins=a.bins))
    t = {f"device_{k}": [] for k in dev}
    t.update(download=[], host_quantile=[], host_histogram=[], host_histogram2d=[])
    res = {}
    for rep in range(a.reps + 1):
        for k, fn in dev.items():
            ctx.sync()
            dt, res[k] = timed(fn)
            if rep:
                t[f"device_{k}"].append(dt)
        if a.device_only:
            continue
        dt, (x, w) = timed(lambda: (d.field("samples"), d.importance_weights()))
        if rep:
            t["download"].append(dt)
        if rep == 0 or rep > a.host_reps:  # (NumPy needs no warm-up)
            continue
        host = ensemble.MergedRun(niter=d.niter, samples=x)
        host.importance_weights = lambda: w  # the device's own weights: the two sides work on the same numbers
        for k, fn in (("quantile", lambda: host.quantile(Q)), ("histogram", lambda: host.histogram(bins=a.bins)),
                      ("histogram2d", lambda: host.histogram2d(pairs[:a.host_pairs], bins=a.bins))):
            dt, res["host_" + k] = timed(fn)
            t["host_" + k].append(dt)
    M = d.niter
    out = dict(runs=a.runs, nlive=a.nlive, points=M, ndim=D, bins=a.bins, reps=a.reps)
    for k, v in t.items():
        if v:
            out[k + "_s"] = stat(v)
    must = PASSES * M * (8 * D + 8)
    out["quantile_pass_bytes"] = must
    out["quantile_bytes_per_s"] = must / out["device_quantile_s"]["median"]
    if not a.device_only and "host_quantile" in res:
        out["quantile_max_diff"] = float(np.max(np.abs(res["quantile"] - res["host_quantile"])))
        out["histogram_max_diff"] = float(np.max(np.abs(res["histogram"][0] - res["host_histogram"][0])))
        out["host_pairs"] = min(a.host_pairs, len(pairs))
        out["histogram2d_max_diff"] = float(np.max(np.abs(res["histogram2d"][0][:a.host_pairs] - res["host_histogram2d"][0])))
        dev_s = sum(out[f"device_{k}_s"]["median"] for k in dev)
        out["device_all_three_s"] = dev_s
        out["download_over_device_all_three"] = out["download_s"]["median"] / dev_s
    d.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
