"""Times the seed step of one dynamic batch both ways on the same DeviceMergedRun.

Workload: a C2 base (D = 25) merged on the device -- the 64-run ensemble of tools/merged_errors.py
(`run_ensemble_merged(merge='device')`, nlive 2000, K 512), or with --synthetic `--runs` drawn static runs of `--nlive`
live and `--dead` dead points each (tools/fold_timing.py's ladders: the seed step reads values and rows, not how they
were sampled) -- and the bounds its weight function asks for; one batch of `--strands` strands of `--nlive-batch` seeds.

  host    what run_dynamic(seeds='host', merge='device') does per batch: the logl and logvol columns down
          (dynamic._base_columns), dynamic.batch_seed per strand on one Generator, the chosen rows by a gather.  This leg
          needs nothing of the device's choice and runs on a build without it.
  device  DeviceMergedRun.batch_seeds(): dh_merged_batch_seed for all strands; the indices, the chosen rows gathered on
          the device and their ln L come back.

Every leg runs once untimed, then `--host-reps` / `--reps` times; median and range per leg, one JSON line at the end.

    python tools/seed_timing.py [--form host|device|both] [--synthetic] [--runs 64] [--nlive 2000] [--dead 83438]
                                [--strands 64] [--nlive-batch 500] [--reps 7] [--host-reps 2]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stat(v):
    v = np.asarray(v)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="both", choices=("host", "device", "both"))
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--runs", type=int, default=64)
    ap.add_argument("--nlive", type=int, default=2000)
    ap.add_argument("--queue", type=int, default=512)
    ap.add_argument("--dead", type=int, default=83438)
    ap.add_argument("--strands", type=int, default=64)
    ap.add_argument("--nlive-batch", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=2)
    a = ap.parse_args()
    import inputs
    from dynesty_amd import _lib, backend, dynamic, ensemble
    prob = inputs.problem("C2")
    ctx = _lib.Context(0)
    t = time.perf_counter()
    if a.synthetic:
        from fold_timing import drawn
        d = ctx.merge_runs(prob, **drawn(np.random.default_rng(5), a.runs, a.nlive, a.dead, prob.ndim, -60.0, 0.0))
    else:
        backend.set_backend(ctx)
        d = ensemble.run_ensemble_merged(prob, a.runs, merge='device', nlive=a.nlive, queue_size=a.queue, entropy=(21,))
        d.pop("runs")
    bounds = d.weight_function(pfrac=0.8)
    S, k = a.strands, a.nlive_batch
    res = dict(base="synthetic" if a.synthetic else "C2 ensemble", runs=a.runs, nlive=a.nlive, ndim=prob.ndim,
               base_points=d.niter, base_seconds=time.perf_counter() - t, bounds=[float(x) for x in bounds], strands=S,
               nlive_batch=k, reps=a.reps, host_reps=a.host_reps)
    if a.form in ("host", "both"):
        t_host, parts = [], None
        for rep in range(a.host_reps + 1):
            rstate = np.random.default_rng(7)
            t0 = time.perf_counter()
            cols = dynamic._base_columns(d)
            t1 = time.perf_counter()
            picked = [dynamic.batch_seed(d, bounds, k, rstate, columns=cols) for _ in range(S)]
            t2 = time.perf_counter()
            if not picked[0]["prior"]:
                pick = np.concatenate([s["idx"] for s in picked])
                d.gather(pick, "samples_u")
                cols[0][pick]
            t3 = time.perf_counter()
            if rep:
                t_host.append(t3 - t0)
                parts = dict(columns_s=t1 - t0, batch_seed_s=t2 - t1, gather_s=t3 - t2)
        res["host_seed_s"] = stat(t_host)
        res["host_parts_last_rep"] = parts
        res["host_prior"] = bool(picked[0]["prior"])
        res["host_vol_idx"] = int(picked[0]["vol_idx"])
    if a.form in ("device", "both"):
        if not hasattr(d, "batch_seeds"):
            raise SystemExit("this build has no device choice (DeviceMergedRun.batch_seeds): --form host")
        t_dev, s = [], None
        for rep in range(a.reps + 1):
            ctx.sync()
            t0 = time.perf_counter()
            s = d.batch_seeds(bounds[0], k, S, 1000 + rep)
            dt = time.perf_counter() - t0
            if rep:
                t_dev.append(dt)
        res["device_seed_s"] = stat(t_dev)
        res["device_reps_ms"] = [round(1e3 * x, 3) for x in t_dev]
        res.update(passes=s["passes"], lo=s["lo"], count=s["count"], n_pos=s["n_pos"], device_prior=bool(s["prior"]),
                   device_vol_idx=s["vol_idx"], row_bytes=S * k * (prob.ndim + 1) * 8)
        if "host_seed_s" in res:
            res["host_over_device"] = res["host_seed_s"]["median"] / res["device_seed_s"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
