"""Times the statistical errors of a merged run: realizations of the prior volumes on the device against the route
they replace, download + NumPy.

Workload: 64 C2 runs (nlive 2000, K 512), merged on the device (`run_ensemble_merged(merge='device')`), once; with
--synthetic drawn runs of the same size (tests/merge_cases.make) merged by Context.merge_runs instead, which is what a
kernel trace wants.  Then, alternating the two sides in one process, `--reps` of each after one untimed round of both:
  device  logz_realizations(nreal) for nreal in 1, 64, 256, without and with means (each call ends in a stream
          synchronisation and the read-back of its results); reweight(); jitter_run()
  host    what there was before: the download of logl, samples_n and samples (timed apart), then the package's own
          NumPy form (ensemble.MergedRun.logz_realizations) on --host-real realizations, scaled to one; and, where a
          copy of the reference is importable, utils.jitter_run(approx=True) per realization
With --bootstrap the strand bootstrap too (the synthetic runs then carry slot ids):
  device  bootstrap_realizations(nboot) for nboot in 1, 64, 256, without and with jitter and means; resample_run()
  host    the download of logl, samples_run, samples_id, final and samples (timed apart), then the package's NumPy form
          (ensemble.MergedRun.bootstrap_realizations) on --host-boot bootstraps, scaled to one
and `bootstrap_over_realization`: one bootstrap without means over one realization of the same merged run, each computed
alone (nboot = 1 over nreal = 1), which is how a bootstrap is always computed (M' differs between bootstraps);
`bootstrap_over_batched_realization`: per bootstrap of 64 over per realization of 64, where the realizations share
their loads in tiles of 4.
One JSON line at the end.  `f64_fraction_*`: the fp64 vector instructions of a call over the chip's measured rate
(58.7 TFLOP/s = 29.35e12 v_fma_f64 lanes per second), with the instructions per point and realization
counted in the kernels' code on the jitter path (me_step_sums 93, me_integrate 287: all v_*_f64 of the unrolled 8-point
body / 8; with means 32 more, the mean sums' v_fma_f64 per point over a tile of 32 columns).

    python tools/merged_errors.py [--runs 64] [--reps 5] [--host-real 8] [--device-only] [--synthetic] [--bootstrap]
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

F64_PER_POINT = 93 + 287
F64_PER_POINT_MEANS = F64_PER_POINT + 32
F64_LANES_PER_S = 29.35e12


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
    ap.add_argument("--host-real", type=int, default=8, help="realizations of the NumPy form per repetition")
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--synthetic", action="store_true", help="drawn runs of --niter dead points each, no sampling")
    ap.add_argument("--niter", type=int, default=83438)
    ap.add_argument("--bootstrap", action="store_true", help="time the strand bootstrap too")
    ap.add_argument("--host-boot", type=int, default=2, help="bootstraps of the NumPy form per repetition")
    a = ap.parse_args()
    import inputs
    from dynesty_amd import _lib, backend, ensemble
    prob = inputs.problem("C2")
    ctx = _lib.Context(0)
    backend.set_backend(ctx)
    if a.synthetic:
        import merge_cases
        args = merge_cases.make(np.random.default_rng(1), [a.niter] * a.runs, a.nlive, prob.ndim)
        pt = {k: args[k] for k in ("dead_id", "dead_it", "dead_nc", "live_it")} if a.bootstrap else {}
        d = ctx.merge_runs(prob, args["niter"], args["dead_logl"], args["live_logl"], args["dead_u"], args["live_u"], **pt)
        del args
    else:
        d = ensemble.run_ensemble_merged(prob, a.runs, merge='device', nlive=a.nlive, queue_size=a.queue, entropy=(21,))
    M, D = d.niter, prob.ndim
    rng = np.random.default_rng(2)
    logp_new = d.field("logl") + 0.3 * rng.standard_normal(M)
    dev = {}
    for n in (1, 64, 256):
        dev[f"realize_{n}"] = lambda n=n: d.logz_realizations(n, seed=1)
        dev[f"realize_{n}_means"] = lambda n=n: d.logz_realizations(n, seed=1, means=True)
    dev["reweight"] = lambda: d.reweight(logp_new)
    dev["jitter_run"] = lambda: d.jitter_run(seed=1, real=0)
    if a.bootstrap:
        for n in (1, 64, 256):
            dev[f"bootstrap_{n}"] = lambda n=n: d.bootstrap_realizations(n, seed=1)
            dev[f"bootstrap_{n}_jitter"] = lambda n=n: d.bootstrap_realizations(n, seed=1, jitter=True)
            dev[f"bootstrap_{n}_means"] = lambda n=n: d.bootstrap_realizations(n, seed=1, means=True)
            dev[f"bootstrap_{n}_jitter_means"] = lambda n=n: d.bootstrap_realizations(n, seed=1, jitter=True, means=True)
        dev["resample_run"] = lambda: d.resample_run(seed=1, boot=0)
    t = {f"device_{k}": [] for k in dev}
    t.update(download=[], host_realize=[], host_realize_means=[], reference_jitter_approx=[], download_bootstrap=[],
             host_bootstrap=[], host_bootstrap_jitter=[])
    res = {}
    try:
        from dynesty import utils as dyu
    except Exception:
        dyu = None
    for rep in range(a.reps + 1):
        for k, fn in dev.items():
            ctx.sync()
            dt, res[k] = timed(fn)
            if rep:
                t[f"device_{k}"].append(dt)
        if a.device_only:
            continue
        dt, (logl, n, x) = timed(lambda: (d.field("logl"), d.field("samples_n"), d.field("samples")))
        if rep:
            t["download"].append(dt)
        if rep == 0 or rep > a.host_reps:  # (NumPy needs no warm-up)
            continue
        host = ensemble.MergedRun(niter=M, logl=logl, samples_n=n, samples=x)
        dt, res["host"] = timed(lambda: host.logz_realizations(a.host_real, seed=1))
        t["host_realize"].append(dt / a.host_real)
        dt, res["host_means"] = timed(lambda: host.logz_realizations(a.host_real, seed=1, means=True))
        t["host_realize_means"].append(dt / a.host_real)
        if a.bootstrap:
            dt, f = timed(lambda: {k: d.field(k) for k in ("logl", "samples_run", "samples_id", "final", "samples", "samples_n")})
            t["download_bootstrap"].append(dt)
            hb = ensemble.MergedRun(niter=M, **{k: v for k, v in f.items() if k != "final"})
            dt, res["host_boot"] = timed(lambda: hb.bootstrap_realizations(a.host_boot, seed=1))
            t["host_bootstrap"].append(dt / a.host_boot)
            dt, _ = timed(lambda: hb.bootstrap_realizations(a.host_boot, seed=1, jitter=True))
            t["host_bootstrap_jitter"].append(dt / a.host_boot)
        if dyu is not None:
            full = d.to_merged_run()
            r = dyu.Results({k: full[k] for k in ("samples_u", "samples_id", "samples_it", "logl", "samples", "samples_n",
                                                  "logvol", "logwt", "logz", "logzerr", "information", "ncall")})
            dt, _ = timed(lambda: dyu.jitter_run(r, rstate=np.random.default_rng(0), approx=True))
            t["reference_jitter_approx"].append(dt)
    out = dict(runs=a.runs, nlive=a.nlive, points=M, ndim=D, reps=a.reps, synthetic=bool(a.synthetic))
    for k, v in t.items():
        if v:
            out[k + "_s"] = stat(v)
    for n in (64, 256):
        for sfx in ("", "_means"):
            s = out[f"device_realize_{n}{sfx}_s"]["median"]
            out[f"f64_fraction_{n}{sfx}"] = (F64_PER_POINT_MEANS if sfx else F64_PER_POINT) * M * n / s / F64_LANES_PER_S
            out[f"point_realizations_per_s_{n}{sfx}"] = M * n / s
    if not a.device_only and "host" in res:
        out["host_real"] = a.host_real
        out["logz_max_diff_device_host"] = float(np.max(np.abs(res["realize_64"]["logz"][:a.host_real] - res["host"]["logz"])))
        out["mean_max_diff_device_host"] = float(np.max(np.abs(res["realize_64_means"]["mean"][:a.host_real] - res["host_means"]["mean"])))
        for n in (64, 256):
            out[f"download_over_device_{n}"] = out["download_s"]["median"] / out[f"device_realize_{n}_s"]["median"]
            out[f"host_route_over_device_{n}"] = (out["download_s"]["median"] + n * out["host_realize_s"]["median"]) / \
                out[f"device_realize_{n}_s"]["median"]
    if a.bootstrap:
        out["bootstrap_over_realization"] = out["device_bootstrap_1_s"]["median"] / out["device_realize_1_s"]["median"]
        out["bootstrap_jitter_over_realization"] = out["device_bootstrap_1_jitter_s"]["median"] / out["device_realize_1_s"]["median"]
        out["bootstrap_over_batched_realization"] = out["device_bootstrap_64_s"]["median"] / out["device_realize_64_s"]["median"]
        bz = res["bootstrap_256"]["logz"]
        out["bootstrap_logz_mean_sd_256"] = [float(bz.mean()), float(bz.std(ddof=1))]
        out["bootstrap_npoints_min_max_256"] = [int(res["bootstrap_256"]["npoints"].min()), int(res["bootstrap_256"]["npoints"].max())]
        if "host_boot" in res:
            out["host_boot"] = a.host_boot
            out["logz_max_diff_device_host_bootstrap"] = float(np.max(np.abs(res["bootstrap_64"]["logz"][:a.host_boot] - res["host_boot"]["logz"])))
            for n in (1, 64, 256):
                out[f"host_bootstrap_route_over_device_{n}"] = (out["download_bootstrap_s"]["median"] + n * out["host_bootstrap_s"]["median"]) / \
                    out[f"device_bootstrap_{n}_s"]["median"]
    lz = res["realize_256"]["logz"]
    out["logz_mean_sd_256"] = [float(lz.mean()), float(lz.std(ddof=1))]
    out["summary"] = dict(logz=d.summary["logz"], logzerr=d.summary["logzerr"])
    d.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
