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
With --dynamic the run-level analysis of DESIGN section 3.8.4 in place of the lists above (the synthetic runs carry slot
ids): kld_realizations(256) beside logz_realizations(256) without means, kld_realizations(64) of both bootstrap modes
beside bootstrap_realizations(64), kld_error(), weight_function() without and with its three weight arrays; and the route
weight_function replaces: the download of logl, logz, logvol, logwt and samples_n plus the NumPy form.
One JSON line at the end.  `f64_fraction_*`: the fp64 vector instructions of a call over the chip's measured rate
(58.7 TFLOP/s = 29.35e12 v_fma_f64 lanes per second), with the instructions per point and realization
counted in the kernels' code on the jitter path (me_step_sums 93, me_integrate 287: all v_*_f64 of the unrolled 8-point
body / 8; with means 32 more, the mean sums' v_fma_f64 per point over a tile of 32 columns).

    python tools/merged_errors.py [--runs 64] [--reps 5] [--host-real 8] [--device-only] [--synthetic] [--bootstrap]
                                    [--dynamic]
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
    ap.add_argument("--dynamic", action="store_true", help="time the divergence and the weight function instead")
    a = ap.parse_args()
    import inputs
    from dynesty_amd import _lib, backend, ensemble
    prob = inputs.problem("C2")
    ctx = _lib.Context(0)
    backend.set_backend(ctx)
    if a.synthetic:
        import merge_cases
        args = merge_cases.make(np.random.default_rng(1), [a.niter] * a.runs, a.nlive, prob.ndim)
        pt = {k: args[k] for k in ("dead_id", "dead_it", "dead_nc", "live_it")} if a.bootstrap or a.dynamic else {}
        d = ctx.merge_runs(prob, args["niter"], args["dead_logl"], args["live_logl"], args["dead_u"], args["live_u"], **pt)
        del args
    else:
        d = ensemble.run_ensemble_merged(prob, a.runs, merge='device', nlive=a.nlive, queue_size=a.queue, entropy=(21,))
    M, D = d.niter, prob.ndim
    rng = np.random.default_rng(2)
    logp_new = d.field("logl") + 0.3 * rng.standard_normal(M)
    if a.dynamic:
        return dynamic(a, ctx, d)
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


def dynamic(a, ctx, d):
    from dynesty_amd import ensemble
    dev = dict(realize_256=lambda: d.logz_realizations(256, seed=1), kld_256=lambda: d.kld_realizations(256, seed=1),
               bootstrap_64=lambda: d.bootstrap_realizations(64, seed=1),
               kld_64_resample=lambda: d.kld_realizations(64, seed=1, error="resample"),
               bootstrap_64_jitter=lambda: d.bootstrap_realizations(64, seed=1, jitter=True),
               kld_64_simulate=lambda: d.kld_realizations(64, seed=1, error="simulate"),
               kld_error=lambda: d.kld_error(seed=1, index=0), weight_function=lambda: d.weight_function(),
               weight_function_weights=lambda: d.weight_function(return_weights=True))
    t = {f"device_{k}": [] for k in dev}
    t.update(download_weight_function=[], host_weight_function=[])
    res = {}
    for rep in range(a.reps + 1):
        for k, fn in dev.items():
            ctx.sync()
            dt, res[k] = timed(fn)
            if rep:
                t[f"device_{k}"].append(dt)
        if a.device_only or rep == 0:
            continue
        dt, f = timed(lambda: {k: d.field(k) for k in ("logl", "logz", "logvol", "logwt", "samples_n")})
        t["download_weight_function"].append(dt)
        host = ensemble.MergedRun(niter=d.niter, **f)
        dt, res["host_wf"] = timed(lambda: host.weight_function())
        t["host_weight_function"].append(dt)
    out = dict(runs=a.runs, nlive=a.nlive, points=d.niter, reps=a.reps, synthetic=bool(a.synthetic), dynamic=True)
    for k, v in t.items():
        if v:
            out[k + "_s"] = stat(v)
    med = lambda k: out[f"device_{k}_s"]["median"]  # noqa: E731
    out["kld_256_over_realize_256"] = med("kld_256") / med("realize_256")
    out["kld_64_resample_over_bootstrap_64"] = med("kld_64_resample") / med("bootstrap_64")
    out["kld_64_simulate_over_bootstrap_64_jitter"] = med("kld_64_simulate") / med("bootstrap_64_jitter")
    if "host_wf" in res:
        assert res["host_wf"] == res["weight_function"], (res["host_wf"], res["weight_function"])
        out["host_route_over_device_weight_function"] = (out["download_weight_function_s"]["median"] +
                                                          out["host_weight_function_s"]["median"]) / med("weight_function")
    k = res["kld_256"]["kld"]
    out["kld_mean_sd_256"] = [float(k.mean()), float(k.std(ddof=1))]
    out["logl_bounds"] = [float(x) for x in res["weight_function"]]
    d.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
