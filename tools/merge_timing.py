"""Times the combiner leg of a merged ensemble: `run_ensemble_merged(merge='host')` against `merge='device'`.

Workload: 64 C2 runs (nlive 2000, K 512, parity RNG).  The two forms alternate, five of each (after one untimed
round of both); per form the tool reports median and range of
  - host: `run_ensemble_merged(merge='host')` end to end and nothing else -- the yardstick (the code path of
    merge_static_runs, unchanged) -- the ns_ensemble call inside it, and the combiner leg = end to end minus the loop;
  - device: `merge='device'` end to end INCLUDING mean_and_cov() and 10^5 equal-weight samples brought to the host,
    the ns_ensemble call inside it, the combiner leg = end to end minus the loop, and the part of that leg that is the
    merge alone (before the moments and the samples);
  - host_summaries: what the host form has no call for -- mean and covariance (GEMM form) and 10^5 systematic samples
    in NumPy from the host's merged run -- timed apart from the yardstick, as a like-for-like figure for the device
    form's last two calls.
One JSON line at the end.

    python tools/merge_timing.py [--runs 64] [--reps 5] [--device-only] [--check-hp]
(--device-only: for a kernel trace; --check-hp: ln Z of both forms against the long-double restatement of the same runs)
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


class Timed:
    """Backend pass-through that times ns_ensemble."""

    def __init__(self, ctx):
        self.ctx, self.loop = ctx, 0.0

    def __getattr__(self, name):
        return getattr(self.ctx, name)

    def ns_ensemble(self, *a, **kw):
        t = time.perf_counter()
        out = self.ctx.ns_ensemble(*a, **kw)
        self.loop = time.perf_counter() - t
        return out


def host_form(ensemble, prob, args, nsamp, be):
    t0 = time.perf_counter()
    m = ensemble.run_ensemble_merged(prob, merge='host', **args)
    t1 = time.perf_counter()
    loop = be.loop
    # not part of the yardstick: NumPy moments and systematic samples of the host's merged run
    w = m.importance_weights()
    ws = w.sum()
    mean = (w @ m.samples) / ws
    dx = m.samples - mean
    cov = ws / (ws ** 2 - (w ** 2).sum()) * ((dx * w[:, None]).T @ dx)
    rs = np.random.default_rng(1)
    c = np.cumsum(w)
    idx = np.searchsorted(c / c[-1], (rs.random() + np.arange(nsamp)) / nsamp, side='right')
    eq = m.samples[idx[rs.permutation(nsamp)]]
    t2 = time.perf_counter()
    r = m["runs"]
    return dict(total=t1 - t0, loop=loop, extra=t2 - t1), (m.niter, float(m.logz[-1]), mean, cov, eq,
                                                            (r["dead_logl"], r["niter"], r["live_logl"]))


def device_form(ensemble, prob, args, nsamp, be):
    t0 = time.perf_counter()
    d = ensemble.run_ensemble_merged(prob, merge='device', **args)
    t1 = time.perf_counter()
    loop = be.loop
    mean, cov = d.mean_and_cov()
    eq = d.resample_equal(nsamp, np.random.default_rng(1))
    t2 = time.perf_counter()
    out = d.niter, d.summary["logz"], mean, cov, eq
    d.release()
    return dict(total=t2 - t0, loop=loop, extra=t1 - t0 - loop), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=64)
    ap.add_argument("--nlive", type=int, default=2000)
    ap.add_argument("--queue", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--check-hp", action="store_true",
                    help="also ln Z of the same runs by the long-double restatement (tests/merge_hp_ref.py; minutes)")
    a = ap.parse_args()
    import inputs
    from dynesty_amd import _lib, backend, ensemble
    prob = inputs.problem("C2")
    be = Timed(_lib.Context(0))
    backend.set_backend(be)
    args = dict(runs=a.runs, nlive=a.nlive, queue_size=a.queue, entropy=(21,))
    forms = dict(device=device_form) if a.device_only else dict(host=host_form, device=device_form)
    t = {k: dict(total=[], loop=[], extra=[]) for k in forms}
    res = {}
    for rep in range(a.reps + 1):
        for name, fn in forms.items():
            dt, res[name] = fn(ensemble, prob, args, a.samples, be)
            if rep:  # the first round warms both forms up
                for k, v in dt.items():
                    t[name][k].append(v)
    out = dict(runs=a.runs, nlive=a.nlive, queue=a.queue, reps=a.reps, points=int(res["device"][0]))

    def stat(v):
        v = np.asarray(v)
        return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))
    for name in forms:
        tot, loop = np.array(t[name]["total"]), np.array(t[name]["loop"])
        out[f"{name}_total_s"], out[f"{name}_loop_s"], out[f"{name}_combiner_s"] = stat(tot), stat(loop), stat(tot - loop)
    out["device_merge_alone_s"] = stat(t["device"]["extra"])
    if "host" in forms:
        out["host_summaries_s"] = stat(t["host"]["extra"])
        out["logz_host"], out["logz_device"] = res["host"][1], res["device"][1]
        out["mean_max_diff"] = float(np.max(np.abs(res["host"][2] - res["device"][2])))
        out["cov_max_diff"] = float(np.max(np.abs(res["host"][3] - res["device"][3])))
        out["equal_samples_identical"] = bool(np.array_equal(res["host"][4], res["device"][4]))
    if a.check_hp and "host" in forms:
        import merge_hp_ref as hp
        print("long-double restatement ...", file=sys.stderr, flush=True)
        dl, nit, ll = res["host"][5]
        ref = hp.merge_hp([dl[i] for i in range(len(nit))], nit, ll)
        out["logz_long_double"] = float(ref["logz"][-1])
        out["logz_host_minus_ld"] = float(np.longdouble(res["host"][1]) - ref["logz"][-1])
        out["logz_device_minus_ld"] = float(np.longdouble(res["device"][1]) - ref["logz"][-1])
        out["logz_bound"] = float(hp.bounds(ref)["logz"][-1])
    M, D = out["points"], prob.ndim
    out["device_bytes_per_s"] = M * (16 * D + 80) / out["device_combiner_s"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
