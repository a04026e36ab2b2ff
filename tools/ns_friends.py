"""Friends bounds in the resident loop: R runs of the eggbox in 2-D (nlive 500, dlogz 0.01, sample='unif' with the
reference's defaults, enlarge 1 / bootstrap 5) through ns_ensemble at queue size K; one warm-up ensemble, then one
timed ensemble; prints one JSON line.

usage: python tools/ns_friends.py [runs=64] [bound=balls|cubes] [K=64]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynesty_amd import _lib, problems  # noqa: E402

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 64
kind = sys.argv[2] if len(sys.argv) > 2 else "balls"
K = int(sys.argv[3]) if len(sys.argv) > 3 else 64
ctx = _lib.Context(0)
prob = problems.eggbox(2)
ctx.ns_ensemble(prob, runs, 500, K, bound=kind, sample="unif", entropy=[20], dlogz=0.01)  # warm-up
t = time.perf_counter()
r = ctx.ns_ensemble(prob, runs, 500, K, bound=kind, sample="unif", entropy=[21], dlogz=0.01)
dt = time.perf_counter() - t
lz = r["logz"]
print(json.dumps(dict(runs=runs, bound=kind, K=K, secs=round(dt, 4), mean_logz=float(lz.mean()),
                      se=float(lz.std(ddof=1) / np.sqrt(runs)), truth=prob.logz_truth,
                      status_ok=int((r["status"] == 0).sum()), niter=float(r["niter"].mean()),
                      ncall=float(r["ncall"].mean()), nbound=float(r["nbound"].mean()), nfills=int(r["nfills"]))))
