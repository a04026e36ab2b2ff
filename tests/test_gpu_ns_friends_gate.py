"""The eggbox in 2-D with RadFriends / SupFriends bounds and the uniform sampler (the reference's defaults: enlarge 1,
bootstrap 5) through the device-resident loop, 64 runs per bound, against 32 runs of the real reference at the same
queue size (K = 64) and serial (tests/golden/friends_logz_ref.json by tools/ref_friends_runs.py), with the checks of
test_gpu_logz_gate.py::test_c1_device_unif_ensemble_vs_reference_ensemble.  The call count is the check that the radius
(bootstrap replicas) and the 1/q rule make the union of shapes as tight as the reference's."""
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TRUTH = 235.856


@pytest.fixture(scope="module")
def ctx():
    from dynesty_amd import _lib
    return _lib.Context(0)


def bound(se_a, se_b):
    return max(0.05, 3.0 * math.sqrt(se_a * se_a + se_b * se_b))


@pytest.mark.parametrize("kind,K", [("balls", 64), ("cubes", 64), ("balls", 1), ("cubes", 1)])
def test_friends_device_ensemble_vs_reference_ensemble(ctx, kind, K):
    from dynesty_amd import problems
    g = json.load(open(os.path.join(GOLD, "friends_logz_ref.json")))["ensembles"]
    ref = g[f"{kind}_K{K}"]
    r = ctx.ns_ensemble(problems.eggbox(2), 64, 500, K, bound=kind, sample="unif", entropy=[2026, 3, K], dlogz=0.01)
    assert np.all(r["status"] == 0)
    lz = r["logz"]
    mean, se = lz.mean(), lz.std(ddof=1) / math.sqrt(len(lz))
    assert abs(mean - ref["mean"]) < bound(se, ref["se"]), (mean, se, ref["mean"], ref["se"])
    assert 0.6 < lz.std(ddof=1) / ref["std"] < 1.6
    assert abs(r["logzerr"].mean() - ref["mean_logzerr"]) < 0.01
    assert abs(r["niter"].mean() / ref["mean_niter"] - 1) < 0.02
    assert abs(r["ncall"].mean() / ref["mean_ncall"] - 1) < 0.08
    assert abs(r["nbound"].mean() / ref["mean_nbound"] - 1) < 0.25
    assert abs(mean - TRUTH) < 4 * se, (mean, se)
