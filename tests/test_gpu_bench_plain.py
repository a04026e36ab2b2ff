"""A plain `bench.py` run (no --full): the headline line only, and --dump-outputs writes what the last timed step
computed -- here on a 256-run shard, whose outputs exceed the size cap, so a fixed sample of runs is kept."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--runs", "256", "--steps", "3",
                          "--warmup", "1", "--preroll", "2", "--dump-outputs", str(tmp_path)],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["unit"] == "proposals/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    for key in ("cpu_baseline", "roofline", "rccl_ranks"):  # --full only
        assert key not in line
    assert "verified" not in line["config"] and "end_to_end" not in line["config"]

    files = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= bench.DUMP_MAX_BYTES
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    sel = files["runs_sampled"].astype(int)
    assert 0 < len(sel) < 256 and np.all(np.diff(sel) > 0) and sel[-1] < 256
    n, kq, d = len(sel), 512, 25
    assert files["u"].shape == (n, kq, d) and files["logl"].shape == (n, kq) and files["covs"].shape[:2] == (n, 8)
    # what a caller of the timed path receives: bounds built, every walker walked all its steps inside the cube
    assert np.all(files["status"] == 0) and np.all(files["nells"] >= 1)
    assert np.all(files["accept"] + files["reject"] == 45)
    assert np.all((files["u"] > 0) & (files["u"] < 1))
    prob = bench.c2_problem()
    _, loglstar = bench.make_shard(prob, 1, 10, 0)
    moved = files["accept"] > 0
    assert moved.mean() > 0.9 and np.all(files["logl"][moved] > loglstar)
    unused = np.arange(8)[None, :] >= files["nells"][:, None]
    assert np.all(files["logvols"][unused] == 0) and np.all(files["logvols"][~unused] != 0)
