"""What dh_ns_batch decides before it touches the device (dynesty_amd/csrc/ns_batch_plan.h), on the host: a stand-alone
program (tests/host/ns_batch_plan_dump.cpp, which includes only that header, built with the address and
undefined-behaviour sanitizers; nothing is preloaded) is fed every combination the entry point refuses and a few it
accepts, and prints verdicts and sizes, which are checked against a restatement here."""
import json
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, SHAPE, NLIVE, SAMPLER, BOUND, KEEP, LOGL_MIN, LOGL_MAX, SEED, START = range(10)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is part of the build environment")
    exe = tmp_path_factory.mktemp("ns_batch_plan") / "dump"
    # -x c++: the header is plain C++17; a program of its own, so the sanitizers' runtime is linked in.  Host code only.
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-sanitize-recover=all", "-O1", "-g", "-Wall", "-I",
                           os.path.join(ROOT, "dynesty_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "host", "ns_batch_plan_dump.cpp")])

    def run(requests):
        inp = "".join(" ".join(str(x) for x in r) + "\n" for r in requests)
        res = subprocess.run([str(exe)], input=inp, capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
        out = res.stdout.splitlines()
        assert len(out) == len(requests)
        return [json.loads(line) for line in out]
    return run


def num(x):
    return "inf" if x == math.inf else "-inf" if x == -math.inf else "nan" if x != x else repr(float(x))


def check(runs=3, nlive=50, ndim=5, K=16, sampler=0, bound=1, keep=0, lmin=-8.0, lmax=math.inf, have=1, seed_lo=-7.9,
          nbad=-1, bad=0.0, start=0):
    return ["check", runs, nlive, ndim, K, sampler, bound, keep, num(lmin), num(lmax), have, num(seed_lo), nbad,
            num(bad), start]


def test_accepted_requests(dump):
    reqs = [check(), check(sampler=1), check(sampler=2), check(sampler=6, bound=0), check(nlive=4), check(nlive=65535, runs=1),
            check(lmax=-7.99), check(K=1), check(K=2048), check(runs=1, ndim=1), check(start=3),
            check(lmin=-1e300, seed_lo=-1e299)]
    for r, g in zip(reqs, dump(reqs)):
        assert g["verdict"] == OK and g["where"] == -1 and g["text"] == "ok", (r, g)


def test_every_refused_combination(dump):
    cases = [
        (check(sampler=3), SAMPLER), (check(sampler=4), SAMPLER), (check(sampler=5), SAMPLER),  # Philox rwalk / rslice / slice
        (check(sampler=7), SAMPLER), (check(sampler=-1), SAMPLER), (check(sampler=8), SAMPLER),  # Philox unif; no such code
        (check(bound=2, sampler=6), BOUND), (check(bound=3, sampler=6), BOUND), (check(bound=-1), BOUND),  # friends
        (check(keep=1), KEEP),
        (check(lmin=-math.inf), LOGL_MIN), (check(lmin=math.inf), LOGL_MIN), (check(lmin=math.nan), LOGL_MIN),
        (check(nbad=0, bad=-8.0), SEED),             # a seed AT logl_min
        (check(nbad=149, bad=-8.5), SEED),           # the last seed below it
        (check(nbad=77, bad=math.nan), SEED),        # a NaN seed
        (check(nbad=5, bad=-math.inf), SEED),
        (check(nlive=1), NLIVE), (check(nlive=0), NLIVE), (check(nlive=-4), NLIVE), (check(nlive=65536), NLIVE),
        (check(nlive=2), NLIVE), (check(nlive=3), NLIVE),  # below the loop's own four live points
        (check(lmax=-8.0), LOGL_MAX), (check(lmax=-9.0), LOGL_MAX), (check(lmax=math.nan), LOGL_MAX),
        (check(lmax=-math.inf), LOGL_MAX),
        (check(runs=0), SHAPE), (check(ndim=0), SHAPE), (check(K=0), SHAPE), (check(have=0), SHAPE),
        (check(start=1), START), (check(start=2), START),
    ]
    got = dump([c[0] for c in cases])
    for (req, want), g in zip(cases, got):
        assert g["verdict"] == want, (req, g)
        assert g["text"] != "ok" and g["text"] != "?"
    where = {tuple(c[0]): g["where"] for c, g in zip(cases, got)}
    assert where[tuple(check(nbad=0, bad=-8.0))] == 0 and where[tuple(check(nbad=149, bad=-8.5))] == 149
    assert where[tuple(check(nbad=77, bad=math.nan))] == 77
    assert where[tuple(check(start=1))] == 12 and where[tuple(check(start=2))] == 17  # the last of three runs
    assert where[tuple(check(keep=1))] == -1


def test_the_first_reason_wins_in_the_documented_order(dump):
    """shape, nlive_new, sampler, bound, keep, logl_min, logl_max, seeds, start rows"""
    reqs = [check(runs=0, nlive=1, sampler=3), check(nlive=1, sampler=3, bound=2), check(sampler=3, bound=2, keep=1),
            check(bound=2, keep=1, lmin=math.nan), check(keep=1, lmin=math.inf), check(lmin=math.inf, lmax=-math.inf),
            check(lmax=-9.0, nbad=3, bad=-9.0), check(nbad=3, bad=-9.0, start=1)]
    want = [SHAPE, NLIVE, SAMPLER, BOUND, KEEP, LOGL_MIN, LOGL_MAX, SEED]
    assert [g["verdict"] for g in dump(reqs)] == want


def pad256(b):
    return (b + 255) & ~255


def test_sizes(dump):
    shapes = [(3, 50, 5, 16), (1, 64, 5, 16), (64, 2000, 25, 512), (2, 96, 40, 32), (1, 4, 1, 1), (5, 7, 3, 2048),
              (1, 65535, 2, 2048)]
    got = dump([["sizes", *s] for s in shapes])
    for (R, N, D, K), g in zip(shapes, got):
        fills = -(-N // K)
        assert g["seed_fills"] == fills, (R, N, D, K, g)
        assert g["stage_points"] == R * N
        want = (2 * pad256(R * N * D * 8) + pad256(R * N * 8) + pad256(R * N * 4) + pad256(R * 4) + 2 * pad256(R * 8) +
                pad256(R * 32) + pad256(R * 48))
        assert g["stage_bytes"] == want, (R, N, D, K, g, want)
    assert got[0]["seed_fills"] == 4 and got[1]["seed_fills"] == 4 and got[2]["seed_fills"] == 4  # 50/16, 64/16, 2000/512
