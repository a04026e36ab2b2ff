"""The resident loop's state between two calls (dynesty_amd/csrc/ns_state.h), held to its contract on the host: a
stand-alone program (tests/host/ns_state_dump.cpp, which includes only that header, built with the address and
undefined-behaviour sanitizers; nothing is preloaded) evaluates the stop rule a continuation applies before its first
fill against a restatement of the reference's top-of-loop tests (sampler.py:1071-1100), round-trips an image's header,
rejects every damaged image the import must reject, and adds up an image's bytes against a restatement here."""
import itertools
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 88  # sizeof(dh_ns_state::Header)
DLOGZ, LOGL_MAX, MAXITER, MAXCALL, PLATEAU = 1, 2, 4, 8, 16
IMG = dict(ok=0, short_header=1, magic=2, version=3, run_size=4, plan_size=5, shape=6, truncated=7, rows=8,
           capacity=9, ndim=10)
WRITER = dict(version=100, sizeof_run=176, plan_bytes=64, ndim=5)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is part of the build environment")
    exe = tmp_path_factory.mktemp("ns_state") / "dump"
    # -x c++: the header is plain C++17 and is compiled as such; a program of its own, so the sanitizers' runtime is
    # linked in.  Host code only: -fno-gpu-sanitize says so outright
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-sanitize-recover=all", "-O1", "-g", "-Wall", "-I",
                           os.path.join(ROOT, "dynesty_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "host", "ns_state_dump.cpp")])

    def run(requests):
        inp = "".join(" ".join(x if isinstance(x, str) else repr(x) for x in r) + "\n" for r in requests)
        res = subprocess.run([str(exe)], input=inp, capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
        out = res.stdout.splitlines()
        assert len(out) == len(requests)
        return [json.loads(line) for line in out]
    return run


def num(x):
    return "inf" if x == math.inf else "-inf" if x == -math.inf else repr(float(x))


# ---- the stop rule -------------------------------------------------------------------------------------------------
def reference_stop(logvol, logz, lmax, loglstar, dead_prev, it, ncall, dlogz, logl_max, maxiter, maxcall):
    """sampler.py:1071-1100 on the state a run holds: live_logl's maximum is lmax, its minimum loglstar, the last dead
    point's ln L (`loglstar` there) dead_prev; maxiter / maxcall None = sys.maxsize"""
    with np.errstate(over="ignore"):
        delta_logz = np.logaddexp(0, lmax + logvol - logz)
    m = 0
    if it > (maxiter if maxiter >= 0 else math.inf):
        m |= MAXITER
    if ncall > (maxcall if maxcall >= 0 else math.inf):
        m |= MAXCALL
    if delta_logz < dlogz:
        m |= DLOGZ
    if dead_prev > logl_max:
        m |= LOGL_MAX
    if lmax - loglstar == 0:  # np.ptp(live_logl) == 0
        m |= PLATEAU
    return m, float(delta_logz)


def stop_request(s, c):
    return ["stop"] + [num(v) for v in s[:5]] + [str(s[5]), str(s[6]), num(c[0]), num(c[1]), str(c[2]), str(c[3])]


def test_stop_rule_matches_the_reference(dump):
    # (logvol, logz, lmax, loglstar, dead_prev, it, ncall)
    mid = (-4.5, -10.2, -3.1, -6.0, -6.2, 900, 5000)
    late = (-14.0, -10.4, -2.9, -2.95, -2.96, 2800, 60000)
    fresh = (0.0, -1e300, -2.0, -80.0, -1e300, 0, 200)  # ns_init / ns_start: nothing integrated yet
    plateau = (-3.0, -9.0, -5.0, -5.0, -5.0, 600, 2000)  # the worst live value has reached the largest
    states = [mid, late, fresh, plateau]
    cases = []
    for s in states:
        dz = reference_stop(*s, 0.0, math.inf, -1, -1)[1]
        dl = [0.1, 1e-3] + ([dz * (1 - 1e-9), dz * (1 + 1e-9)] if math.isfinite(dz) else [1e299])  # either side of dz
        lm = [math.inf, s[4], math.nextafter(s[4], -math.inf), s[4] + 1.0]  # dead_prev == logl_max: strict
        mi = [-1, s[5], s[5] - 1, s[5] + 1, 0]  # it == maxiter, it == maxiter + 1
        mc = [-1, s[6], s[6] - 1, s[6] + 1]  # ncall == maxcall
        cases += [(s, c) for c in itertools.product(dl, lm, mi, mc)]
    # loglstar == lmax exactly and one ulp below
    cases += [((-3.0, -9.0, -5.0, math.nextafter(-5.0, -math.inf), -5.2, 600, 2000), (0.01, math.inf, -1, -1))]
    got = dump([stop_request(s, c) for s, c in cases])
    seen = set()
    for (s, c), g in zip(cases, got):
        want, dz = reference_stop(*s, *c)
        assert g["mask"] == want, (s, c, g, want)
        assert g["dz"] == pytest.approx(dz, rel=1e-14), (s, g, dz)
        seen.add(want)
    # the grid reaches none of the tests, each of the criteria on its own, and the plateau
    assert 0 in seen and {DLOGZ, LOGL_MAX, MAXITER, MAXCALL} <= seen
    assert all(any(w & bit for w in seen) for bit in (DLOGZ, LOGL_MAX, MAXITER, MAXCALL, PLATEAU))


def test_stop_rule_edges_one_by_one(dump):
    s = (-4.5, -10.2, -3.1, -6.0, -6.2, 900, 5000)
    none = (1e-6, math.inf, -1, -1)

    def mask(state=s, **c):
        rule = dict(zip(("dlogz", "logl_max", "maxiter", "maxcall"), none))
        rule.update(c)
        return dump([stop_request(state, tuple(rule.values()))])[0]["mask"]
    assert mask() == 0
    assert mask(maxiter=900) == 0 and mask(maxiter=899) == MAXITER  # it == maxiter goes on; it == maxiter + 1 stops
    assert mask(maxcall=5000) == 0 and mask(maxcall=4999) == MAXCALL
    assert mask(logl_max=-6.2) == 0 and mask(logl_max=math.nextafter(-6.2, -math.inf)) == LOGL_MAX
    dz = reference_stop(*s, *none)[1]
    assert mask(dlogz=dz * (1 + 1e-9)) == DLOGZ and mask(dlogz=dz * (1 - 1e-9)) == 0
    assert mask(state=s[:3] + (s[2],) + s[4:]) == PLATEAU
    fresh = (0.0, -1e300, -2.0, -80.0, -1e300, 0, 200)
    assert mask(state=fresh, dlogz=1e299) == 0  # delta ln Z of a state with ln Z = -1e300 is ~1e300
    assert mask(state=fresh, maxiter=0) == 0 and mask(state=fresh, maxcall=199) == MAXCALL


# ---- the image -----------------------------------------------------------------------------------------------------
def pad8(n):
    return (n + 7) & ~7


def image_bytes(plan_bytes, runs, fixed_bytes, elems, rows):
    """header | plan | one int64 per run | the fixed arrays | per dead-point array and run: its rows, padded"""
    return HEADER + pad8(plan_bytes) + 8 * runs + fixed_bytes + sum(pad8(r * e) for e in elems for r in rows)


def test_image_size_arithmetic(dump):
    reqs, want = [], []
    for plan_bytes, fixed, elems, rows in itertools.product(
            [64, 460, 461], [0, 8, 123456], [[8], [8, 40, 4, 4, 4], [8, 24, 4, 4, 4]],
            [[0], [1], [151, 151, 151, 151, 151], [3, 0, 2 ** 31 + 5], [7, 1, 300]]):
        reqs.append(["size", str(plan_bytes), str(len(rows)), str(fixed), str(len(elems))] + [str(e) for e in elems] +
                    [str(r) for r in rows])
        want.append(image_bytes(plan_bytes, len(rows), fixed, elems, rows))
    for g, w in zip(dump(reqs), want):
        assert g["header"] == HEADER and g["bytes"] == w, (g, w)
    # the capacity is no part of it: the same rows at any max_iter are the same bytes (nothing above takes a capacity)


def image_request(what, rows, cap=1000, fixed=4096, max_iter=0, **reader):
    r = dict(WRITER)
    r.update(reader)
    return ["image", what, str(r["version"]), str(r["sizeof_run"]), str(r["plan_bytes"]), str(r["ndim"]), str(max_iter),
            str(len(rows)), str(cap), str(fixed)] + [str(x) for x in rows]


def test_header_round_trip_and_rejections(dump):
    rows = [151, 151, 0, 999, 1000]
    cases = [
        (image_request("ok", rows), "ok", 1000),
        (image_request("ok", rows, max_iter=1000), "ok", 1000),
        (image_request("ok", rows, max_iter=40000), "ok", 40000),  # more room on import
        (image_request("magic", rows), "magic", 0),
        (image_request("version", rows), "version", 0),
        (image_request("ok", rows, version=101), "version", 0),
        (image_request("runsize", rows), "run_size", 0),
        (image_request("ok", rows, sizeof_run=184), "run_size", 0),
        (image_request("plan", rows), "plan_size", 0),
        (image_request("short1", rows), "truncated", 0),
        (image_request("cuthdr", rows), "short_header", 0),
        (image_request("ok", [151, 1001]), "rows", 0),  # a row count above the saved capacity
        (image_request("ok", [151, -1]), "rows", 0),
        (image_request("ok", rows, max_iter=999), "capacity", 0),  # max_iter below a run's niter
        (image_request("ok", rows, ndim=3), "ndim", 0),
        (image_request("short1", [0], fixed=0), "truncated", 0),  # the smallest image there is, one byte short
    ]
    got = dump([c[0] for c in cases])
    for (req, want, cap), g in zip(cases, got):
        assert g["code"] == IMG[want], (req, g)
        assert g["cap"] == cap, (req, g)
        if all(0 <= int(x) <= int(req[8]) for x in req[10:]):
            assert g["same"] == 1, (req, g)  # the undamaged image came back as written
    assert got[0]["total"] == image_bytes(64, 5, 4096, [8], rows)
