"""Where the host-pointer entry points outside the combiner stage their arrays (dynesty_amd/csrc/stage_plan.h), held to
its invariants on the host: a stand-alone program (tests/host/stage_plan_dump.cpp, which includes only that header, built
with the address and undefined-behaviour sanitizers) walks every layout over a grid of shapes -- the smallest legal shape
of each call, a bench-sized one (64 x 512 walkers, 25 dimensions), a wide one (512 dimensions), every optional array on
and off.  The layouts' geometry is checked, and their totals against a restatement of the byte counts the entry points
reserved by hand before the layouts existed, so the arena never grows where it did not grow before.  Where a layout needs
more than the parent reserved, the parent under-counted: those shapes are listed by name with the exact excess."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K_ALL = [1, 65, 64 * 512]
D_ALL = [1, 25, 512]
FLAGS = (0, 1)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is part of the build environment")
    exe = tmp_path_factory.mktemp("stage_plan") / "dump"
    # -x c++: the header is plain C++17 and is compiled as such, with no HIP in sight; a program of its own, so the
    # sanitizers' runtime is linked in and nothing is preloaded.  Host code only: -fno-gpu-sanitize says so outright
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                           "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "dynesty_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "host", "stage_plan_dump.cpp")])

    def run(requests):
        inp = "".join(" ".join(str(int(x)) if not isinstance(x, str) else x for x in r) + "\n" for r in requests)
        res = subprocess.run([str(exe)], input=inp, capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr, res.stderr[-2000:]
        out = res.stdout.splitlines()
        assert len(out) == len(requests)
        return [json.loads(line) for line in out]
    return run


def al(nbytes):
    return (nbytes + 255) & ~255


def check_geometry(req, lay, sizes):
    """`sizes`: the arrays in the order the call takes them, (name, bytes wanted or None).  Aligned, in that order,
    disjoint, each at least as large as asked, inside the total; what is not wanted is null and takes no room -- and
    nothing else is; the two walks agree."""
    assert lay["total"] == lay["end"], req
    assert [s[0] for s in lay["slots"]] == [name for name, _ in sizes], req
    end = 0
    for (name, off, nbytes, null), (_, want) in zip(lay["slots"], sizes):
        assert off % 256 == 0 and off >= end, (req, name)
        assert null == (nbytes == 0) == (want is None), (req, name)
        assert nbytes == (want or 0) and off + nbytes <= lay["total"], (req, name)
        if want is None:
            assert off == al(end), (req, name)  # no room: the next array starts where this one would have
        end = off + nbytes
    assert lay["total"] == al(end), req


def opt(nbytes, on):
    return nbytes if on else None


# ---- per layout: the arrays (name, bytes | None) in the order of the call, and the parent's hand-written reserve ------
def friends_batch_ws_bytes(R, n, d, nboot):  # friends.hip, unchanged by the layouts
    nd, nw, reps = n * d, (n + 63) // 64, max(nboot, 1)
    return (2 * al(R * nd * 8) + al(R * n * nw * 8) + al(R * n * 4) + 2 * al(R * 4) + al(R * d * 8) + al(R * 16) +
            al(R * reps * n * 8) + al(R * 8) + 1024)


def lay_propose(k, ndim, ncdim, m, idx, bc):
    kd = k * ndim
    sizes = [("u0", kd * 8), ("axes", m * ncdim * ncdim * 8), ("axes_idx", opt(k * 4, idx)), ("bc", opt(ndim, bc)),
             ("rng", k * 32), ("u", kd * 8), ("inside", k * 4), ("rng_out", k * 32)]
    return sizes, 2 * kd * 8 + m * ncdim * ncdim * 8 + k * (4 + 4 + 64) + ndim + 8192


def lay_rwalk(k, ndim, ncdim, m, idx, bc, philox):
    kd = k * ndim
    sizes = [("u0", kd * 8), ("axes", m * ncdim * ncdim * 8), ("axes_idx", opt(k * 4, idx)), ("bc", opt(ndim, bc)),
             ("rng", opt(k * 32, not philox)), ("u", kd * 8), ("v", kd * 8), ("logl", k * 8), ("naccept", k * 4),
             ("nreject", k * 4), ("rng_out", opt(k * 32, not philox))]
    per = (4 + 8 + 4 + 4) if philox else (4 + 8 + 4 + 4 + 64)
    return sizes, 3 * kd * 8 + m * ncdim * ncdim * 8 + k * per + ndim + 16 * 256


def lay_eval(k, ndim):
    kd = k * ndim
    return [("u", kd * 8), ("v", kd * 8), ("logl", k * 8)], 2 * kd * 8 + k * 8 + 4096


def lay_seed(k, n_words):
    return [("entropy", n_words * 4), ("states", k * 32)], k * 32 + 1024


def lay_stream(nn, nu):
    return [("state", 32), ("normals", (nn + 1) * 8), ("unifs", (nu + 1) * 8), ("state_out", 32)], (nn + nu) * 8 + 4096


def lay_slice(k, ndim, m, idx, philox):
    kd = k * ndim
    sizes = [("u0", kd * 8), ("axes", m * ndim * ndim * 8), ("axes_idx", opt(k * 4, idx)), ("rng", opt(k * 32, not philox)),
             ("u", kd * 8), ("v", kd * 8), ("logl", k * 8), ("ncalls", k * 4), ("nexpand", k * 4), ("ncontract", k * 4),
             ("flags", k * 4), ("rng_out", k * 32)]
    return sizes, 3 * kd * 8 + m * ndim * ndim * 8 + k * (8 + 20 + 64) + 8192


def lay_unif(k, ndim, ncdim, m, bc, philox):
    kd, mm = k * ndim, max(m, 1)
    sizes = [("ctrs", opt(m * ncdim * 8, m > 0)), ("axes", opt(m * ncdim * ncdim * 8, m > 0)),
             ("ams", opt(m * ncdim * ncdim * 8, m > 1)), ("cumprob", opt(m * 8, m > 1)), ("bc", opt(ndim, bc)),
             ("rng", opt(k * 32, not philox)), ("u", kd * 8), ("v", kd * 8), ("logl", k * 8), ("ncalls", k * 4),
             ("flags", k * 4), ("rng_out", k * 32)]
    return sizes, 2 * kd * 8 + mm * (2 * ncdim * ncdim + ncdim + 1) * 8 + k * (8 + 8 + 64) + ndim + 8192


def lay_unif_friends(k, ndim, n, bc, r32, r32o):
    kd, nd, dd = k * ndim, n * ndim, ndim * ndim
    sizes = [("ctrs", nd * 8), ("axes", dd * 8), ("axes_inv", dd * 8), ("ct", nd * 8), ("bc", opt(ndim, bc)),
             ("rng", k * 32), ("u", kd * 8), ("v", kd * 8), ("logl", k * 8), ("ncalls", k * 4), ("flags", k * 4),
             ("rng_out", k * 32), ("rng32", opt(k * 16, r32)), ("rng32_out", opt(k * 16, r32o))]
    return sizes, 2 * kd * 8 + 2 * nd * 8 + 2 * dd * 8 + k * (8 + 8 + 64 + 32) + ndim + 8192


def lay_bound_draw(nsamp, d, m):
    dd = d * d
    sizes = [("state", 32), ("ctrs", m * d * 8), ("axes", m * dd * 8), ("ams", opt(m * dd * 8, m > 1)),
             ("cumprob", opt(m * 8, m > 1)), ("x", nsamp * d * 8), ("idx", nsamp * 4), ("q", nsamp * 4), ("status", 4),
             ("state_out", 32), ("work", 2 * d * 8)]
    return sizes, (m * (2 * dd + d + 1) + nsamp * d + 2 * d) * 8 + nsamp * 8 + 8192


def lay_slice_feed(k, ndim, kind, m, nlook, idx, consumed):
    kd = k * ndim
    sizes = [("axes", opt(m * ndim * ndim * 8, kind == 0)), ("axes_idx", opt(k * 4, kind == 0 and idx)), ("st6", k * 48),
             ("consumed", opt(k * 4, consumed)), ("dirs", opt(kd * 8, kind == 0)), ("perm", opt(kd * 4, kind == 1)),
             ("look", opt(k * nlook * 8, nlook > 0))]
    return sizes, (m * ndim * ndim * 8 + kd * 8 if kind == 0 else 0) + kd * 4 + k * (48 + 4 + 4 + nlook * 8) + 8192


def lay_friends_update(n, d, nboot, prev):
    nd, dd, nw, reps = n * d, d * d, (n + 63) // 64, max(nboot, 1)
    sizes = [("x", nd * 8), ("y", nd * 8), ("mv", nd * 8), ("prev", opt(dd * 8, prev)), ("bits", n * nw * 8),
             ("label", n * 4), ("nc", 8), ("mean", d * 8), ("cov", dd * 8), ("am", dd * 8), ("axes", dd * 8),
             ("axes_inv", dd * 8), ("info", 32), ("status", 8), ("mask", opt(nboot * n, nboot > 0)), ("nn", reps * n * 8),
             ("r", 8)]
    return sizes, nd * 8 * 3 + n * nw * 8 + n * 4 + dd * 8 * 6 + reps * n * 9 + 65536


def lay_friends_batch(R, n, d, nboot, wsb, prev, active):
    nd, dd = n * d, d * d
    sizes = [("x", R * nd * 8), ("prev", opt(R * dd * 8, prev)), ("mask", opt(R * nboot * n, nboot > 0)),
             ("active", opt(R * 4, active)), ("cov", R * dd * 8), ("am", R * dd * 8), ("axes", R * dd * 8),
             ("axes_inv", R * dd * 8), ("logvol", R * 8), ("rmax", R * 8), ("nclusters", R * 4), ("status", R * 4),
             ("ws", wsb)]
    return sizes, (R * nd * 8 + (R * dd * 8 if prev else 0) + (R * nboot * n if nboot > 0 else 0) + R * 4 +
                   R * (4 * dd * 8 + 16 + 8) + wsb + 65536)


def lay_friends_within(n, d, m, bits):
    nd, md, dd, nw = n * d, m * d, d * d, (n + 63) // 64
    sizes = [("ctrs", nd * 8), ("x", md * 8), ("axes_inv", dd * 8), ("ct", nd * 8), ("xt", md * 8), ("counts", m * 4),
             ("bits", opt(m * nw * 8, bits))]
    return sizes, (nd + md) * 16 + dd * 8 + m * 4 + (m * nw * 8 if bits else 0) + 8192


def lay_friends_draw(nsamp, n, d):
    nd, dd = n * d, d * d
    sizes = [("state", 48), ("ctrs", nd * 8), ("axes", dd * 8), ("axes_inv", dd * 8), ("ct", nd * 8), ("x", nsamp * d * 8),
             ("q", nsamp * 4), ("state_out", 48)]
    return sizes, nd * 16 + dd * 16 + nsamp * (d * 8 + 4) + 8192


def lay_rebuild(n, d, me, leaf):
    dd = d * d
    sizes = [("pts", n * d * 8), ("nells", 4), ("status", 4), ("nnodes", 4), ("ctrs", me * d * 8), ("covs", me * dd * 8),
             ("ams", me * dd * 8), ("axes", me * dd * 8), ("axlens", me * d * 8), ("logvols", me * 8),
             ("leaf_of_point", opt(n * 4, leaf))]
    return sizes, (n * d + me * (3 * dd + 2 * d + 1)) * 8 + n * 4 + 8192


def lay_ell_from_cov(m, d):
    dd = d * d
    sizes = [("covs", m * dd * 8), ("axes", m * dd * 8), ("ams", m * dd * 8), ("axlens", m * d * 8), ("logvols", m * 8),
             ("status", m * 4)]
    return sizes, m * (3 * dd + d + 2) * 8 + 8192


def lay_improve_cov(m, d):
    dd, LD = d * d, d | 1
    sizes = [("padded", m * d * LD * 8), ("covs", m * dd * 8), ("ams", m * dd * 8), ("axes", m * dd * 8), ("good", m * 4)]
    return sizes, m * (d * LD + 3 * dd + 1) * 8 + 8192


def lay_scale_logvol(m, d):
    dd = d * d
    sizes = [("covs", m * dd * 8), ("ams", m * dd * 8), ("axes", m * dd * 8), ("axlens", m * d * 8), ("logvols", m * 8),
             ("targets", m * 8)]
    return sizes, m * (3 * dd + d + 2) * 8 + 8192


def lay_boot_expand(runs, n, d, wsb):
    sizes = [("pts", runs * n * d * 8), ("ent", runs * 32), ("ws", wsb), ("shift", runs * 8), ("expand", runs * 8),
             ("bstatus", runs * 4)]
    return sizes, wsb + runs * n * d * 8 + runs * (32 + 16) + 4096


def lay_contains(k, d, m, mask, quad):
    nwords = (k + 63) // 64
    sizes = [("x", k * d * 8), ("ctrs", m * d * 8), ("ams", m * d * d * 8), ("count", k * 4),
             ("mask", opt(nwords * m * 8, mask)), ("quad", opt(k * m * 8, quad))]
    return sizes, (k * d + m * d + m * d * d + k * m) * 8 + k * 4 + nwords * m * 8 + 8192


def lay_ns_consume(R, N, K, run_bytes, pt):
    sizes = [("st", R * run_bytes), ("live_logl", R * N * 8), ("dead_logl", R * K * 8), ("r_logl", R * K * 8),
             ("r_a", R * K * 4), ("trace_slot", R * K * 4), ("trace_src", R * K * 4), ("trace_n", R * 8), ("ndone", 64),
             ("bstatus", R * 4), ("live_it", opt(R * N * 4, pt)), ("dead_id", opt(R * K * 4, pt)),
             ("dead_it", opt(R * K * 4, pt)), ("dead_nc", opt(R * K * 4, pt))]
    return sizes, R * (run_bytes + N * 24 + K * 40 + 64) + 16384


def lay_contains_runs(runs, wpr, d, me, nells, run_mode, bstatus, first):
    """dh_contains_runs has no hand-written predecessor: its reserve is the sum of its arrays, each rounded up."""
    sizes = [("x", runs * wpr * d * 8), ("ctrs", runs * me * d * 8), ("ams", runs * me * d * d * 8),
             ("nells", opt(runs * 4, nells)), ("run_mode", opt(runs * 4, run_mode)), ("bstatus", opt(runs * 4, bstatus)),
             ("flag", runs * 4), ("first", opt(runs * 4, first))]
    return sizes, sum(al(b) for _, b in sizes if b is not None)


def lay_enlarge_runs(runs, me, d, active, run_shift):
    """dh_enlarge_runs has no hand-written predecessor either: the sum of its arrays, each rounded up."""
    m, dd = runs * me, d * d
    sizes = [("covs", m * dd * 8), ("ams", m * dd * 8), ("axes", m * dd * 8), ("axlens", m * d * 8), ("logvols", m * 8),
             ("nells", runs * 4), ("active", opt(runs * 4, active)), ("run_shift", opt(runs * 8, run_shift))]
    return sizes, sum(al(b) for _, b in sizes if b is not None)


LAYOUTS = {"propose": lay_propose, "rwalk": lay_rwalk, "eval": lay_eval, "seed": lay_seed, "stream": lay_stream,
           "slice": lay_slice, "unif": lay_unif, "unif_friends": lay_unif_friends, "bound_draw": lay_bound_draw,
           "slice_feed": lay_slice_feed, "friends_update": lay_friends_update, "friends_batch": lay_friends_batch,
           "friends_within": lay_friends_within, "friends_draw": lay_friends_draw, "rebuild": lay_rebuild,
           "ell_from_cov": lay_ell_from_cov, "improve_cov": lay_improve_cov, "scale_logvol": lay_scale_logvol,
           "boot_expand": lay_boot_expand, "contains": lay_contains, "ns_consume": lay_ns_consume,
           "contains_runs": lay_contains_runs, "enlarge_runs": lay_enlarge_runs}

# Shapes whose layout needs more than the parent reserved, with the exact excess in bytes: the parent under-counted.
# dh_bootstrap_expand reserved 32 + 16 bytes per run beside the workspace and the points, and took 32 (entropy) + 8
# (shift) + 8 (expand) + 4 (status) = 52; its 4096 bytes of slack covered the difference up to 768 runs.
# At 4096 runs: 4 x 4096 bytes short, less the slack, plus what the alignment of six arrays takes at that workspace size.
UNDERCOUNTED = {("boot_expand", 4096, n, d, wsb): excess
                for n, d in ((2, 1), (2000, 25), (2, 512))
                for wsb, excess in ((1, 12543), (4097, 12543), (123456789, 12523))}


def walk(dump, requests):
    seen = set()
    for req, lay in zip(requests, dump(requests)):
        sizes, parent = LAYOUTS[req[0]](*req[1:])
        check_geometry(req, lay, sizes)
        if req in UNDERCOUNTED:
            seen.add(req)
            assert lay["total"] - parent == UNDERCOUNTED[req], (req, lay["total"], parent)
        else:
            assert lay["total"] <= parent, (req, lay["total"], parent)
    return seen


def test_walk_layouts(dump):
    reqs = []
    for k, d, m, idx, bc in itertools.product(K_ALL, D_ALL, (1, 3), FLAGS, FLAGS):
        for nc in sorted({1, d}):
            reqs.append(("propose", k, d, nc, m, idx, bc))
            reqs += [("rwalk", k, d, nc, m, idx, bc, philox) for philox in FLAGS]
    reqs += [("eval", k, d) for k, d in itertools.product(K_ALL, D_ALL)]
    reqs += [("seed", k, nw) for k, nw in itertools.product(K_ALL + [7], (1, 4, 64))]
    reqs += [("stream", nn, nu) for nn, nu in itertools.product((0, 1, 31, 32, 100000), repeat=2)]
    assert not walk(dump, reqs)


def test_walk2_layouts(dump):
    reqs = [("slice", k, d, m, idx, philox) for k, d, m, idx, philox in itertools.product(K_ALL, D_ALL, (1, 3), FLAGS, FLAGS)]
    for k, d, m, bc, philox in itertools.product(K_ALL, D_ALL, (0, 1, 2, 40), FLAGS, FLAGS):
        reqs += [("unif", k, d, nc, m, bc, philox) for nc in sorted({1, d})]
    reqs += [("unif_friends", k, d, n, bc, r32, r32o)
             for k, d, n, bc, r32, r32o in itertools.product(K_ALL, D_ALL, (1, 2000), FLAGS, FLAGS, FLAGS)]
    reqs += [("bound_draw", ns, d, m) for ns, d, m in itertools.product((1, 65, 100000), D_ALL, (1, 2, 40))]
    reqs += [("slice_feed", k, d, kind, m, nlook, idx, cons)
             for k, d, kind, m, nlook, idx, cons in itertools.product(K_ALL, D_ALL, (0, 1, 2), (1, 3), (0, 1, 64), FLAGS, FLAGS)]
    assert not walk(dump, reqs)


def test_friends_layouts(dump):
    N_ALL = [2, 65, 2000]
    reqs = [("friends_update", n, d, nboot, prev) for n, d, nboot, prev in itertools.product(N_ALL, D_ALL, (0, 1, 20), FLAGS)]
    reqs += [("friends_batch", R, n, d, nboot, friends_batch_ws_bytes(R, n, d, nboot), prev, act)
             for R, n, d, nboot, prev, act in itertools.product((1, 64), N_ALL, D_ALL, (0, 1, 20), FLAGS, FLAGS)]
    reqs += [("friends_within", n, d, m, bits) for n, d, m, bits in itertools.product([1] + N_ALL, D_ALL, K_ALL, FLAGS)]
    reqs += [("friends_draw", ns, n, d) for ns, n, d in itertools.product((1, 65, 100000), [1] + N_ALL, D_ALL)]
    assert not walk(dump, reqs)


def test_rebuild_boot_bound_layouts(dump):
    reqs = [("rebuild", n, d, me, leaf) for n, d, me, leaf in itertools.product((2, 2000, 64 * 512), D_ALL, (1, 40), FLAGS)]
    for word in ("ell_from_cov", "improve_cov", "scale_logvol"):
        reqs += [(word, m, d) for m, d in itertools.product((1, 40, 4096), D_ALL)]
    reqs += [("boot_expand", runs, n, d, wsb)
             for runs, (n, d), wsb in itertools.product((1, 64, 4096), ((2, 1), (2000, 25), (2, 512)), (1, 4097, 123456789))]
    reqs += [("contains", k, d, m, mask, quad) for k, d, m, mask, quad in itertools.product(K_ALL, D_ALL, (1, 40), FLAGS, FLAGS)]
    reqs += [("contains_runs", runs, wpr, d, me, nells, rm, bs, first)
             for runs, wpr, d, me, nells, rm, bs, first in itertools.product((1, 7, 64), (1, 83, 512), D_ALL, (1, 4), FLAGS, FLAGS,
                                                                             FLAGS, FLAGS)]
    reqs += [("enlarge_runs", runs, me, d, act, rs)
             for runs, me, d, act, rs in itertools.product((1, 5, 64), (1, 4, 40), D_ALL, FLAGS, FLAGS)]
    assert walk(dump, reqs) == set(UNDERCOUNTED)  # every named exception is met, with its exact excess


def test_ns_consume_layout(dump):
    reqs = [("ns_consume", R, N, K, rb, pt)
            for R, N, K, rb, pt in itertools.product((1, 64, 4096), (4, 500, 65535), (1, 64, 8192), (8, 200, 1024), FLAGS)]
    assert not walk(dump, reqs)
