"""Where the fold of dynamic batches keeps its arrays (dynesty_amd/csrc/merge_plan.h: the batch column, the fold's
scratch and stage, the row gather), held to its invariants on the host: a stand-alone program
(tests/host/fold_plan_dump.cpp, which includes only that header, built with the address and undefined-behaviour
sanitizers) walks every layout over a grid of shapes.  Checked: every array aligned, inside the total and disjoint from
the others; what is not wanted null and without room; the totals against the byte counts written out here; the static
LDS of the fold's kernels against the CU's 160 KB; and that the fold left the merged run's own layout alone (its batch
column is an allocation of its own)."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024
K_CHUNK = 2048

M_ALL = [1, 7, 2047, 2048, 2049, 524289, 2 ** 30]
W_ALL = [1, 5, 2049, 2 ** 30]
D_ALL = [1, 3, 33, 512]
RN_ALL = [(1, 1), (3, 5), (64, 2000)]
FLAGS = (0, 1)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is part of the build environment")
    exe = tmp_path_factory.mktemp("fold_plan") / "dump"
    # plain C++17, a program of its own: the sanitizers' runtime is linked in, nothing is preloaded, host code only
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
                           "-fno-sanitize-recover=all", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "dynesty_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "host", "fold_plan_dump.cpp")])

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


def ceil_div(a, b):
    return (a + b - 1) // b


def moment_chunks(M, cols):
    n = max(min(ceil_div(M, 2048), 1024, (8 << 20) // (cols or 1)), 1)
    return ceil_div(M, ceil_div(M, n))


def check_geometry(req, lay, unwanted=()):
    """Aligned, inside the total, no overlap; what is not wanted is null and takes no room -- and nothing else is."""
    assert lay["total"] == lay["end"], req  # the two walks agree
    end = 0
    for name, off, nbytes, null in lay["slots"]:
        assert off % 256 == 0 and off >= end, (req, name)
        assert off + nbytes <= lay["total"], (req, name)
        assert null == (nbytes == 0) == (name in unwanted), (req, name, unwanted)
        end = off + nbytes
    assert lay["total"] == al(end)
    names = [s[0] for s in lay["slots"]]
    assert len(set(names)) == len(names) and set(unwanted) <= set(names), req


def test_fold_scratch_geometry_and_total(dump):
    reqs = [("fold_scratch", M, W, R, N, D, pt)
            for M, W, (R, N), D, pt in itertools.product(M_ALL, W_ALL, RN_ALL, D_ALL, FLAGS) if (M + W) * D < 2 ** 32]
    assert len(reqs) > 300
    for req, lay in zip(reqs, dump(reqs)):
        _, M, W, R, N, D, pt = req
        check_geometry(req, lay, () if pt else ("n_id", "n_it", "n_nc"))
        T = M + W
        sizes = ([8 * (R + 1), 8 * R] + [8 * W] * 3 + [8 * W * D] * 2 + [8 * W] + [8 * T] * 3 +
                 [8 * moment_chunks(T, D + 2) * (D + 2), 8, 64] + [4 * W] * 3 + [4 * R * N] + [4 * W] * (6 if pt else 3) +
                 [4 * T] * 3 + [4 * R, 4, 16, 8, (ceil_div(T, K_CHUNK) + 1) * 16])
        assert lay["total"] == sum(al(s) for s in sizes), req
        slots = {s[0]: s[2] for s in lay["slots"]}
        assert slots["src"] == slots["finnew"] == slots["gstart"] == 4 * T and slots["ustage"] == slots["vstage"] == 8 * W * D


def test_batch_column_stage_and_row_gather(dump):
    reqs = [("batch", T) for T in M_ALL]
    for req, lay in zip(reqs, dump(reqs)):
        check_geometry(req, lay)
        assert lay["total"] == al(4 * req[1]) and [s[0] for s in lay["slots"]] == ["batch"]
    pt_only = ("dead_id", "dead_it", "dead_nc", "live_it")
    reqs = [("fold_stage", R, N, D, S, pt) for (R, N), D, S, pt in itertools.product(RN_ALL, D_ALL, (1, 7, 30000), FLAGS)]
    for req, lay in zip(reqs, dump(reqs)):
        _, R, N, D, S, pt = req
        check_geometry(req, lay, () if pt else pt_only)
        sizes = [8 * R * S, 8 * R * N, 8 * R * S * D, 8 * R * N * D] + ([4 * R * S] * 3 + [4 * R * N] if pt else [])
        assert lay["total"] == sum(al(s) for s in sizes), req
    reqs = [("gather_rows", n, D) for n, D in itertools.product((1, 7, 4097, 8388607 // 512), D_ALL)]
    for req, lay in zip(reqs, dump(reqs)):
        check_geometry(req, lay)
        assert lay["total"] == al(8 * req[1]) + al(8 * req[1] * req[2]), req


def test_the_merged_run_layout_is_untouched_by_the_fold(dump):
    """The batch column is no part of carve_merged's walk (tests/test_merge_plan_cpu.py pins its total): the names here."""
    (lay,) = dump([("merged", 2049, 3, 1)])
    assert [s[0] for s in lay["slots"]] == ["logl", "logvol", "logwt", "logz", "logzerr", "h", "w", "cw", "u", "v", "mom",
                                            "run", "seq", "n", "fin", "id", "it", "nc"]


def test_static_lds_of_the_fold_kernels_fits_a_cu(dump):
    (a,) = dump([("lds",)])
    assert a["rank"] == 1024 * 8 and a["scan"] == 2 * 256 * 16
    assert 0 < a["rank"] <= LDS and 0 < a["scan"] <= LDS
