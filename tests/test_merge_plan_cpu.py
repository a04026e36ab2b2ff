"""What the combiner's entry points launch and where their scratch lies (dynesty_amd/csrc/merge_plan.h), held to its
invariants on the host: a stand-alone program (tests/host/merge_plan_dump.cpp, which includes only that header, built
with the address and undefined-behaviour sanitizers) walks every layout and evaluates the launch arithmetic over a grid
of shapes.  The layouts' geometry is checked, their totals against a restatement of the byte counts the entry points
reserved by hand before the layouts existed (so the arena never grows where it did not grow before), the launch
arithmetic against a restatement of the expressions it replaced, and every LDS size against the CU's 160 KB."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024
K_CHUNK, K_PART, K_HIST_BINS = 2048, 5, 16384

M_ALL = [1, 7, 2047, 2048, 2049, 524288, 524289, 2 ** 31 - 2049 - 1]  # (the last three cross scan_carry's 256-block step)
D_ALL = [1, 3, 25, 512]
RN_ALL = [(1, 1), (3, 5), (64, 2000)]
NREAL_ALL = [1, 4, 5, 64, 65, 65536]
NQ_ALL = [1, 16]
NCOL_ALL = [1, 15, 16, 78, 79, 512]
FLAGS = (0, 1)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is part of the build environment")
    exe = tmp_path_factory.mktemp("merge_plan") / "dump"
    # -x c++: the header is plain C++17 and is compiled as such, with no HIP in sight; a program of its own, so the
    # sanitizers' runtime is linked in and nothing is preloaded.  Host code only: -fno-gpu-sanitize says so outright
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                           "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "dynesty_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "host", "merge_plan_dump.cpp")])

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


def nblk_of(M):
    return ceil_div(M, K_CHUNK)


# ---- the parent's expressions (the library before the layouts: one 2561-line merge.hip) -------------------------------
def parent_moment_chunks(M, cols):
    n = min(ceil_div(M, 2048), 1024, (8 << 20) // (cols or 1))
    n = max(n, 1)
    chunk = ceil_div(M, n)
    return ceil_div(M, chunk), chunk


def parent_merged(M, D, pt):  # carve_merged, as it stood
    sizes = [8 * M] * 8 + [8 * M * D] * 2 + [8 * (3 + D)] + [4 * M] * 4 + ([4 * M] * 3 if pt else [])
    return sum(al(s) for s in sizes)


def parent_scratch(M, R, N, D):  # carve_scratch, as it stood
    nchunk = parent_moment_chunks(M, D + 2)[0]
    sizes = [8 * (R + 1), 8 * R] + [8 * M] * 6 + [8 * nchunk * (D + 2), 8, 64] + [4 * M] * 3 + [4 * R * N, 16, 8,
                                                                                                  (nblk_of(M) + 1) * 16]
    return sum(al(s) for s in sizes)


def parent_stage(R, N, D, S1):  # dh_merge_runs
    return (R * S1 + R * N) * (8 + 8 * D + 12) + 16 * 256


def parent_gather(n, D):  # dh_merged_gather
    return n * (8 * D + 8) + 1024


def parent_hist(two, n, nbx, nby):  # run_hist (1-D: nby = 0)
    total = n * (nbx * nby if two else nbx)
    return total * 16 + n * (nbx + nby + 2) * 8 + (2 * n if two else n) * 4 + 8 * 256


def parent_quantile(nq, ncol):  # dh_merged_quantile
    return ncol * nq * (256 * 8 + 64) + ncol * 32 + 32 * 256


def parent_real(M, D, nreal, mean, kld):  # realize_core
    tile = min(nreal, 64)
    return (M * 2 + tile * nblk_of(M) * (1 + K_PART + (D if mean else 0) + (1 if kld else 0)) + nreal * (3 + D)) * 8 + 18 * 256


def parent_fields(M):  # dh_merged_realization
    return M * 7 * 8 + (nblk_of(M) + 1) * 16 + 18 * 256


def parent_boot(M, S, D, cap, fields, mean):  # boot_carve
    nblk, nbx = nblk_of(max(M, cap)), nblk_of(cap)
    return (S * 4 + M * 8 + 64 + (nblk + 1) * 16 + cap * 16 +
            (cap * 48 if fields else (nbx * (2 + K_PART + (D if mean else 0)) + 4 + D) * 8) + 27 * 256)


def parent_tie_scratch(M):  # boot_ties
    return (nblk_of(M) + 1) * 16 + 1024


def parent_weights(M):  # weights_enqueue
    return M * 16 + (nblk_of(M) + 1) * 16 + 8 * 256


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


def walk(dump, requests, bound, unwanted=lambda r: (), exact=False):
    for req, lay in zip(requests, dump(requests)):
        check_geometry(req, lay, unwanted(req))
        ref = bound(req)
        assert lay["total"] == ref if exact else lay["total"] <= ref, (req, lay["total"], ref)
    return len(requests)


def test_merged_run_and_merge_scratch_equal_the_parent(dump):
    reqs = [("merged", M, D, pt) for M, D, pt in itertools.product(M_ALL, D_ALL, FLAGS)]
    walk(dump, reqs, lambda r: parent_merged(r[1], r[2], r[3]), lambda r: () if r[3] else ("id", "it", "nc"), exact=True)
    reqs = [("scratch", M, R, N, D) for M, (R, N), D in itertools.product(M_ALL, RN_ALL, D_ALL)]
    walk(dump, reqs, lambda r: parent_scratch(*r[1:]), exact=True)


def test_arena_layouts_stay_inside_the_parent_reserves(dump):
    pt_only = ("dead_id", "dead_it", "dead_nc", "live_it")
    reqs = [("stage", R, N, D, S, pt) for (R, N), D, S, pt in itertools.product(RN_ALL, D_ALL, (1, 7, 100, 30000), FLAGS)]
    n = walk(dump, reqs, lambda r: parent_stage(*r[1:5]), lambda r: () if r[5] else pt_only)
    reqs = [("gather", k, D, given) for k, D, given in itertools.product((1, 7, 4097, 8388607 // 512), D_ALL, FLAGS)]
    n += walk(dump, reqs, lambda r: parent_gather(r[1], r[2]), lambda r: () if r[3] else ("idx",))
    reqs = [("hist", 0, k, nb, 0) for k, nb in itertools.product(NCOL_ALL, (1, 7, 100, 4096))]
    reqs += [("hist", 1, k, nbx, nby) for k, (nbx, nby) in itertools.product((1, 7, 300, 65536), ((1, 1), (7, 3), (128, 128), (1, 16384)))]
    n += walk(dump, reqs, lambda r: parent_hist(*r[1:]), lambda r: () if r[1] else ("ye",))
    reqs = [("real", M, D, nreal, rwt, mean, kld)
            for M, D, nreal, rwt, mean, kld in itertools.product(M_ALL, D_ALL, NREAL_ALL, FLAGS, FLAGS, FLAGS)]
    n += walk(dump, reqs, lambda r: parent_real(r[1], r[2], r[3], r[5], r[6]),
              lambda r: [nm for nm, on in (("rwt", r[4]), ("mpart", r[5]), ("kpart", r[6])) if not on])
    reqs = [("fields", M, rwt, kld) for M, rwt, kld in itertools.product(M_ALL, FLAGS, FLAGS)]
    n += walk(dump, reqs, lambda r: parent_fields(r[1]), lambda r: [nm for nm, on in (("rwt", r[2]), ("kld", r[3])) if not on])
    n += walk(dump, [("tie_scratch", M) for M in M_ALL], lambda r: parent_tie_scratch(r[1]))
    n += walk(dump, [("weights", M) for M in M_ALL], lambda r: parent_weights(r[1]))
    print(f"{n} layouts")


def test_bootstrap_buffer_in_both_forms_first_and_regrown(dump):
    batch_only, fields_only = ("sums", "partr", "mpart", "out", "kpart"), ("step", "logvol", "logwt", "logz", "kld", "wide")
    reqs = []
    for M, (R, N), D, fields, mean in itertools.product(M_ALL, RN_ALL, D_ALL, FLAGS, FLAGS):
        first = M + M // 4 + K_CHUNK
        for Mx in (first + 1, 3 * M + 5):  # what the regrow rule makes of an M' the first carve cannot hold
            reqs += [("boot", M, R * N, D, cap, fields, mean) for cap in (first, Mx + Mx // 4 + K_CHUNK)]
    arith = dump([("arith", M, 1, 1, 1, 1, 1, 1) for M in M_ALL])
    for M, a in zip(M_ALL, arith):
        assert a["cap_first"] == a["cap_regrown"] == M + M // 4 + K_CHUNK  # the parent's `cap`, at M and at M'
    walk(dump, reqs, lambda r: parent_boot(*r[1:]),
         lambda r: batch_only if r[5] else fields_only + (() if r[6] else ("mpart",)))


def test_quantile_layout_and_its_zeroed_block(dump):
    reqs = [("quantile", nq, ncol) for nq, ncol in itertools.product(NQ_ALL, NCOL_ALL)]
    walk(dump, reqs, lambda r: parent_quantile(r[1], r[2]))
    for req, lay in zip(reqs, dump(reqs)):
        z0, zb = lay["zero"]
        slots = {s[0]: s for s in lay["slots"]}
        inside = ["table", "total", "cmax", "last", "flags"]  # next to each other, cleared by one memset
        assert z0 == slots["table"][1] and z0 + zb == slots["cmin"][1] <= lay["total"], req
        for name, off, nbytes, _ in lay["slots"]:
            assert (z0 <= off and off + nbytes <= z0 + zb) == (name in inside), (req, name)
        S = req[1] * req[2]
        assert [slots[k][2] for k in inside] == [S * 256 * 8, 8, req[2] * 8, req[2] * 4, 16], req


def test_own_allocations(dump):
    """The tie structure and the covariance workspace are allocations of their own: the parent's byte counts plus at
    most the alignment of their two arrays."""
    reqs = [("ties", M, R * N) for M, (R, N) in itertools.product(M_ALL, RN_ALL)]
    for req, lay in zip(reqs, dump(reqs)):
        check_geometry(req, lay)
        assert (req[1] + 1 + req[2]) * 4 <= lay["total"] < (req[1] + 1 + req[2]) * 4 + 2 * 256
    reqs = [("cov", M, D) for M, D in itertools.product(M_ALL, D_ALL)]
    for req, lay in zip(reqs, dump(reqs)):
        check_geometry(req, lay)
        parent = (parent_moment_chunks(req[1], req[2] ** 2)[0] + 1) * req[2] ** 2 * 8
        assert parent <= lay["total"] < parent + 2 * 256


def test_launch_arithmetic_equals_the_parent(dump):
    reqs = [("arith", M, D, nreal, nq, ncol, n, nb)
            for M, D, nreal, (nq, ncol), (n, nb) in itertools.product(
                M_ALL, D_ALL, NREAL_ALL, itertools.product(NQ_ALL, NCOL_ALL), ((1, 1), (15, 100), (512, 4096), (3, 16384), (65536, 49)))]
    for (_, M, D, nreal, nq, ncol, n, nb), a in zip(reqs, dump(reqs)):
        assert (a["nchunk1"], a["chunk1"]) == parent_moment_chunks(M, D + 2)
        assert (a["nchunk2"], a["chunk2"]) == parent_moment_chunks(M, D * D)
        rows = max(ceil_div(M, 2048), 256)
        assert (a["rows"], a["groups"]) == (rows, ceil_div(M, rows))
        cpt = 78 // nq
        tile_cols = min(cpt, ncol)
        tile_sel = tile_cols * nq
        assert a["cpt"] == cpt
        assert a["lds_digit"] == tile_sel * (256 * 8 + 16) + tile_cols * 4
        assert a["lds_succ"] == tile_sel * (8 + 16) + tile_cols * 4
        assert a["combine"] == (1 if tile_cols < 16 else 0)
        per = min(K_HIST_BINS // nb, 1024)
        assert a["per"] == per and a["lds_hist"] == min(per, n) * nb * 8
        assert a["lds_int"] == 2 * 256 * 3 * 8 and a["lds_int_mean"] == (2 * 256 * 3 + 4 * 2048 + 8 * 4 * 32) * 8
        assert a["tile"] == min(nreal, 64)
        assert a["cap_first"] == M + M // 4 + 2048 and a["nblk"] == nblk_of(M)
        # the moment sums: at most 1024 chunks and 64 MB of partial sums, every point in exactly one chunk
        for nchunk, chunk, cols in ((a["nchunk1"], a["chunk1"], D + 2), (a["nchunk2"], a["chunk2"], D * D)):
            assert 1 <= nchunk <= 1024 and nchunk * cols * 8 <= 64 << 20
            assert (nchunk - 1) * chunk < M <= nchunk * chunk
        assert a["groups"] <= 2048 and (a["groups"] - 1) * a["rows"] < M <= a["groups"] * a["rows"]


def test_every_lds_size_fits_a_cu(dump):
    """Over all arguments the entry points admit: nq 1..16, ncol 1..512; 1-D bins up to 4096 for up to 512 columns; 2-D
    bins up to kHistBins for up to 65536 pairs; the integrals with and without means."""
    reqs = [("arith", 1, 1, 1, nq, ncol, 1, 1) for nq in range(1, 17) for ncol in range(1, 513)]
    for req, a in zip(reqs, dump(reqs)):
        assert 0 < a["lds_succ"] <= a["lds_digit"] <= LDS, req
        assert a["cpt"] * req[4] <= 78 and a["cpt"] >= 1, req
    bins = sorted(set([1, 2, 3, 15, 16, 17, 100, 1024, 4095, 4096]))
    reqs = [("arith", 1, 1, 1, 1, 1, n, nb) for n in (1, 2, 3, 4, 5, 16, 511, 512) for nb in bins]
    bins2 = sorted(set(bins + [4097, 8191, 8192, 8193, 16383, 16384] + [x * y for x in (1, 7, 127, 128) for y in (1, 3, 128)]))
    reqs += [("arith", 1, 1, 1, 1, 1, n, nb) for n in (1, 2, 3, 1023, 1024, 1025, 65536) for nb in bins2]
    for req, a in zip(reqs, dump(reqs)):
        assert 1 <= a["per"] <= 1024 and a["per"] * req[7] <= K_HIST_BINS, req
        assert 0 < a["lds_hist"] <= K_HIST_BINS * 8 <= LDS, req
        assert a["lds_int"] <= a["lds_int_mean"] <= LDS, req
