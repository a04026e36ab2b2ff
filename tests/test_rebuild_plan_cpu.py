"""What the rebuild launches and where its scratch lies (dynesty_amd/csrc/rebuild_plan.h), held to its invariants on
the host: a stand-alone program (tests/host/rebuild_plan_dump.cpp, which includes only that header) prints the plan
and the scratch layout of every shape of a grid, and the grids, chunks, LDS sizes and offsets are checked against the
co-residency rules, against a restatement of the launcher's formulas as they stood before the plan was split off, and
against the launches recorded on an MI355X (tests/golden/rebuild_launches.json)."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_BYTES = 64  # sizeof(Node) of rebuild.hip: 11 ints, padding, 2 doubles
ERR_ARG = -6
K_LDS_LIMIT = 159 * 1024

RUNS = [1, 3, 64, 128, 144, 160, 256]
SHAPES = [(9, 2), (300, 1), (2400, 2), (5000, 2), (2000, 5), (2000, 13), (2000, 14), (2000, 25), (900, 30), (900, 31),
          (1200, 44), (65536, 4)]
# (num_cu, occ_root, occ_split, occ_tree): DESIGN 3.3 / tests/test_codegen_budget.py pin 2 / 5 / 2 on the MI355X's 256 CUs
CAPS = [(256, 2, 5, 2), (256, 1, 1, 1), (8, 2, 5, 2)]
DEFAULT_SW = dict(fast=1, deep=1, deep_from=-1, root_parts=1, wave_ell=1)
SWITCHES = [DEFAULT_SW] + [dict(DEFAULT_SW, **kv) for kv in (dict(deep=0), dict(deep_from=0), dict(deep_from=1),
                                                             dict(deep_from=3), dict(fast=0), dict(root_parts=0),
                                                             dict(wave_ell=0))]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is part of the build environment")
    exe = tmp_path_factory.mktemp("rebuild_plan") / "dump"
    # -x c++: the header is plain C++17 and is compiled as such, with no HIP in sight
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "dynesty_amd", "csrc"),
                           "-o", str(exe), os.path.join(ROOT, "tests", "host", "rebuild_plan_dump.cpp")])
    return str(exe)


def case(runs, n, d, mode, caps=CAPS[0], pct=87, coop=0, sw=DEFAULT_SW, max_ells=None):
    if max_ells is None:
        max_ells = max(1, n // (2 * d)) if mode == 0 else 1
    return dict(runs=runs, n=n, d=d, mode=mode, max_ells=max_ells, caps=caps, pct=pct, coop=coop, sw=sw)


def run_dump(exe, cases):
    inp = "".join("{runs} {n} {d} {mode} {max_ells} {nb} {c[0]} {c[1]} {c[2]} {c[3]} {pct} {coop} {s[fast]} {s[deep]} "
                  "{s[deep_from]} {s[root_parts]} {s[wave_ell]}\n".format(nb=NODE_BYTES, c=c["caps"], s=c["sw"], **c)
                  for c in cases)
    out = subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    return [json.loads(line) for line in out]


@pytest.fixture(scope="module")
def grid(dump):
    cases = [case(runs, n, d, mode, caps, pct, coop, sw)
             for runs, (n, d), mode, caps, pct, coop, sw in itertools.product(RUNS, SHAPES, (0, 1), CAPS, (87, 40), (0, 1),
                                                                              SWITCHES)]
    return cases, run_dump(dump, cases)


# ---- the launcher's formulas as they stood in rebuild_launch_full before the split (the reference) ----
def lds_base(D, TP):
    LD = D | 1
    return ((TP * LD + 4 * D * LD + 7 * D + 2 + 256 + 128) * 8 + (320 + D + 8) * 4 + 15) & ~15


def lds_common(D, TP=256):
    P = (D + 1) & ~1
    base, jb = lds_base(D, TP), 4 * P * (P | 1) * 8
    return base if base + jb > 79 * 1024 else base + jb


def lds_split(D, TP):
    return ((TP * (D | 1) + 5 * D + 2 + 256 + 128) * 8 + (320 + D + 8) * 4 + 15) & ~15


def lds_wave(D):
    return ((128 * (D | 1) + 4 * D * (D | 1) + 2 * D + 64) * 8 + 15) & ~15


def parent_scalars(c):
    """The scalars, caps and the root's parts (rebuild_launch_full at the parent commit)."""
    runs, n, d, mode, sw = c["runs"], c["n"], c["d"], c["mode"], c["sw"]
    num_cu, occ_root, occ_split, occ_tree = c["caps"]
    s = dict(max_nodes=1 if mode == 1 else n // d + 3, maxw=n // (4 * d) + 1)
    s["reslist_cap"] = s["max_nodes"] * 24 + 64
    lv = 4
    while (1 << lv) < n // (2 * d) + 1:
        lv += 1
    s["levels"] = 0 if mode == 1 else 2 * lv + 8
    s["tps"] = 256 if lds_split(d, 256) * 5 <= K_LDS_LIMIT else 128
    s["maxp"] = n // s["tps"] + s["maxw"] + 1
    s["fast"] = 1 if mode == 0 and sw["fast"] != 0 else 0
    nlev = s["levels"]
    if s["fast"] and sw["deep"] != 0:
        nlev = min(s["levels"], lv)
    if s["fast"] and 0 <= sw["deep_from"] < s["levels"]:
        nlev = sw["deep_from"]
    s["nlev"] = nlev
    s["tail"] = 1 if s["fast"] and nlev < s["levels"] else 0
    s["tree_from"] = nlev if s["tail"] else s["levels"] + 1
    s["kp_cap"] = s["levels"] * (n // s["tps"] + 1) + 8 if s["tail"] else 0
    s["tq_cap"] = runs * (2 * s["max_nodes"] + s["levels"] * (n // s["tps"] + 1) + 8) if s["tail"] else 0
    s["cap_root"], s["cap_split_level"] = num_cu * occ_root, num_cu * occ_split
    s["cap_tree"] = num_cu * occ_tree if s["tail"] else 0
    s["cap_split"] = min(s["cap_split_level"], s["cap_tree"]) if s["tail"] else s["cap_split_level"]
    rp = (n + 255) // 256 if n > 1 else 1
    if rp > s["cap_root"] or (c["coop"] and runs * rp > s["cap_root"]):
        rp = 1
    if sw["root_parts"] == 0:
        rp = 1
    s["rp"] = rp
    s["rootbuf_stride"] = 2 * (rp * (2 * d + d * d + 1) + d * d + 8)
    return s


def parent_layout(c, s):
    """The b_* sizes and the hand-out order of the parent's launcher: (name, offset, bytes) per array, and the total."""
    runs, n, d, mode, max_ells = c["runs"], c["n"], c["d"], c["mode"], c["max_ells"]
    levels, maxw, maxp, max_nodes, tail, fast = s["levels"], s["maxw"], s["maxp"], s["max_nodes"], s["tail"], s["fast"]
    NS = d + 3 * d * d + d + d * (d | 1)
    n_cnt_old = runs * (3 * levels + 5 + levels * maxw * 16)
    n_cnt_tree = runs + 64 + runs * max_nodes * 16 + 2 * s["tq_cap"] + 2 if tail else 0
    b = [("perm", runs * n * 4), ("perm2", runs * n * 4), ("lab", runs * n), ("nodes", runs * max_nodes * NODE_BYTES),
         ("estore", runs * max_nodes * NS * 8), ("reslist", runs * s["reslist_cap"] * 4),
         ("counters", (n_cnt_old + n_cnt_tree) * 4), ("split_list", 2 * runs * maxw * 4),
         ("ell_list", max(levels, 1) * runs * 2 * maxw * 4), ("scale_g", runs * d * 8),
         ("pts_scaled", 0 if mode == 1 else runs * n * d * 8), ("part_list", 2 * runs * maxp * 2 * 4),
         ("part_base", 2 * runs * maxw * 4), ("kpart", 0 if mode == 1 else 2 * runs * maxp * (2 * d + 2) * 16),
         ("kpart_tail", 2 * runs * s["kp_cap"] * (2 * d + 2) * 16 if tail else 0),
         ("rootbuf", runs * s["rootbuf_stride"] * 8), ("fin_lse", runs * max_nodes * 8), ("fin_int", runs * max_nodes * 2 * 4),
         ("out_node", runs * max_ells * 4 if fast else 0), ("out_fast", runs * max_ells * 4 if fast else 0),
         ("root_eig", runs * (2 * d * d + d + 2) * 8 if fast else 0)]
    out, off = [], 0
    for name, nbytes in b:
        out.append([name, off, nbytes])
        off += (nbytes + 255) & ~255
    cnt = dict(nnodes=0, nsplit=runs, nell=runs + (levels + 1) * runs)
    cnt["nparts"] = cnt["nell"] + levels * runs
    cnt["kerr"] = cnt["nparts"] + (levels + 1) * runs
    cnt["kbar"] = cnt["kerr"] + runs
    if tail:
        cnt["kp_top"] = n_cnt_old
        cnt["tq_ctl"] = cnt["kp_top"] + runs
        cnt["nbar"] = cnt["tq_ctl"] + 64
        q = cnt["nbar"] + runs * max_nodes * 16
        cnt["tq_items"] = q + (q & 1)  # (the block starts on a 256-byte boundary: an odd int offset is 4 mod 8)
    return out, off, cnt


UNWANTED = {"pts_scaled": lambda c, s: c["mode"] == 1, "kpart": lambda c, s: c["mode"] == 1,
            "kpart_tail": lambda c, s: not s["tail"], "out_node": lambda c, s: not s["fast"],
            "out_fast": lambda c, s: not s["fast"], "root_eig": lambda c, s: not s["fast"]}
COUNTER_ORDER = ["nnodes", "nsplit", "nell", "nparts", "kerr", "kbar", "kp_top", "tq_ctl", "nbar", "tq_items"]


def check_plan(c, p):
    runs, n, d, mode = c["runs"], c["n"], c["d"], c["mode"]
    num_cu = c["caps"][0]
    s = parent_scalars(c)
    parts = (n + s["tps"] - 1) // s["tps"]
    if mode == 0 and parts > s["cap_split"]:  # the documented DH_ERR_ARG: a node's parts cannot be resident together
        assert p["rc"] == ERR_ARG and "co-resident workgroups of k_split" in p["err"], (c, p)
        return 0
    assert p["rc"] == 0, (c, p)
    for k, v in s.items():
        assert p[k] == v, (c, k, p[k], v)
    # ---- root ----
    rp_full = (n + 255) // 256 if n > 1 else 1
    chunks = [min(p["root_chunk"], runs - r0) for r0 in range(0, runs, p["root_chunk"])]
    assert p["root_chunk"] >= 1 and sum(chunks) == runs  # every run exactly once
    if p["rp"] > 1:
        assert p["root_chunk"] * p["rp"] <= s["cap_root"], (c, p["rp"], p["root_chunk"])
    else:
        assert p["root_chunk"] == runs
    if c["coop"] and runs * rp_full > s["cap_root"]:
        assert p["rp"] == 1
    if rp_full > s["cap_root"]:
        assert p["rp"] == 1
    assert p["rp"] in (1, rp_full)
    # ---- LDS ----
    assert p["lds"] == lds_common(d) and p["lds_split"] == lds_split(d, p["tps"]) and p["lds_wave"] == lds_wave(d)
    assert max(p["lds"], p["lds_split"], p["lds_top"], p["lds_fin"]) <= K_LDS_LIMIT
    assert (p["tps"] == 256) == (5 * lds_split(d, 256) <= K_LDS_LIMIT) == (d <= 13)
    if d > 30 or mode == 1:
        assert p["lds_top"] == 0
    # (the 512-point tile fits up to D = 29: at D = 30 the padded row is 31 doubles, 120 bytes past the limit)
    assert p["lds_top"] == (lds_common(d, 512) if mode == 0 and lds_common(d, 512) <= K_LDS_LIMIT else 0)
    assert (p["lds_top"] > 0) == (mode == 0 and d <= 29)
    if p["fin_extra_off"]:
        assert p["fin_extra_off"] % 16 == 0 and p["fin_extra_off"] >= p["lds"]
        assert p["lds_fin"] == p["fin_extra_off"] + p["max_nodes"] * NODE_BYTES + (p["reslist_cap"] * 4 if p["fin_res_lds"] else 0)
    else:
        assert p["lds_fin"] == p["lds"] and not p["fin_res_lds"]
    # ---- the levels ----
    assert len(p["level"]) == p["nlev"] <= 2 * 16 + 8
    room = s["cap_split_level"] * c["pct"] // 100
    for L, l in enumerate(p["level"]):
        assert l["gp"] == min(p["maxp"], n // p["tps"] + 2 ** L + 1), (c, L, l)
        assert l["cr"] >= 1 and (l["cr"] * l["gp"] <= room or l["cr"] == 1), (c, L, l, room)
        assert l["nchunk"] * l["cr"] >= runs and l["nchunk"] * l["cr"] - runs < l["nchunk"], (c, L, l)
        assert l["ge"] == min(2 * p["maxw"], 2 ** (L + 1))
        assert 1 <= l["ge_l"] <= l["ge"] and l["ge_l"] == min(l["ge"], max(1, 8 * 2 * num_cu // runs)), (c, L, l)
        assert 1 <= l["gw_l"] <= l["ge"] and l["gw_l"] == min(l["ge"], max(1, 16384 // runs)), (c, L, l)
        assert l["g_ell"] == (l["ge_l"] if p["fast"] else l["ge"])  # the slow form: the worst case
        assert bool(l["top"]) == (p["lds_top"] > 0 and (n >> (L + 1)) > 256 and 2 * runs * l["ge"] <= num_cu), (c, L, l)
        assert (l["tp"], l["lds_ell"]) == ((512, p["lds_top"]) if l["top"] else (256, p["lds"]))
        assert l["lds_ell"] <= K_LDS_LIMIT
        wave = bool(p["fast"] and c["sw"]["wave_ell"] and 8 * p["lds_wave"] <= K_LDS_LIMIT and
                    (n >> (L + 1)) <= 256)  # from the level where the average child fits two wavefront tiles
        assert bool(l["wave"]) == wave and (not wave or p["lds_wave"] <= K_LDS_LIMIT), (c, L, l)
    if p["tail"]:
        assert 1 <= p["g_tree"] <= s["cap_tree"]
        assert p["g_tree"] == min(s["cap_tree"], runs * (n // p["tps"] + 2 * p["maxw"] + 1))
    assert p["g_out"] == min(c["max_ells"], 8)
    # ---- the scratch layout ----
    ref_slots, ref_total, ref_cnt = parent_layout(c, s)
    assert p["slots"] == ref_slots and p["total"] == ref_total, (c, p["slots"], ref_slots)
    end, last = 0, -1
    for name, off, nbytes in p["slots"]:
        assert off % 256 == 0 and off >= end, (c, name)  # aligned, in list order, no overlap
        if nbytes:
            assert off > last, (c, name)  # strictly increasing among the arrays that take room
            last = off
        end = off + nbytes
        if name in UNWANTED and UNWANTED[name](c, s):
            assert nbytes == 0, (c, name)
        else:
            assert nbytes > 0, (c, name)
    assert p["total"] == (end + 255) & ~255
    k = p["counters"]
    names = COUNTER_ORDER if p["tail"] else COUNTER_ORDER[:6]
    offs = [k[nm] for nm in names]
    assert offs == sorted(offs) and offs[0] == 0, (c, k)  # the documented order
    assert len(set(offs)) == len(offs) or p["levels"] == 0, (c, k)  # (Ellipsoid.update: no levels, empty per-level counters)
    assert {nm: k[nm] for nm in names} == ref_cnt, (c, k, ref_cnt)
    cnt_bytes = dict((nm, nb) for nm, _, nb in p["slots"])["counters"]
    assert cnt_bytes == 4 * k["ints"]
    if p["tail"]:
        assert k["tq_items"] % 2 == 0 and k["tq_items"] + 2 * p["tq_cap"] <= k["ints"]  # 8-byte items, inside the block
    else:
        assert k["kbar"] + p["levels"] * runs * p["maxw"] * 16 <= k["ints"]
    return 1


def test_grid_invariants_and_parent_layout(grid):
    cases, plans = grid
    ok = sum(check_plan(c, p) for c, p in zip(cases, plans))
    print(f"{len(cases)} shapes, {ok} plans, {len(cases) - ok} documented argument errors")
    assert ok > len(cases) // 2 and ok < len(cases)


def test_fixed_points(dump):
    """From the project's record (EXPERIMENTS R6.5): the bench rebuild is six level pairs and the tail with
    128-point parts and an eight-part root in one launch; 128 runs x 8 parts go as two chunks of 64, 144 as 64 + 64 + 16."""
    p64, p128, p144 = run_dump(dump, [case(r, 2000, 25, 0) for r in (64, 128, 144)])
    assert (p64["tps"], p64["nlev"], p64["tail"], p64["rp"], p64["root_chunk"]) == (128, 6, 1, 8, 64)
    assert p64["tree_from"] == 6 and len(p64["level"]) == 6
    assert (p128["rp"], p128["root_chunk"]) == (8, 64)
    assert (p144["rp"], p144["root_chunk"]) == (8, 64)
    assert [min(64, 144 - r0) for r0 in range(0, 144, p144["root_chunk"])] == [64, 64, 16]


def test_argument_errors(dump):
    bad = [(case(1, 1 << 20, 2048, 1), "d=2048 is beyond the narrow path"),  # (the launcher sends D > 44 to the wide path first)
           (case(1, 1 << 27, 16, 1), "n x d = 2147483648 elements per run exceeds 2^31"),
           (case(1, 1 << 27, 16, 0), "n x d = 2147483648 elements per run exceeds 2^31"),  # before the limit on n
           (case(1, 65537, 4, 0), "MultiEllipsoid.update supports at most 65536 points per run (n = 65537)"),
           (case(1, 2000, 25, 2, max_ells=1), "bad arguments (n=2000 d=25 mode=2)"),
           (case(1, 2000, 25, -1, max_ells=1), "bad arguments (n=2000 d=25 mode=-1)"),
           (case(1, 0, 25, 0, max_ells=1), "bad arguments (n=0 d=25 mode=0)"),
           (case(1, 2000, 0, 0, max_ells=1), "bad arguments (n=2000 d=0 mode=0)"),
           (case(1, 2000, 25, 0, max_ells=0), "bad arguments (n=2000 d=25 mode=0)")]
    for (c, text), p in zip(bad, run_dump(dump, [c for c, _ in bad])):
        assert p["rc"] == ERR_ARG and p["err"] == "rebuild: " + text, (c, p)
    ok = run_dump(dump, [case(1, 65536, 4, 0), case(1, 65537, 4, 1), case(1, (1 << 27) - 1, 16, 1)])
    assert [p["rc"] for p in ok] == [0, 0, 0]


def launches_of(c, p):
    """The launch sequence of one rebuild as rebuild_launch_full enqueues it: (kernel, workgroups, block)."""
    runs = c["runs"]
    main = [["k_root_parts", min(p["root_chunk"], runs - r0) * p["rp"], 256] for r0 in range(0, runs, p["root_chunk"])]
    ell = "k_ell<false, true>" if p["fast"] and p["tail"] else "k_ell<false, false>" if p["fast"] else "k_ell<true, false>"
    for l in p["level"]:
        main.append(["k_split", l["nchunk"] * l["cr"] * l["gp"], 256])
        if l["wave"]:
            main.append(["k_ell_wave", runs * l["gw_l"], 64])
        main.append([ell, runs * l["g_ell"], 256])
    if p["tail"]:
        main.append(["k_tree", p["g_tree"], 256])
    main.append(["k_finish", runs, 256])
    if p["fast"]:
        main.append(["k_out_eig", runs * p["g_out"], 256])
    return main, ([["k_root_eig", runs, 256]] if p["fast"] else [])


def test_plan_reproduces_the_recorded_launches(dump):
    """tests/golden/rebuild_launches.json: the rebuild kernels of a kernel trace taken on an MI355X with the library
    as it stood BEFORE the plan was split off, per shape and switch setting; the caps that go with it are in the file."""
    with open(os.path.join(ROOT, "tests", "golden", "rebuild_launches.json")) as f:
        gold = json.load(f)
    caps = tuple(gold["caps"][k] for k in ("num_cu", "occ_root", "occ_split", "occ_tree"))
    cases = [case(g["runs"], g["n"], g["d"], g["mode"], caps, g["split_resident_pct"], g["coop_launch"],
                  dict(DEFAULT_SW, **g["switches"]), g["max_ells"]) for g in gold["cases"]]
    assert len(cases) >= 20
    for g, c, p in zip(gold["cases"], cases, run_dump(dump, cases)):
        assert p["rc"] == 0, (c, p)
        main, side = launches_of(c, p)
        assert main == g["main"], (c, main, g["main"])
        assert side == g["side"], (c, side, g["side"])
