"""Per-kernel times of dh_merged_fold from a rocprofv3 kernel trace of tools/fold_timing.py --form device:

    rocprofv3 --kernel-trace -d DIR -- python tools/fold_timing.py --form device
    python tools/fold_kernels.py DIR [D T]

A fold's launches are those from the mg_live_rank before an mf_place to the mg_summary after it (the merge of the base,
which the tool repeats before every fold, launches the same shared kernels and is left out).  Per kernel: launches per
fold and the median over the folds of their summed duration; then the fold's span on the device (first start to last
end) and, with D and T = M + W, the bytes per second mf_rows achieves (u and v of every point read and written once)."""
import csv
import glob
import re
import statistics
import sys


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    m = re.match(r"(\w+)<([^>]*)", name)
    return (m.group(1) + "<" + m.group(2).split(",")[0] + ">") if m else name.split("(")[0]


def main():
    f = sorted(glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True))[-1]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    names = [short(r["Kernel_Name"]) for r in rows]
    folds = []
    for i, n in enumerate(names):
        if n != "mf_place":
            continue
        a = max(k for k in range(i) if names[k] == "mg_live_rank")
        b = min(k for k in range(i, len(names)) if names[k] == "mg_summary")
        folds.append((a, b))
    folds = folds[1:]  # the first is the warm-up
    per, spans = {}, []
    for a, b in folds:
        acc = {}
        for k in range(a, b + 1):
            acc.setdefault(names[k], [0, 0.0])
            acc[names[k]][0] += 1
            acc[names[k]][1] += (int(rows[k]["End_Timestamp"]) - int(rows[k]["Start_Timestamp"])) / 1e3
        for n, (c, t) in acc.items():
            per.setdefault(n, []).append((c, t))
        spans.append((int(rows[b]["End_Timestamp"]) - int(rows[a]["Start_Timestamp"])) / 1e3)
    print(f"{len(folds)} folds; device span median {statistics.median(spans):.1f} us (min {min(spans):.1f}, max {max(spans):.1f})")
    total = 0.0
    for n, v in sorted(per.items(), key=lambda kv: -statistics.median(t for _, t in kv[1])):
        med = statistics.median(t for _, t in v)
        total += med
        print(f"{n:40s} launches {v[0][0]:3d}  median {med:9.1f} us  (min {min(t for _, t in v):.1f}, max {max(t for _, t in v):.1f})")
    print(f"sum of the kernels' medians {total:.1f} us")
    if len(sys.argv) > 3 and "mf_rows" in per:
        D, T = int(sys.argv[2]), int(sys.argv[3])
        med = statistics.median(t for _, t in per["mf_rows"])
        print(f"mf_rows: {T} points x {32 * D} bytes in {med:.1f} us = {T * 32 * D / med / 1e6:.2f} TB/s")


if __name__ == "__main__":
    main()
