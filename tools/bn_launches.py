"""BatchNorm-family launches of the steady-state steps of a rocprofv3 kernel trace (the CSV tools/trace_gaps.py reads): per
(kernel, grid) the launches per step and the mean / min duration, and the family's total per step.

    python tools/bn_launches.py <dir>/t_kernel_trace.csv
"""
import collections
import csv
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
ends = [i for i, r in enumerate(rows) if "sgd_multi_kernel" in r["Kernel_Name"]]
skip = 4
rs = rows[ends[skip] + 1:ends[-1] + 1]
steps = len(ends) - 1 - skip
tab = collections.defaultdict(list)
for r in rs:
    n = r["Kernel_Name"]
    if "bn_" not in n:
        continue
    n = n.replace("(anonymous namespace)::", "").replace("void ", "")
    for stop in "(":
        if stop in n:
            n = n[:n.index(stop)]
    grid = "x".join(str(r.get(k, "?")) for k in ("Grid_Size_X", "Grid_Size_Y") if k in r) or str(r.get("Grid_Size", "?"))
    tab[(n, grid)].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
print(f"{steps} steps; kernel, grid (work-items), launches per step, mean us, min us, ms per step")
tot = collections.defaultdict(float)
for (n, grid), d in sorted(tab.items(), key=lambda kv: (kv[0][0], -sum(kv[1]))):
    print(f"  {n:44s} {grid:14s} {len(d) / steps:6.1f} {sum(d) / len(d) / 1e3:9.1f} {min(d) / 1e3:9.1f} {sum(d) / steps / 1e6:8.3f}")
    tot[n] += sum(d) / steps / 1e6
print("per kernel, ms per step:")
for n, t in sorted(tot.items(), key=lambda kv: -kv[1]):
    print(f"  {t:8.3f}  {n}")
print(f"  {sum(tot.values()):8.3f}  BatchNorm family")
