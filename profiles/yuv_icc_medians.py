"""Per-dispatch medians of profiles/yuv_icc_timing.py's phases from rocprofv3's kernel trace.
usage: yuv_icc_medians.py TRACE_DIR PLAN.txt - TRACE_DIR is searched for *kernel_trace.csv; PLAN.txt is the timing script's
output, whose last line is the plan: the phases in order, each with the kernel it dispatches - the words that all occur in its
name in the trace - how often, and the labels of the phases whose kernels it replaces.  The dispatches of a kernel are taken
in start order and dealt to the phases in plan order, the warm-up ones dropped (profiles/icc_ingest_medians.py's rule).  Prints
one line per phase: median microseconds with min .. max and GB/s against the bytes the script printed; then, for every fused
phase, the sum of the medians it replaces, with the sum of their minima and of their maxima as the run's own spread."""
import csv
import glob
import json
import os
import statistics
import sys

trace_dir, plan_path = sys.argv[1], sys.argv[2]
plan = json.loads(open(plan_path).read().strip().splitlines()[-1])
rows = []
for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
queues = {p["kernel"]: [(s, e) for s, e, name in rows if all(word in name for word in p["kernel"].split())] for p in plan}
stats = {}
for phase in plan:
    q = queues[phase["kernel"]]
    mine, queues[phase["kernel"]] = q[:phase["dispatches"]], q[phase["dispatches"]:]
    assert len(mine) == phase["dispatches"], (phase, len(mine))
    us = [(e - s) / 1e3 for s, e in mine[phase["warmup"]:]]
    med = statistics.median(us)
    stats[phase["label"]] = (med, min(us), max(us))
    print(f"{phase['label']}: median {med:.2f} us over {len(us)} dispatches (min {min(us):.2f}, max {max(us):.2f}), "
          f"{phase['mb'] / med * 1e3:.1f} GB/s of {phase['mb']:.3f} MB")
for k, left in queues.items():
    assert not left, (k, len(left))
for phase in plan:
    if phase["replaces"]:
        med, lo, hi = stats[phase["label"]]
        parts = [stats[label] for label in phase["replaces"]]
        total, tlo, thi = (sum(p[k] for p in parts) for k in range(3))
        print(f"{phase['label']}: {med:.2f} us (min {lo:.2f}, max {hi:.2f}) against {total:.2f} us for the {len(parts)} it replaces "
              f"(sum of minima {tlo:.2f}, of maxima {thi:.2f}): {med / total:.2f} x")
