"""Per-dispatch medians of the resamplers' kernels from a rocprofv3 kernel trace of profiles/resample_linear_timing.py:
    python3 profiles/resample_linear_medians.py OUT_DIR
One line per (kernel, grid) in order of first dispatch: a call resamples the reference slab (6 images) and the test slab (54)
in separate dispatches, and the script runs two target shapes, so every kernel shows four grids."""
import csv
import glob
import os
import re
import statistics
import sys

rows = {}
for path in glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if "resample" not in r["Kernel_Name"]:
                continue
            name = re.search(r"k_resample\w*(<\w+>)?", r["Kernel_Name"]).group(0)
            key = (name, int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r["Grid_Size"]))
            rows.setdefault(key, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
for (name, grid), v in sorted(rows.items(), key=lambda kv: min(t for t, _ in kv[1])):
    d = sorted(dur for _, dur in v)
    print(f"{name:28s} grid {grid:10d}  n {len(d):3d}  median {statistics.median(d) / 1e3:9.2f} us  min {d[0] / 1e3:9.2f}  max {d[-1] / 1e3:9.2f}")
