"""Kernel timing of the CIEDE2000 maps: the batch of profiles/ciede2000_timing.py - 6 references and 54
tests of 768x512, RGB8 (--depth 8) or 16-bit (--depth 16), the tests moved by up to +-10 codes (8-bit terms) so that no pixel is
skipped - through ce_batch_ciede2000_map with eight thresholds: the full map (block 1), the cell maxima of block 8, the counts
alone and one pair alone, and as the yardstick of the same process ce_batch_ciede2000 on the same batch.  Run it under the
profiler, which times every kernel without the library's events, in a run of its own with no counters:

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o ciede2000_map -- python profiles/ciede2000_map_timing.py --depth 8
    python profiles/ciede2000_map_timing.py --summarise OUT

The first form runs the phases in the order of PHASES, each as one warm-up call (allocations, code object load) and REPEAT timed
ones, and prints the wall time of a call; the second reads the kernel trace the profiler left under OUT, cuts the launches of
either kernel - in the order of their start - into the phases and prints per phase the launches, the median and the throughput
in pixels of pairs (GP/s), and the ratio of every map phase to the yardstick; the last line is JSON."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

W, H, REFS, PAIRS, REPEAT = 768, 512, 6, 54, 20
WHAT = "dh"  # any of the four: the arithmetic up to the terms is shared, and the finisher is a dozen operations
# (label, kernel, pairs) in the order the phases run
PHASES = [("yardstick scores", "k_ciede2000<", PAIRS), ("map block 1", "k_ciede2000_map<", PAIRS), ("map block 8", "k_ciede2000_map<", PAIRS),
          ("map counts only", "k_ciede2000_map<", PAIRS), ("map block 1, what = de", "k_ciede2000_map<", PAIRS),
          ("map block 1, one pair", "k_ciede2000_map<", 1), ("yardstick scores, one pair", "k_ciede2000<", 1)]


def summarise(out_dir):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    rows = []
    for f in files:
        for row in csv.DictReader(open(f)):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    result = {"shape": [W, H], "repeat": REPEAT, "phases": []}
    base = {}
    for kernel in sorted({k for _, k, _ in PHASES}):
        us = [(e - s) / 1e3 for s, e, name in rows if kernel in name]
        mine = [p for p in PHASES if p[1] == kernel]
        assert len(us) == len(mine) * (1 + REPEAT) + 1, (kernel, len(us))  # and the one launch of the closing check
        for n, (label, _, pairs) in enumerate(mine):
            timed = us[n * (1 + REPEAT) + 1:(n + 1) * (1 + REPEAT)]  # without the warm-up launch
            med = statistics.median(timed)
            result["phases"].append({"label": label, "kernel": kernel.rstrip("<"), "pairs": pairs, "launches": len(timed), "median_us": med,
                                     "min_us": min(timed), "gp_per_s": pairs * W * H / med / 1e3})
            if kernel == "k_ciede2000<":
                base[pairs] = med
    for p in result["phases"]:
        p["ratio_to_yardstick"] = p["median_us"] / base[p["pairs"]]
        print(f"{p['label']} [{p['kernel']}]: {p['launches']} launches, median {p['median_us']:.2f} us, min {p['min_us']:.2f} us, "
              f"{p['gp_per_s']:.2f} GP/s, {p['ratio_to_yardstick']:.3f} of the yardstick")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=8, choices=(8, 16))
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    import numpy as np

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import codec_eval_amd as ce

    rng = np.random.default_rng(30)
    maxv = (1 << a.depth) - 1
    dtype, spread = (np.uint8, 10) if a.depth == 8 else (np.uint16, 2570)
    thresholds = [k << 20 for k in (1, 2, 3, 5, 8, 13, 21, 34)]
    with ce.Context(0) as ctx:
        refs = [rng.integers(0, maxv + 1, (H, W, 3)).astype(dtype) for _ in range(REFS)]
        tests = [np.clip(refs[p % REFS].astype(np.int64) + rng.integers(-spread, spread + 1, (H, W, 3)), 0, maxv).astype(dtype) for p in range(PAIRS)]
        b = ce.Batch(ctx, W, H, REFS, PAIRS) if a.depth == 8 else ctx.batch_deep(W, H, REFS, PAIRS, 16, 16)
        for i, r in enumerate(refs):
            b.set_reference(i, r)
        for p, t in enumerate(tests):
            b.set_test(p, p % REFS, t)
        calls = [lambda: b.ciede2000(PAIRS, thresholds), lambda: b.ciede2000_maps(0, PAIRS, WHAT, 1, thresholds),
                 lambda: b.ciede2000_maps(0, PAIRS, WHAT, 8, thresholds), lambda: b.ciede2000_maps(0, PAIRS, WHAT, 1, thresholds, maps=False),
                 lambda: b.ciede2000_maps(0, PAIRS, "de", 1, thresholds), lambda: b.ciede2000_maps(0, 1, WHAT, 1, thresholds),
                 lambda: b.ciede2000(1, thresholds)]
        for (label, _, pairs), call in zip(PHASES, calls):
            call()  # first use
            t0 = time.perf_counter()
            for _ in range(REPEAT):
                call()
            wall = (time.perf_counter() - t0) / REPEAT
            print(f"{label}: {pairs} pairs of {W}x{H} at {a.depth} bits: {wall * 1e6:.1f} us a call (wall, results on the host), "
                  f"{pairs * W * H / wall / 1e9:.2f} GP/s")
        full, over = b.ciede2000_maps(0, 2, "de", 1, thresholds)
        s = b.ciede2000(2, thresholds)
        print("pairs 0 and 1: map sums", [int(m.astype(np.uint64).sum()) for m in full], "sum_q20", [x.sum_q20 for x in s], "over", over.tolist())
        b.close()


if __name__ == "__main__":
    main()
