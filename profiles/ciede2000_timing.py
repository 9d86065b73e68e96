"""Kernel timing of CIEDE2000: a batch of 6 references and 54 tests of 768x512 - RGB8 (--depth 8) or
16-bit (--depth 16) - scored by ce_batch_ciede2000 with eight thresholds, --pairs of them a call (54, or 1 for one pair alone),
and as the yardstick of the same session a linear batch of the same shape scored by ce_batch_hdr_fidelity at depth 12.  Run it
under the profiler, which times every kernel without the library's events, in a run of its own with no counters:

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o ciede2000 -- python profiles/ciede2000_timing.py --pairs 54 --depth 8
    python profiles/ciede2000_timing.py --summarise OUT --pairs 54

The first form does one warm-up call (allocations, code object load) and REPEAT timed ones of either kernel and prints the
wall time of a call; the second reads the kernel trace the profiler left under OUT and prints, per kernel, the launches, the
median and the throughput in pixels of pairs (GP/s), the last line as JSON."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

W, H, REFS, PAIRS, REPEAT = 768, 512, 6, 54, 20
F64_OPS_PER_PIXEL = 706  # counted by hand from ciede2000_pixel.h: its 40 divisions and 9 square roots as one each


def summarise(out_dir, pairs):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    per = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"]
            key = "ciede2000" if "k_ciede2000" in name else "hdr_fidelity" if "k_hdr_fidelity" in name else None
            if key:
                per.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    result = {"shape": [W, H], "pairs": pairs, "kernels": {}}
    for key, us in sorted(per.items()):
        med = statistics.median(us)
        k = {"launches": len(us), "median_us": med, "min_us": min(us), "gp_per_s": pairs * W * H / med / 1e3}
        if key == "ciede2000":
            k["f64_tops"] = k["gp_per_s"] * F64_OPS_PER_PIXEL / 1e3
        result["kernels"][key] = k
        print(f"{key}: {len(us)} launches, median {med:.2f} us, min {min(us):.2f} us, {k['gp_per_s']:.2f} GP/s")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--depth", type=int, default=8, choices=(8, 16))
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.pairs)
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
        lin = ctx.batch_linear(W, H, REFS, PAIRS)
        for i, r in enumerate(refs):
            b.set_reference(i, r)
            lin.set_reference(i, (r.astype(np.float32) / np.float32(maxv)) ** 2)
        for p, t in enumerate(tests):
            b.set_test(p, p % REFS, t)
            lin.set_test(p, p % REFS, (t.astype(np.float32) / np.float32(maxv)) ** 2)
        s = b.ciede2000(a.pairs, thresholds)  # first use
        lin.hdr_fidelity(a.pairs, 12)
        t0 = time.perf_counter()
        for _ in range(REPEAT):
            b.ciede2000(a.pairs, thresholds)
        wall = (time.perf_counter() - t0) / REPEAT
        for _ in range(REPEAT):
            lin.hdr_fidelity(a.pairs, 12)
        print(f"{a.pairs} pairs of {W}x{H} at {a.depth} bits: {wall * 1e6:.1f} us a call (wall, results on the host), "
              f"{a.pairs * W * H / wall / 1e9:.2f} GP/s; pair 0: mean {s[0].mean!r} max {s[0].max!r} dB {s[0].ciede2000_db!r}")
        b.close()
        lin.close()


if __name__ == "__main__":
    main()
