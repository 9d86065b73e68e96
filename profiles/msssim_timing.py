"""Kernel timing of SSIM / MS-SSIM: an RGB8 batch of 6 references and 54 tests of 768x512 scored by
ce_batch_msssim with five levels, --pairs of them a call (54, or 1 for one pair alone).  Run it under the profiler, which
times every kernel without the library's events:

    rocprofv3 --kernel-trace --stats -d OUT -o msssim -- python profiles/msssim_timing.py --pairs 54
    python profiles/msssim_timing.py --summarise OUT --pairs 54

The first form does one warm-up call (allocations, code object load) and REPEAT timed ones and prints the wall time of a call;
the second reads the kernel trace the profiler left under OUT and prints, per msssim kernel, the launches, the median and the
total of a call, and the throughput in level-0 pixels of pairs (GP/s), the last line as JSON."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

W, H, REFS, PAIRS, REPEAT = 768, 512, 6, 54, 20


def summarise(out_dir, pairs):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    per = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"]
            if "msssim" in name:
                key = ("level" if "level" in name else "pool") + ("_u8" if "Ih" in name or "unsigned char" in name else "_f32")
                per.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    calls = REPEAT + 1
    result = {"shape": [W, H], "pairs": pairs, "calls": calls, "kernels": {}}
    total = 0.0
    for key, us in sorted(per.items()):
        a_call = sum(us) / calls
        total += a_call
        result["kernels"][key] = {"launches_a_call": len(us) / calls, "median_us": statistics.median(us), "us_a_call": a_call}
        print(f"{key}: {len(us) / calls:.1f} launches a call, median {statistics.median(us):.2f} us, {a_call:.1f} us a call")
    result["us_a_call"] = total
    result["gp_per_s"] = pairs * W * H / total / 1e3
    print(f"all msssim kernels: {total:.1f} us a call of {pairs} pairs, {result['gp_per_s']:.2f} GP/s")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.pairs)
    import numpy as np

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import codec_eval_amd as ce

    rng = np.random.default_rng(27)
    with ce.Context(0) as ctx:
        refs = [rng.integers(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(REFS)]
        tests = [np.clip(refs[p % REFS].astype(np.int64) + rng.integers(-10, 11, (H, W, 3)), 0, 255).astype(np.uint8) for p in range(PAIRS)]
        b = ce.Batch(ctx, W, H, REFS, PAIRS)
        for i, r in enumerate(refs):
            b.set_reference(i, r)
        for p, t in enumerate(tests):
            b.set_test(p, p % REFS, t)
        s = b.ms_ssim(a.pairs)  # first use
        t0 = time.perf_counter()
        for _ in range(REPEAT):
            b.ms_ssim(a.pairs)
        wall = (time.perf_counter() - t0) / REPEAT
        print(f"{a.pairs} pairs of {W}x{H}: {wall * 1e6:.1f} us a call (wall, results on the host), {a.pairs * W * H / wall / 1e9:.2f} GP/s; "
              f"pair 0: ssim {s[0].ssim!r} ms_ssim {s[0].ms_ssim!r}")
        b.close()


if __name__ == "__main__":
    main()
