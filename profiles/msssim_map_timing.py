"""Kernel timing of the SSIM / MS-SSIM maps on section 27's workload: an RGB8 batch of 6 references and
54 tests of 768x512, at level 0 of five.  --modes lists what the calls ask for, in the order they run: `score` is
ce_batch_msssim itself, for the score kernel's time in the same session; `map1` the block-1 map, `map16` the cell maxima of
block 16, `counts` eight exceedance counts and no map.  --pairs lists how many pairs a call takes (54, or 1 for one pair alone).
Run it under the profiler, which times every kernel without the library's events, in a run of its own:

    rocprofv3 --kernel-trace --stats -d OUT -o maps -- python profiles/msssim_map_timing.py --modes score,map1,map16,counts --pairs 54
    python profiles/msssim_map_timing.py --summarise OUT --modes score,map1,map16,counts --pairs 54

The first form does, per mode, one warm-up call (allocations, code object load) and --repeat timed ones and prints the wall
time of a call.  The second reads the kernel trace the profiler left under OUT: the launches of k_msssim_level_map<u8> in the
order they started fall into one run of 1 + repeat per map mode, in the order of --modes; it prints the median of each run
without its warm-up beside the median of k_msssim_level<u8>, and their ratios, the last line as JSON."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

W, H, REFS, PAIRS, REPEAT = 768, 512, 6, 54, 20
THR = [0, (1 << 32) // 100, (1 << 32) // 20, (1 << 32) // 10, (1 << 32) // 5, 3 * ((1 << 32) // 10), (1 << 32) // 2, (1 << 32) - 1]
MODES = {"map1": dict(block=1), "map16": dict(block=16), "counts": dict(thresholds_q32=THR, maps=False)}


def summarise(out_dir, modes, pairs, repeat):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, "one kernel trace expected under " + out_dir
    assert len(pairs) == 1, "summarise one profiled run: one --pairs"
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    u8 = lambda name: "Ih" in name or "unsigned char" in name  # noqa: E731  level 0 reads the u8 slabs
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    maps = [us(r) for r in rows if "k_msssim_level_map" in r["Kernel_Name"] and u8(r["Kernel_Name"])]
    score = [us(r) for r in rows if "k_msssim_level" in r["Kernel_Name"] and "level_map" not in r["Kernel_Name"] and u8(r["Kernel_Name"])]
    map_modes = [m for m in modes if m != "score"]
    assert len(maps) == len(map_modes) * (repeat + 1), (len(maps), map_modes, repeat)
    result = {"shape": [W, H], "pairs": pairs[0], "repeat": repeat, "median_us": {}, "ratio_to_score": {}}
    if score:
        result["median_us"]["k_msssim_level<u8>"] = statistics.median(score[1:])
        print(f"k_msssim_level<u8>: {len(score)} launches, median {statistics.median(score[1:]):.2f} us")
    for i, m in enumerate(map_modes):
        run = maps[i * (repeat + 1) + 1:(i + 1) * (repeat + 1)]
        result["median_us"][m] = statistics.median(run)
        line = f"k_msssim_level_map<u8> {m}: {len(run)} launches, median {statistics.median(run):.2f} us (min {min(run):.2f}, max {max(run):.2f})"
        if score:
            result["ratio_to_score"][m] = statistics.median(run) / statistics.median(score[1:])
            line += f", {result['ratio_to_score'][m]:.3f} of the score kernel"
        print(line)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default=str(PAIRS), help="pairs a call, a comma-separated list")
    ap.add_argument("--modes", default="score,map1,map16,counts", help="a comma-separated list of score, " + ", ".join(sorted(MODES)))
    ap.add_argument("--repeat", type=int, default=REPEAT, help="timed calls a mode; a block-1 map of 54 pairs is 246 MB to the host a call")
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    modes, pairs = a.modes.split(","), [int(p) for p in a.pairs.split(",")]
    assert all(m == "score" or m in MODES for m in modes), modes
    if a.summarise:
        return summarise(a.summarise, modes, pairs, a.repeat)
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
        for n in pairs:
            for mode in modes:
                call = (lambda: b.ms_ssim(n)) if mode == "score" else (lambda: b.ms_ssim_maps(0, n, 5, 0, "ssim", **MODES[mode]))
                call()  # first use
                t0 = time.perf_counter()
                for _ in range(a.repeat):
                    call()
                wall = (time.perf_counter() - t0) / a.repeat
                print(f"{mode}: {n} pairs of {W}x{H}: {wall * 1e6:.1f} us a call (wall, results on the host), {n * W * H / wall / 1e9:.2f} GP/s")
        b.close()


if __name__ == "__main__":
    main()
