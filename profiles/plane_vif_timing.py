"""Timing of VIFp on a decoder's planes on section 32's workload: 6 references and 54 tests of 768x512
4:2:0, 8 bits, as I420 planes on the host, scored by ce_yuv_plane_vif, with ce_yuv_plane_hvs at step 8 and
ce_yuv_plane_fidelity at levels 1 on the same images, in the same session, as the yardsticks: k_plane_level's level 0 filters the
same five streams with 11 taps where the scale-1 stats kernel has 17.  Kernel times come from the profiler, in a run of its
own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o vif -- python profiles/plane_vif_timing.py
    python profiles/plane_vif_timing.py --summarise OUT

The first form does one warm-up call of each kind (allocations, code object load) and REPEAT timed ones and prints the wall
time of a call (take that figure from a run with the profiler off); the second reads the kernel trace the profiler left under
OUT and prints, per kernel, the launches and the time of a call beside the yardsticks', the last line as JSON."""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

W, H, REFS, PAIRS, REPEAT = 768, 512, 6, 54, 20
CW, CH = W // 2, H // 2


def kernel_key(name):
    """the trace's kernel name, demangled or not -> k_vif_stats_17 ... / k_plane_level / k_plane_hvs / k_plane_sse, or None"""
    m = re.search(r"k_vif_(stats|reduce)(?:<|ILi)(\d+)", name)
    if m:
        return f"k_vif_{m.group(1)}_{m.group(2)}"
    for key in ("k_plane_level", "k_plane_hvs", "k_plane_sse", "k_plane_pool"):
        if key in name:
            return key
    return None


def summarise(out_dir, pairs):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    rows = []
    for f in files:
        rows += [r for r in csv.DictReader(open(f)) if kernel_key(r["Kernel_Name"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    samples = pairs * (W * H + 2 * CW * CH)
    result = {"shape": [W, H], "pairs": pairs, "kernels": {}}
    by_key = {}
    for r in rows:
        by_key.setdefault(kernel_key(r["Kernel_Name"]), []).append(us(r))
    for key, t in sorted(by_key.items()):
        assert len(t) % (REPEAT + 1) == 0, (key, len(t))  # every call of a kind makes the same launches
        a_call = len(t) // (REPEAT + 1)
        timed = t[a_call:]  # without the warm-up call
        result["kernels"][key] = {"launches_a_call": a_call, "us_a_call": sum(timed) / REPEAT, "ns_a_sample": sum(timed) / REPEAT * 1e3 / samples}
        print(f"{key}: {a_call} launches a call, {sum(timed) / REPEAT:.1f} us a call, {sum(timed) / REPEAT * 1e3 / samples:.5f} ns a sample")
    k = result["kernels"]
    vif = sum(v["us_a_call"] for name, v in k.items() if name.startswith("k_vif_"))
    print(f"ce_yuv_plane_vif's kernels together: {vif:.1f} us a call")
    if "k_vif_stats_17" in k and "k_plane_level" in k:
        result["stats_17_over_plane_level_0"] = k["k_vif_stats_17"]["us_a_call"] / k["k_plane_level"]["us_a_call"]
        print(f"k_vif_stats<17> / k_plane_level level 0: {result['stats_17_over_plane_level_0']:.3f} (tap count alone: {17 / 11:.3f})")
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

    rng = np.random.default_rng(31)

    def smooth(shape):
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        v = 0.5 + 0.35 * np.sin(xx / 9.0 + rng.random() * 6.0) * np.cos(yy / 7.0) + 0.1 * np.sin((xx + yy) / 31.0)
        return np.clip(np.rint(v * 255 + rng.normal(0, 0.02 * 255, shape)), 0, 255).astype(np.uint8)

    def timed(what, call):
        s = call()  # first use
        t0 = time.perf_counter()
        for _ in range(REPEAT):
            call()
        print(f"{what}: {a.pairs} pairs of {W}x{H} 4:2:0: {(time.perf_counter() - t0) / REPEAT * 1e6:.1f} us a call (wall, results on the host)")
        return s

    with ce.Context(0) as ctx:
        shapes = ((H, W), (CH, CW), (CH, CW))
        refs = [[smooth(s) for s in shapes] for _ in range(REFS)]
        tests = [[np.clip(np.rint(p.astype(np.float64) + rng.normal(0, 4.0, p.shape)), 0, 255).astype(np.uint8) for p in refs[i % REFS]] for i in range(a.pairs)]
        image = lambda p: ce.YuvImage(list(p), subsampling=ce.YUV_420, depth=8)  # noqa: E731
        ri, ti, table = [image(p) for p in refs], [image(p) for p in tests], [i % REFS for i in range(a.pairs)]
        s = timed("plane_vif", lambda: ctx.plane_vif(ri, ti, W, H, pair_ref=table))
        print(f"pair 0: n_pos {s[0].n_pos[0]} vifp {s[0].vifp!r} luma's scales {s[0].vif_scale[0]!r}")
        timed("plane_hvs step 8", lambda: ctx.plane_hvs(ri, ti, W, H, pair_ref=table, step=8))
        timed("plane_fidelity levels 1", lambda: ctx.plane_fidelity(ri, ti, W, H, pair_ref=table, levels=1))


if __name__ == "__main__":
    main()
