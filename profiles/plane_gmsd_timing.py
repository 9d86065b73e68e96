"""Timing of GMSD on a decoder's planes on section 28's workload: 6 references and 54 tests of 768x512
4:2:0 scored by ce_yuv_plane_gmsd, as 8-bit I420 planes on the host (--mode host8) or as 10-bit P010 surfaces on the device
(--mode dev10), with ce_yuv_plane_fidelity at levels 0 on the same images as the yardstick: k_plane_sse reads the same bytes
and is what a streaming kernel over these planes costs.  Kernel times come from the profiler, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o gmsd -- python profiles/plane_gmsd_timing.py --mode dev10
    python profiles/plane_gmsd_timing.py --summarise OUT --mode dev10

The first form does one warm-up call of each kind (allocations, code object load) and REPEAT timed ones and prints the wall
time of a call (take that figure from a run with the profiler off); the second reads the kernel trace the profiler left under
OUT and prints the medians of k_plane_gmsd and k_plane_sse, their ratio and the time per sample and per position, the last
line as JSON."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

W, H, REFS, PAIRS, REPEAT = 768, 512, 6, 54, 20
CW, CH = W // 2, H // 2


def summarise(out_dir, mode, pairs):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    rows = []
    for f in files:
        rows += [r for r in csv.DictReader(open(f)) if any(k in r["Kernel_Name"] for k in ("k_plane_gmsd", "k_plane_sse"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    samples = pairs * (W * H + 2 * CW * CH)
    result = {"shape": [W, H], "mode": mode, "pairs": pairs, "kernels": {}}
    for key in ("k_plane_gmsd", "k_plane_sse"):
        # REPEAT + 1 calls of one launch each: the first is the warm-up
        t = [us(r) for r in rows if key in r["Kernel_Name"]]
        assert len(t) == REPEAT + 1, (key, len(t))
        med = statistics.median(t[1:])
        result["kernels"][key] = {"median_us": med, "min_us": min(t[1:]), "ns_a_sample": med * 1e3 / samples}
        print(f"{key}: median {med:.1f} us a call (min {min(t[1:]):.1f}), {med * 1e3 / samples:.5f} ns a sample")
    g, s = result["kernels"]["k_plane_gmsd"], result["kernels"]["k_plane_sse"]
    g["ns_a_position"] = g["median_us"] * 1e3 / (samples / 4)
    result["gmsd_over_sse"] = g["median_us"] / s["median_us"]
    print(f"k_plane_gmsd / k_plane_sse: {result['gmsd_over_sse']:.2f}; {g['ns_a_position']:.5f} ns a position ({samples // 4} positions)")
    print(json.dumps(result))


class DeviceCopy:
    def __init__(self, lib, a):
        self.lib, self.ptr = lib, C.c_void_p()
        assert lib.hipMalloc(C.byref(self.ptr), C.c_size_t(a.nbytes)) == 0
        assert lib.hipMemcpy(self.ptr, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0

    def __del__(self):
        self.lib.hipFree(self.ptr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("host8", "dev10"), default="host8")
    ap.add_argument("--pairs", type=int, default=PAIRS)
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.mode, a.pairs)
    import numpy as np

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import codec_eval_amd as ce

    rng = np.random.default_rng(31)
    depth = 8 if a.mode == "host8" else 10
    L, dt = (1 << depth) - 1, np.uint8 if depth == 8 else np.uint16
    keep = []

    def image(planes):
        y, cb, cr = planes
        if a.mode == "host8":
            return ce.YuvImage([y, cb, cr], subsampling=ce.YUV_420, depth=8)
        uv = np.empty((CH, 2 * CW), np.uint16)
        uv[:, 0::2], uv[:, 1::2] = cb, cr
        bufs = [DeviceCopy(ce.lib(), np.ascontiguousarray(p << 6)) for p in (y, uv)]  # P010: the value in the top ten bits
        keep.append(bufs)
        return ce.YuvImage([b.ptr.value for b in bufs], ce.YUV_420, ce.YUV_SEMIPLANAR, depth=10, msb_aligned=True, memory=ce.MEM_DEVICE,
                           pitches=[2 * W, 4 * CW])

    def smooth(shape):
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
        v = 0.5 + 0.35 * np.sin(xx / 9.0 + rng.random() * 6.0) * np.cos(yy / 7.0) + 0.1 * np.sin((xx + yy) / 31.0)
        return np.clip(np.rint(v * L + rng.normal(0, 0.02 * L, shape)), 0, L).astype(dt)

    with ce.Context(0) as ctx:
        shapes = ((H, W), (CH, CW), (CH, CW))
        refs = [[smooth(s) for s in shapes] for _ in range(REFS)]
        tests = [[np.clip(np.rint(p.astype(np.float64) + rng.normal(0, 4.0 * L / 255, p.shape)), 0, L).astype(dt) for p in refs[i % REFS]] for i in range(a.pairs)]
        ri, ti, table = [image(p) for p in refs], [image(p) for p in tests], [i % REFS for i in range(a.pairs)]
        s = ctx.plane_gmsd(ri, ti, W, H, pair_ref=table)  # first use
        t0 = time.perf_counter()
        for _ in range(REPEAT):
            ctx.plane_gmsd(ri, ti, W, H, pair_ref=table)
        wall = (time.perf_counter() - t0) / REPEAT
        print(f"{a.mode}: {a.pairs} pairs of {W}x{H} 4:2:0: {wall * 1e6:.1f} us a call (wall, results on the host); "
              f"pair 0: n_pos {s[0].n_pos} gmsd {s[0].gmsd!r} gmsm {s[0].gmsm!r} max_dis {s[0].max_dis}")
        ctx.plane_fidelity(ri, ti, W, H, pair_ref=table, levels=0)
        t0 = time.perf_counter()
        for _ in range(REPEAT):
            ctx.plane_fidelity(ri, ti, W, H, pair_ref=table, levels=0)
        wall = (time.perf_counter() - t0) / REPEAT
        print(f"{a.mode}, plane_fidelity levels 0: {wall * 1e6:.1f} us a call (wall)")


if __name__ == "__main__":
    main()
