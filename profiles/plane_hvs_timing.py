"""Timing of PSNR-HVS / PSNR-HVS-M on a decoder's planes on section 28's workload: 6 references and 54
tests of 768x512 4:2:0 scored by ce_yuv_plane_hvs at steps 8 and 7, as 8-bit I420 planes on the host (--mode host8) or as
10-bit P010 surfaces on the device (--mode dev10), with ce_yuv_plane_fidelity at levels 0 and 1 on the same images as the
yardsticks: k_plane_sse reads the same bytes, k_plane_level's level 0 filters the same samples.  Kernel times come from the
profiler, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o hvs -- python profiles/plane_hvs_timing.py --mode dev10
    python profiles/plane_hvs_timing.py --summarise OUT --mode dev10

The first form does one warm-up call of each kind (allocations, code object load) and REPEAT timed ones and prints the wall
time of a call (take that figure from a run with the profiler off); the second reads the kernel trace the profiler left under
OUT and prints, per kernel, the launches and the time of a call and k_plane_hvs's time per sample and per DCT block beside the
yardsticks', the last line as JSON."""
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
STEPS = (8, 7)


def blocks(step):
    n = lambda w, h: ((w - 8) // step + 1) * ((h - 8) // step + 1)  # noqa: E731
    return n(W, H) + 2 * n(CW, CH)


def summarise(out_dir, mode, pairs):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    rows = []
    for f in files:
        rows += [r for r in csv.DictReader(open(f)) if any(k in r["Kernel_Name"] for k in ("k_plane_hvs", "k_plane_sse", "k_plane_level"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    # the run's order: per step REPEAT + 1 calls of one k_plane_hvs launch each, step 8 first; then the two yardsticks
    hvs = [us(r) for r in rows if "k_plane_hvs" in r["Kernel_Name"]]
    assert len(hvs) == len(STEPS) * (REPEAT + 1), len(hvs)
    result = {"shape": [W, H], "mode": mode, "pairs": pairs, "kernels": {}}
    samples = pairs * (W * H + 2 * CW * CH)
    for i, step in enumerate(STEPS):
        t = hvs[i * (REPEAT + 1) + 1:(i + 1) * (REPEAT + 1)]
        med = statistics.median(t)
        result["kernels"][f"k_plane_hvs_step{step}"] = {"median_us": med, "ns_a_sample": med * 1e3 / samples, "ns_a_block": med * 1e3 / (pairs * blocks(step))}
        print(f"k_plane_hvs step {step}: median {med:.1f} us a call, {med * 1e3 / samples:.5f} ns a sample, {med * 1e3 / (pairs * blocks(step)):.3f} ns a DCT block "
              f"({pairs * blocks(step)} blocks)")
    for key in ("k_plane_sse", "k_plane_level"):
        t = [us(r) for r in rows if key in r["Kernel_Name"]]
        if not t:
            continue
        calls = (REPEAT + 1) * (2 if key == "k_plane_sse" else 1)  # the SSE kernel runs at levels 0 and 1
        result["kernels"][key] = {"launches_a_call": len(t) / calls, "us_a_call": sum(t) / calls, "ns_a_sample": sum(t) / calls * 1e3 / samples}
        print(f"{key}: {len(t) / calls:.1f} launches a call, {sum(t) / calls:.1f} us a call, {sum(t) / calls * 1e3 / samples:.5f} ns a sample")
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
        for step in STEPS:
            s = ctx.plane_hvs(ri, ti, W, H, pair_ref=table, step=step)  # first use
            t0 = time.perf_counter()
            for _ in range(REPEAT):
                ctx.plane_hvs(ri, ti, W, H, pair_ref=table, step=step)
            wall = (time.perf_counter() - t0) / REPEAT
            print(f"{a.mode}, step {step}: {a.pairs} pairs of {W}x{H} 4:2:0: {wall * 1e6:.1f} us a call (wall, results on the host); "
                  f"pair 0: blocks {s[0].n_blocks} psnr_hvs {s[0].psnr_hvs!r} psnr_hvsm {s[0].psnr_hvsm!r}")
        for levels in (0, 1):
            ctx.plane_fidelity(ri, ti, W, H, pair_ref=table, levels=levels)
            t0 = time.perf_counter()
            for _ in range(REPEAT):
                ctx.plane_fidelity(ri, ti, W, H, pair_ref=table, levels=levels)
            wall = (time.perf_counter() - t0) / REPEAT
            print(f"{a.mode}, plane_fidelity levels {levels}: {wall * 1e6:.1f} us a call (wall)")


if __name__ == "__main__":
    main()
