"""Timing of the plane-domain scores: 6 references and 54 tests of 768x512 4:2:0 scored by
ce_yuv_plane_fidelity, as 8-bit I420 planes on the host (--mode host8) or as 10-bit P010 surfaces on the device (--mode dev10),
--pairs of them a call (54, or 1 for one pair alone), and as the yardstick the existing k_psnr_sse on an RGB8 batch whose images
hold as many bytes as one image's planes.  Kernel times come from the profiler, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o plane -- python profiles/plane_fidelity_timing.py --mode dev10 --pairs 54
    python profiles/plane_fidelity_timing.py --summarise OUT --mode dev10 --pairs 54

The first form does one warm-up call (allocations, code object load) and REPEAT timed ones of levels = 0, of levels = 5 and of
the batch's PSNR and prints the wall time of a call (take that figure from a run with the profiler off); the second reads the
kernel trace the profiler left under OUT and prints, per kernel, the launches and the time of a call, the bytes the SSE kernels
must read over their time beside k_psnr_sse's, and the level kernels' time per level-0 position, the last line as JSON."""
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
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # MI355X: the data sheet's peak and a measured float4 copy, bytes a second


def summarise(out_dir, mode, pairs):
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + out_dir
    per = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"]
            for key in ("k_plane_sse", "k_plane_level", "k_plane_pool", "k_psnr_sse"):
                if key in name:
                    kind = "_u8" if ("Ih" in name or "Li1" in name or "unsigned char" in name or "<1>" in name) else \
                           "_u16" if ("It" in name or "Li2" in name or "unsigned short" in name or "<2>" in name) else "_f32" if "plane" in key else ""
                    per.setdefault(key + kind, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    bps = 1 if mode == "host8" else 2
    image_bytes = (W * H + 2 * CW * CH) * bps
    result = {"shape": [W, H], "mode": mode, "pairs": pairs, "kernels": {}}
    for key, us in sorted(per.items()):
        # the SSE kernels run in the calls of levels = 0 and of levels = 5, the others in those of levels = 5 or of the batch
        calls = (REPEAT + 1) * (2 if "plane_sse" in key else 1)
        result["kernels"][key] = {"launches_a_call": len(us) / calls, "median_us": statistics.median(us), "us_a_call": sum(us) / calls}
        print(f"{key}: {len(us) / calls:.1f} launches a call, median {statistics.median(us):.2f} us, {sum(us) / calls:.1f} us a call")
    k = result["kernels"]
    sse = next((v for n, v in k.items() if n.startswith("k_plane_sse")), None)
    if sse:
        rate = pairs * 2 * image_bytes / (sse["us_a_call"] * 1e-6)
        result["sse_bytes_per_s"] = rate
        print(f"plane SSE: {pairs * 2 * image_bytes} bytes a call, {rate / 1e9:.0f} GB/s = {100 * rate / HBM_SPEC:.1f} % of the HBM peak "
              f"({100 * rate / HBM_COPY:.1f} % of a measured copy)")
    yard = next((v for n, v in k.items() if n.startswith("k_psnr_sse")), None)
    if yard:
        rate = pairs * 2 * image_bytes / (yard["us_a_call"] * 1e-6)
        result["psnr_sse_bytes_per_s"] = rate
        print(f"k_psnr_sse on {image_bytes}-byte RGB8 images: {rate / 1e9:.0f} GB/s = {100 * rate / HBM_SPEC:.1f} % of the HBM peak")
    lv = next((v for n, v in k.items() if n.startswith("k_plane_level") and not n.endswith("f32")), None)
    if lv:
        positions = pairs * ((W - 10) * (H - 10) + 2 * (CW - 10) * (CH - 10))
        result["level0_ns_per_position"] = lv["us_a_call"] * 1e3 / positions
        print(f"level 0 of the three planes: {positions} positions a call, {result['level0_ns_per_position']:.4f} ns a position")
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

    rng = np.random.default_rng(28)
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

    with ce.Context(0) as ctx:
        shapes = ((H, W), (CH, CW), (CH, CW))
        refs = [[rng.integers(0, L + 1, s).astype(dt) for s in shapes] for _ in range(REFS)]
        tests = [[np.clip(p.astype(np.int64) + rng.integers(-10, 11, p.shape), 0, L).astype(dt) for p in refs[i % REFS]] for i in range(a.pairs)]
        ri, ti, table = [image(p) for p in refs], [image(p) for p in tests], [i % REFS for i in range(a.pairs)]
        for levels in (0, 5):
            s = ctx.plane_fidelity(ri, ti, W, H, pair_ref=table, levels=levels)  # first use
            t0 = time.perf_counter()
            for _ in range(REPEAT):
                ctx.plane_fidelity(ri, ti, W, H, pair_ref=table, levels=levels)
            wall = (time.perf_counter() - t0) / REPEAT
            print(f"{a.mode}, levels {levels}: {a.pairs} pairs of {W}x{H} 4:2:0: {wall * 1e6:.1f} us a call (wall, results on the host); "
                  f"pair 0: psnr {s[0].psnr!r} ms_ssim {s[0].ms_ssim!r}")
        # the yardstick: k_psnr_sse on RGB8 images of as many bytes as one image's planes (a third of them pixels)
        px = (W * H + 2 * CW * CH) * (1 if depth == 8 else 2) // 3
        bw, bh = (512, px // 512)
        assert bw * bh == px
        b = ce.Batch(ctx, bw, bh, REFS, a.pairs)
        for i in range(REFS):
            b.set_reference(i, rng.integers(0, 256, (bh, bw, 3)).astype(np.uint8))
        for p in range(a.pairs):
            b.set_test(p, p % REFS, rng.integers(0, 256, (bh, bw, 3)).astype(np.uint8))
        cfg = ce.MetricConfig(psnr=True)
        b.run(a.pairs, cfg)
        t0 = time.perf_counter()
        for _ in range(REPEAT):
            b.run(a.pairs, cfg)
        wall = (time.perf_counter() - t0) / REPEAT
        print(f"batch PSNR of {a.pairs} pairs of {bw}x{bh} RGB8 ({bw * bh * 3} bytes an image): {wall * 1e6:.1f} us a launch and collect (wall)")
        b.close()


if __name__ == "__main__":
    main()
