"""Kernel timing of the fused Y'CbCr + CICP ingest against the two kernels it replaces, on the same
images in the same run: 54 images of 768x512 and 8 of 3840x2160 into the test slot of a linear batch by
ce_batch_set_test_yuv_cicp - P010 4:2:0 BT.2020 limited range at (9, 16, depth 16) and at (9, 16, depth 10), 8-bit I420 at
(1, 13, depth 8) - and, as the yardstick, the same planes through ce_batch_set_test_yuv into a depth-16 deep batch (k_yuv)
followed by the RGB16 image that writes through ce_batch_set_test_cicp (k_tagged with cicp_px); for the 8-bit planes the
RGB8 pair of the same two.  All sources are host images: only the kernels are compared.  The phases run in the printed order with a
synchronise between them, one warm-up call first, and the last line printed is the plan as JSON:
profiles/yuv_cicp_ingest_medians.py reads it with the kernel trace and gives the per-dispatch medians of each phase.  No
counters: collect those in a run of their own.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/yuv_cicp_ingest_timing.py > out/plan.txt
    python3 profiles/yuv_cicp_ingest_medians.py out out/plan.txt"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

L = ce.lib()
rng = np.random.default_rng(1)
plan = []
with ce.Context(0) as ctx:
    for W, H, N in ((768, 512, 54), (3840, 2160, 8)):
        cw, ch = W // 2, H // 2
        y10 = (rng.integers(64, 941, (H, W)).astype(np.uint16) << 6).astype(np.uint16)
        c10 = (rng.integers(64, 961, (ch, 2 * cw)).astype(np.uint16) << 6).astype(np.uint16)
        p010 = ce.YuvImage([y10, c10], ce.YUV_420, ce.YUV_SEMIPLANAR, ce.YUV_BT2020, ce.YUV_LIMITED, ce.CHROMA_TRIANGLE, 10, True)
        y8, cb8, cr8 = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))
        i420 = ce.YuvImage([y8, cb8, cr8], ce.YUV_420, ce.YUV_PLANAR, ce.YUV_BT601, ce.YUV_FULL, ce.CHROMA_TRIANGLE, 8, False)
        rgb16 = ctx.yuv_to_rgb16(p010, W, H, 16)
        rgb8 = ctx.yuv_to_rgb8(i420, W, H)
        plan.append({"label": f"{W}x{H} setup (the yardstick's RGB images)", "kernel": "k_yuv<", "dispatches": 2, "mb": 0.0, "warmup": 2})
        b_lin = ctx.batch_linear(W, H, 1, 1)
        b_deep = ctx.batch_deep(W, H, 1, 1, 16, 16)
        b_rgb8 = ce.Batch(ctx, W, H, 1, 1)
        pq16, pq10, srgb = ce.ColourDescription(9, 16, 16, 203.0), ce.ColourDescription(9, 16, 10, 203.0), ce.ColourDescription(1, 13, 8)
        # (label, kernel in the trace, bytes per pixel the kernel must move, call)
        phases = [
            ("fused P010 (9, 16, 16)", "k_yuv_tagged< cicp_px<", 3 + 12, lambda: b_lin.set_test_yuv_cicp(0, 0, p010, pq16)),
            ("fused P010 (9, 16, 10)", "k_yuv_tagged< cicp_px<", 3 + 12, lambda: b_lin.set_test_yuv_cicp(0, 0, p010, pq10)),
            ("fused I420 (1, 13, 8)", "k_yuv_tagged< cicp_px<", 1.5 + 12, lambda: b_lin.set_test_yuv_cicp(0, 0, i420, srgb)),
            ("yardstick P010 -> deep 16 (yuv420_16_deep)", "k_yuv<", 3 + 6, lambda: b_deep.set_test_yuv(0, 0, p010)),
            ("yardstick RGB16 (9, 16, 16) (cicp_rgb16_m)", "k_tagged< cicp_px<", 6 + 12, lambda: b_lin.set_test_cicp(0, 0, rgb16, pq16)),
            ("yardstick I420 -> RGB8 (yuv420_8)", "k_yuv<", 1.5 + 3, lambda: b_rgb8.set_test_yuv(0, 0, i420)),
            ("yardstick RGB8 (1, 13, 8) (cicp_rgb8)", "k_tagged< cicp_px<", 3 + 12, lambda: b_lin.set_test_cicp(0, 0, rgb8, srgb)),
        ]
        for name, kernel, bytes_per_px, call in phases:
            call()  # first use: staging allocations, table upload, code object load
            assert L.hipDeviceSynchronize() == 0
            t = time.perf_counter()
            for _ in range(N):
                call()
            assert L.hipDeviceSynchronize() == 0
            ms = (time.perf_counter() - t) * 1e3
            mb = bytes_per_px * W * H / 1e6
            print(f"{W}x{H} {name} [{kernel}]: {N} images in {ms:.3f} ms (host clock, upload and submission included), {bytes_per_px} B/px = "
                  f"{mb:.3f} MB per dispatch")
            plan.append({"label": f"{W}x{H} {name}", "kernel": kernel, "dispatches": N + 1, "mb": mb, "warmup": 1})
        for b in (b_lin, b_deep, b_rgb8):
            b.close()
print(json.dumps(plan))
