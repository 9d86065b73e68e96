"""Kernel timing of the CICP ingest: 54 images of 768x512 into the test slots of a linear batch by
ce_batch_set_test_cicp at (9, 16, 10) from RGB16 - table gather, matrix, clamp - and at (1, 13, 8) from RGB8 - table only -
a float image through the CE_PIXEL_RGB_F32 upload and, as the yardstick on the same pixel count, the RGB16 image through
ingest_deep_rgb16 into a deep batch.  All sources are host images: only the kernels are compared.  The phases run in this
order with a synchronise between them.  No counters: collect those in a run of their own.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/cicp_ingest_timing.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

L = ce.lib()
rng = np.random.default_rng(1)
W, H, N = 768, 512, 54
with ce.Context(0) as ctx:
    px8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    px10 = rng.integers(0, 1024, (H, W, 3)).astype(np.uint16)
    pxf = rng.random((H, W, 3), np.float32)
    b_lin = ctx.batch_linear(W, H, 1, 2)
    b_deep = ctx.batch_deep(W, H, 1, 2, 10, 10)
    pq, srgb = ce.ColourDescription.BT2020_PQ, ce.ColourDescription.SRGB
    # (label, kernel name in the trace, bytes per pixel the kernel must move, call)
    phases = [
        ("cicp (9, 16, 10) RGB16", "cicp_rgb16_m", 6 + 12, lambda: b_lin.set_test_cicp(0, 0, px10, pq)),
        ("cicp (1, 13, 8) RGB8", "cicp_rgb8", 3 + 12, lambda: b_lin.set_test_cicp(0, 0, px8, srgb)),
        ("linear f32 upload", "ingest_linear_f32", 12 + 12, lambda: b_lin.set_test(0, 0, pxf)),
        ("ingest_deep RGB16 (yardstick)", "ingest_deep_rgb16", 6 + 6, lambda: b_deep.set_test_fmt(0, 0, px10, ce.PIXEL_RGB16)),
    ]
    for name, kernel, bytes_per_px, call in phases:
        call()  # first use: staging allocations, table upload, code object load
        assert L.hipDeviceSynchronize() == 0
        t = time.perf_counter()
        for _ in range(N):
            call()
        assert L.hipDeviceSynchronize() == 0
        ms = (time.perf_counter() - t) * 1e3
        print(f"{name} [{kernel}]: {N} images in {ms:.3f} ms (host clock, upload and submission included), {bytes_per_px} B/px = "
              f"{bytes_per_px * W * H / 1e6:.3f} MB per dispatch")
    b_lin.close(), b_deep.close()
