"""Kernel timing of the alpha compositor: one 768x512 RGBA8 image into the test slots of a resident
batch over K = 1 and K = 2 backgrounds (54 dispatches each), 250 images of 512x512 over K = 2, an RGBA16 image into a deep
10 / 10 batch over K = 2 and, as the yardstick on the same pixel counts, the same images through ingest_rgba8 (alpha
dropped).  All sources are host images: only the kernels are compared.  The phases run in this order with a synchronise
between them, so the dispatches of one kernel name split by start time.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/alpha_timing.py"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

L = ce.lib()
rng = np.random.default_rng(1)
with ce.Context(0) as ctx:
    big8 = rng.integers(0, 256, (512, 768, 4), dtype=np.uint8)
    big16 = rng.integers(0, 1024, (512, 768, 4)).astype(np.uint16)
    sq8 = rng.integers(0, 256, (512, 512, 4), dtype=np.uint8)
    bw8, bw10 = np.array(ce.ALPHA_BLACK_WHITE), np.array([(0, 0, 0), (1023, 1023, 1023)])
    b_big = ce.Batch(ctx, 768, 512, 1, 2)
    b_deep = ce.Batch(ctx, 768, 512, 1, 2, depths=(10, 10))
    b_sq = ce.Batch(ctx, 512, 512, 1, 2)
    # (label, dispatches, pixels, bytes per pixel the kernel must move, call)
    phases = [
        ("alpha_rgba8 768x512 K=1", 54, 768 * 512, 4 + 3, lambda: b_big.set_test_over(0, [0], big8, ce.PIXEL_RGBA8, bw8[:1])),
        ("alpha_rgba8 768x512 K=2", 54, 768 * 512, 4 + 6, lambda: b_big.set_test_over(0, [0, 0], big8, ce.PIXEL_RGBA8, bw8)),
        ("ingest_rgba8 768x512", 54, 768 * 512, 4 + 3, lambda: b_big.set_test_fmt(0, 0, big8, ce.PIXEL_RGBA8)),
        ("alpha_rgba16_deep 768x512 K=2", 54, 768 * 512, 8 + 12, lambda: b_deep.set_test_over(0, [0, 0], big16, ce.PIXEL_RGBA16, bw10)),
        ("ingest_deep_rgba16 768x512", 54, 768 * 512, 8 + 6, lambda: b_deep.set_test_fmt(0, 0, big16, ce.PIXEL_RGBA16)),
        ("alpha_rgba8 512x512 K=2", 250, 512 * 512, 4 + 6, lambda: b_sq.set_test_over(0, [0, 0], sq8, ce.PIXEL_RGBA8, bw8)),
        ("ingest_rgba8 512x512", 250, 512 * 512, 4 + 3, lambda: b_sq.set_test_fmt(0, 0, sq8, ce.PIXEL_RGBA8)),
    ]
    for name, n, px, bytes_per_px, call in phases:
        call()  # first use: staging allocations, code object load
        assert L.hipDeviceSynchronize() == 0
        t = time.perf_counter()
        for _ in range(n):
            call()
        assert L.hipDeviceSynchronize() == 0
        ms = (time.perf_counter() - t) * 1e3
        print(f"{name}: {n} images in {ms:.3f} ms (host clock, upload and submission included), {bytes_per_px} B/px = "
              f"{bytes_per_px * px / 1e6:.3f} MB per dispatch")
    b_big.close(), b_deep.close(), b_sq.close()
