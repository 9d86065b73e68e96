"""Kernel timing of linear-light compositing: 768x512 RGBA8 and RGBA16 images into the test slots of a
linear batch by ce_batch_set_test_cicp_over over 1, 2 and 8 backgrounds (k_tagged_over with cicp_px), the float frame
(k_linear_over) over the same, and beside them, from the same run, the plain launch of the same format and pixel (k_tagged
with cicp_px, alpha dropped) and section 14's integer composite (k_alpha into an RGB8 and a deep batch) over 1, 2 and 8
backgrounds.  The pixel is BT.2020 PQ for the 16-bit source (depth 10) and Display P3 sRGB for the 8-bit one, both with the
primaries matrix.  The phases run in the printed order with a synchronise between them, one warm-up call first, and the last
line printed is the plan as JSON in the form profiles/icc_ingest_medians.py reads.  No counters: collect those in a run of
their own.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/alpha_linear_timing.py > out/plan.txt
    python3 profiles/icc_ingest_medians.py out out/plan.txt"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import codec_eval_amd as ce  # noqa: E402

L = ce.lib()
rng = np.random.default_rng(1)
plan = []
W, H, N = 768, 512, 48  # 48 test slots: six calls over eight backgrounds fill them

with ce.Context(0) as ctx:
    rgba8 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    rgba16 = rng.integers(0, 1024, (H, W, 4)).astype(np.uint16)
    rgba16[..., 3] = rng.integers(0, 1024, (H, W))
    f32 = rng.random((H, W, 4), np.float32)
    p3, pq = ce.ColourDescription(12, 13, 8, 203.0), ce.ColourDescription(9, 16, 10, 203.0)
    lin, b8, deep = ctx.batch_linear(W, H, 8, N), ce.Batch(ctx, W, H, 8, N), ctx.batch_deep(W, H, 8, N, 10, 10)
    bg_lin = rng.random((8, 3), np.float32)
    bg8, bg10 = rng.integers(0, 256, (8, 3)), rng.integers(0, 1024, (8, 3))
    # (label, kernel in the trace: every word is in its name, bytes per pixel the kernel must move, call number i)
    phases = [
        ("yardstick plain cicp RGBA8 -> linear slot", "k_tagged<1, cicp_px<true>", 4 + 12, lambda i: lin.set_test_cicp(i % N, 0, rgba8, p3)),
        ("yardstick plain cicp RGBA16 -> linear slot", "k_tagged<5, cicp_px<true>", 8 + 12, lambda i: lin.set_test_cicp(i % N, 0, rgba16, pq)),
    ]
    for n in (1, 2, 8):
        refs = list(range(n))
        at = lambda i, n=n: (i * n) % (N - n + 1)
        phases += [
            (f"over cicp RGBA8 x {n} backgrounds", "k_tagged_over<1, cicp_px<true>", 4 + 12 * n,
             lambda i, n=n, refs=refs, at=at: lin.set_test_cicp_over(at(i), refs, rgba8, p3, bg_lin[:n])),
            (f"over cicp RGBA16 x {n} backgrounds", "k_tagged_over<5, cicp_px<true>", 8 + 12 * n,
             lambda i, n=n, refs=refs, at=at: lin.set_test_cicp_over(at(i), refs, rgba16, pq, bg_lin[:n])),
            (f"over float RGBA x {n} backgrounds", "k_linear_over<false>", 16 + 12 * n,
             lambda i, n=n, refs=refs, at=at: lin.set_test_linear_over(at(i), refs, f32, bg_lin[:n])),
            (f"yardstick k_alpha RGBA8 -> RGB8 slots x {n} backgrounds", "k_alpha<false, false, 8>", 4 + 3 * n,
             lambda i, n=n, refs=refs, at=at: b8.set_test_over(at(i), refs, rgba8, ce.PIXEL_RGBA8, bg8[:n])),
            (f"yardstick k_alpha RGBA16 -> u16 slots x {n} backgrounds", "k_alpha<true, true, 10>", 8 + 6 * n,
             lambda i, n=n, refs=refs, at=at: deep.set_test_over(at(i), refs, rgba16, ce.PIXEL_RGBA16, bg10[:n])),
        ]
    for name, kernel, bytes_per_px, call in phases:
        call(0)  # first use: staging allocations, code object load
        assert L.hipDeviceSynchronize() == 0
        t = time.perf_counter()
        for i in range(N):
            call(i)
        assert L.hipDeviceSynchronize() == 0
        ms = (time.perf_counter() - t) * 1e3
        mb = bytes_per_px * W * H / 1e6
        print(f"{W}x{H} {name} [{kernel}]: {N} images in {ms:.3f} ms (host clock, upload and submission included), {bytes_per_px} B/px = "
              f"{mb:.3f} MB per dispatch")
        plan.append({"label": name, "kernel": kernel, "dispatches": N + 1, "mb": mb, "warmup": 1})
    for b in (lin, b8, deep):
        b.close()
print(json.dumps(plan))
