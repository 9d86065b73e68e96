"""Kernel timing of the HLG ingest against the CICP ingest of the same images in the same run: 54
images of 768x512 into the test slot of a linear batch by ce_batch_set_test_hlg from RGB16 at depth 10 and at depth 16
(k_tagged with hlg_px), and by ce_batch_set_test_yuv_hlg from P010 4:2:0 BT.2020 limited range at depth 16 (k_yuv_tagged with
hlg_px); as the yardsticks the same images through ce_batch_set_test_cicp at (9, 16, the same depth) (k_tagged with cicp_px)
and ce_batch_set_test_yuv_cicp at (9, 16, depth 16) (k_yuv_tagged with cicp_px).  All sources are host images: only the kernels are compared.  The phases run in the printed order
with a synchronise between them, one warm-up call first, and the last line printed is the plan as JSON:
profiles/hlg_ingest_medians.py reads it with the kernel trace and gives the per-dispatch medians of each phase and the two
ratios.  No counters: collect those in a run of their own.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/hlg_ingest_timing.py > out/plan.txt
    python3 profiles/hlg_ingest_medians.py out out/plan.txt"""
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
W, H, N = 768, 512, 54
with ce.Context(0) as ctx:
    cw, ch = W // 2, H // 2
    y10 = (rng.integers(64, 941, (H, W)).astype(np.uint16) << 6).astype(np.uint16)
    c10 = (rng.integers(64, 961, (ch, 2 * cw)).astype(np.uint16) << 6).astype(np.uint16)
    p010 = ce.YuvImage([y10, c10], ce.YUV_420, ce.YUV_SEMIPLANAR, ce.YUV_BT2020, ce.YUV_LIMITED, ce.CHROMA_TRIANGLE, 10, True)
    rgb10 = rng.integers(0, 1024, (H, W, 3)).astype(np.uint16)
    rgb16 = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    b = ctx.batch_linear(W, H, 1, 1)
    hlg10, hlg16 = ce.HlgDescription.BT2100_HLG, ce.HlgDescription.BT2100_HLG.with_depth(16)
    pq10, pq16 = ce.ColourDescription(9, 16, 10, 203.0), ce.ColourDescription(9, 16, 16, 203.0)
    # (label, kernel in the trace: every word is in its name, bytes per pixel the kernel must move, call)
    phases = [
        ("hlg RGB16 depth 10", "k_tagged< hlg_px<", 6 + 12, lambda: b.set_test_hlg(0, 0, rgb10, hlg10)),
        ("hlg RGB16 depth 16", "k_tagged< hlg_px<", 6 + 12, lambda: b.set_test_hlg(0, 0, rgb16, hlg16)),
        ("hlg P010 depth 16", "k_yuv_tagged< hlg_px<", 3 + 12, lambda: b.set_test_yuv_hlg(0, 0, p010, hlg16)),
        ("yardstick cicp RGB16 (9, 16, 10)", "k_tagged< cicp_px<", 6 + 12, lambda: b.set_test_cicp(0, 0, rgb10, pq10)),
        ("yardstick cicp RGB16 (9, 16, 16)", "k_tagged< cicp_px<", 6 + 12, lambda: b.set_test_cicp(0, 0, rgb16, pq16)),
        ("yardstick cicp P010 (9, 16, 16)", "k_yuv_tagged< cicp_px<", 3 + 12, lambda: b.set_test_yuv_cicp(0, 0, p010, pq16)),
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
        plan.append({"label": name, "kernel": kernel, "dispatches": N + 1, "mb": mb, "warmup": 1})
    b.close()
print(json.dumps(plan))
