"""Kernel timing of the ICC ingest: 54 images of 768x512 into the 54 test slots of an RGB8, a deep and
a linear batch by ce_batch_set_test_icc with a Display P3 matrix/TRC profile (tests/icc_restatement.py writes it) - k_icc_encode
for the integer slots, k_tagged with icc_px for the linear ones - and, on the same inputs, the two things they are measured
against: the CICP ingest of the same code values at (12, 13) (k_tagged with cicp_px) and the colour-table gather of
ce_batch_set_test_lut (k_lut_apply) with a table of the same transform.  For the table route the host's one-off cost is
printed too: Pillow's lcms2 over the 2^24 colours, where Pillow is present, and ce_lut_create.  All sources are host images:
only the kernels are compared.  The phases run in the printed order with a synchronise between them, one warm-up call first,
and the last line printed is the plan as JSON: profiles/icc_ingest_medians.py reads it with the kernel trace.  No counters:
collect those in a run of their own.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/icc_ingest_timing.py > out/plan.txt
    python3 profiles/icc_ingest_medians.py out out/plan.txt"""
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codec_eval_amd as ce  # noqa: E402
import icc_restatement as R  # noqa: E402

L = ce.lib()
rng = np.random.default_rng(1)
plan = []
W, H, N = 768, 512, 54
P3 = R.fixtures()["p3"]
with ce.Context(0) as ctx:
    rgb8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb10 = rng.integers(0, 1024, (H, W, 3)).astype(np.uint16)
    rgb16 = rng.integers(0, 65536, (H, W, 3)).astype(np.uint16)
    icc = ce.IccProfile(ctx, P3)
    cube = ce.ColorTable.identity_cube()
    t = time.perf_counter()
    table = R.to_srgb(cube, P3, 8)
    print(f"table route, host: the numpy restatement over 2^24 colours {time.perf_counter() - t:.2f} s")
    try:
        from PIL import Image, ImageCms

        src, dst = ImageCms.ImageCmsProfile(io.BytesIO(P3)), ImageCms.ImageCmsProfile(io.BytesIO(R.fixtures()["srgb_para"]))
        im = Image.fromarray(cube.reshape(4096, 4096, 3))
        t = time.perf_counter()
        ImageCms.profileToProfile(im, src, dst, renderingIntent=ImageCms.Intent.RELATIVE_COLORIMETRIC)
        print(f"table route, host: Pillow's lcms2 over 2^24 colours {time.perf_counter() - t:.2f} s (one thread)")
    except ImportError:
        print("table route, host: Pillow is not installed, lcms2 not timed")
    t = time.perf_counter()
    lut = ce.ColorTable(ctx, table)
    print(f"table route, host: ce_lut_create (50 MB up, expand to 64 MB) {(time.perf_counter() - t) * 1e3:.1f} ms")
    b8, b10, b16, lin = ce.Batch(ctx, W, H, 1, N), ctx.batch_deep(W, H, 1, N, 10, 10), ctx.batch_deep(W, H, 1, N, 16, 16), ctx.batch_linear(W, H, 1, N)
    p3_8, p3_10 = ce.ColourDescription(12, 13, 8), ce.ColourDescription(12, 13, 10)
    # (label, kernel in the trace: every word is in its name, bytes per pixel the kernel must move, call on slot i)
    phases = [
        ("icc RGB8 -> RGB8 slot", "k_icc_encode< icc_px<", 3 + 3, lambda i: b8.set_test_icc(i, 0, rgb8, 8, icc)),
        ("icc RGB16 depth 10 -> deep slot of 10", "k_icc_encode< icc_px<", 6 + 6, lambda i: b10.set_test_icc(i, 0, rgb10, 10, icc)),
        ("icc RGB16 depth 16 -> deep slot of 16", "k_icc_encode< icc_px<", 6 + 6, lambda i: b16.set_test_icc(i, 0, rgb16, 16, icc)),
        ("icc RGB8 -> linear slot", "k_tagged< icc_px<", 3 + 12, lambda i: lin.set_test_icc(i, 0, rgb8, 8, icc)),
        ("icc RGB16 depth 10 -> linear slot", "k_tagged< icc_px<", 6 + 12, lambda i: lin.set_test_icc(i, 0, rgb10, 10, icc)),
        ("yardstick cicp RGB8 (12, 13, 8) -> linear slot", "k_tagged< cicp_px<", 3 + 12, lambda i: lin.set_test_cicp(i, 0, rgb8, p3_8)),
        ("yardstick cicp RGB16 (12, 13, 10) -> linear slot", "k_tagged< cicp_px<", 6 + 12, lambda i: lin.set_test_cicp(i, 0, rgb10, p3_10)),
        ("yardstick table gather RGB8 -> RGB8 slot", "k_lut_apply", 3 + 4 + 3, lambda i: b8.set_test_lut(i, 0, rgb8, ce.PIXEL_RGB8, lut)),
    ]
    for name, kernel, bytes_per_px, call in phases:
        call(0)  # first use: staging allocations, table upload, code object load
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
    for b in (b8, b10, b16, lin):
        b.close()
    lut.close()
    icc.close()
print(json.dumps(plan))
