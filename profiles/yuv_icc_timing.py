"""Kernel timing of the fused Y'CbCr + ICC ingest: 54 images of 768x512, I420 8-bit and P010, into the 54
test slots of a linear, an RGB8 and a deep-10 batch by ce_batch_set_test_yuv_icc, with the Display P3 matrix/TRC profile and
with one LUT-based profile (mAB, 5^3 CLUT, tetrahedral; tests/icc_restatement.py and icc_lut_restatement.py write them) -
k_yuv_tagged around the ICC pixel for the linear slots, k_yuv_icc_encode for the integer ones.  The integer grid between the two
halves is the session's: the planes' own depth into integer slots, 16 into linear ones.  In the same run, the kernels a fused
launch replaces: k_yuv of the same planes into a slot of that grid's depth, and k_icc_encode / k_tagged with the same pixel on
the resulting RGB (restated on the host, so that nothing else dispatches k_yuv); and the fused CICP ingest of the same planes at
(12, 13), k_yuv_tagged with cicp_px.  P010 into an RGB8 batch has no replaced pair: ce_batch_set_*_icc takes no 16-bit source
there.  All sources are host planes: only the kernels are compared.  The phases run in the printed order with a synchronise
between them, one warm-up call first, and the last line printed is the plan as JSON: profiles/yuv_icc_medians.py reads it with
the kernel trace.  No counters: collect those in a run of their own.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/yuv_icc_timing.py > out/plan.txt
    python3 profiles/yuv_icc_medians.py out out/plan.txt"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codec_eval_amd as ce  # noqa: E402
import icc_lut_restatement as LR  # noqa: E402
import icc_restatement as R  # noqa: E402
import yuv_restatement as Y  # noqa: E402

L = ce.lib()
rng = np.random.default_rng(1)
plan = []
W, H, N = 768, 512, 54
with ce.Context(0) as ctx:
    y8, cb8, cr8 = Y.smooth_planes(rng, W, H, Y.SUB_420, 8)
    y10, cb10, cr10 = ((p << 6).astype(np.uint16) for p in Y.smooth_planes(rng, W, H, Y.SUB_420, 10))
    src = {"I420 8-bit": (ce.YuvImage([y8, cb8, cr8], ce.YUV_420, ce.YUV_PLANAR, ce.YUV_BT601, ce.YUV_FULL), 8, 1.5),
           "P010": (ce.YuvImage([y10, Y.interleave(cb10, cr10)], ce.YUV_420, ce.YUV_SEMIPLANAR, ce.YUV_BT709, ce.YUV_LIMITED, depth=10, msb_aligned=True), 10, 3.0)}
    rgb = {("I420 8-bit", 8): Y.yuv_to_rgb(y8, cb8, cr8, W, H, Y.SUB_420, Y.BT601, Y.FULL, Y.TRIANGLE, 8, 8),
           ("I420 8-bit", 16): Y.yuv_to_rgb(y8, cb8, cr8, W, H, Y.SUB_420, Y.BT601, Y.FULL, Y.TRIANGLE, 8, 16),
           ("P010", 10): Y.yuv_to_rgb(y10, cb10, cr10, W, H, Y.SUB_420, Y.BT709, Y.LIMITED, Y.TRIANGLE, 10, 10, True),
           ("P010", 16): Y.yuv_to_rgb(y10, cb10, cr10, W, H, Y.SUB_420, Y.BT709, Y.LIMITED, Y.TRIANGLE, 10, 16, True)}
    icc = {"P3": (ce.IccProfile(ctx, R.fixtures()["p3"]), "icc_px<"),
           "LUT": (ce.IccLutProfile(ctx, LR.fixtures()["mab_xyz"], 0, ce.ICC_CLUT_TETRAHEDRAL), "icc_lut_px<")}
    batches = {"linear": ctx.batch_linear(W, H, 1, N), "RGB8": ce.Batch(ctx, W, H, 1, N), "deep-10": ctx.batch_deep(W, H, 1, N, 10, 10),
               "deep-16": ctx.batch_deep(W, H, 1, N, 16, 16)}
    out_bytes = {"linear": 12, "RGB8": 3, "deep-10": 6}
    grid_batch = {8: "RGB8", 10: "deep-10", 16: "deep-16"}  # where k_yuv writes integer RGB of that depth
    # (label, kernel in the trace: every word is in its name, bytes per pixel the kernel must move, call on slot i, labels it replaces)
    phases, seen = [], set()

    def add(label, kernel, bytes_per_px, call, replaces=()):
        if label not in seen:
            seen.add(label)
            phases.append((label, kernel, bytes_per_px, call, list(replaces)))
        return label

    for sname, (img, d, in_bytes) in src.items():
        for bname in ("linear", "RGB8", "deep-10"):
            D = 16 if bname == "linear" else d
            frame = "k_yuv_tagged<" if bname == "linear" else "k_yuv_icc_encode<"
            half = "k_tagged<" if bname == "linear" else "k_icc_encode<"
            b = batches[bname]
            for pname, (prof, px) in icc.items():
                replaces = []
                if not (bname == "RGB8" and D != 8):
                    g = batches[grid_batch[D]]
                    replaces.append(add(f"yardstick k_yuv {sname} -> RGB of depth {D}", "k_yuv<", in_bytes + (3 if D == 8 else 6),
                                        lambda i, g=g, img=img: g.set_test_yuv(i, 0, img)))
                    px_rgb = rgb[(sname, D)]
                    replaces.append(add(f"yardstick {pname} RGB of depth {D} -> {bname} slot", f"{half} {px}", (3 if D == 8 else 6) + out_bytes[bname],
                                        lambda i, b=b, px_rgb=px_rgb, D=D, prof=prof: b.set_test_icc(i, 0, px_rgb, D, prof)))
                add(f"fused {pname} {sname} -> {bname} slot, grid {D}", f"{frame} {px}", in_bytes + out_bytes[bname],
                    lambda i, b=b, img=img, D=D, prof=prof: b.set_test_yuv_icc(i, 0, img, D, prof), replaces)
        p3 = ce.ColourDescription(12, 13, 16)
        add(f"yardstick fused cicp (12, 13, 16) {sname} -> linear slot", "k_yuv_tagged< cicp_px<", in_bytes + 12,
            lambda i, img=img, p3=p3: batches["linear"].set_test_yuv_cicp(i, 0, img, p3))
    for name, kernel, bytes_per_px, call, replaces in phases:
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
        plan.append({"label": name, "kernel": kernel, "dispatches": N + 1, "mb": mb, "warmup": 1, "replaces": replaces})
    for b in batches.values():
        b.close()
    for prof, _ in icc.values():
        prof.close()
print(json.dumps(plan))
