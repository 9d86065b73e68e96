"""Kernel timing of the LUT-based ICC ingest: 54 images of 768x512 into the 54 test slots of a linear and
an RGB8 batch by ce_batch_set_test_icc with three LUT profiles (tests/icc_lut_restatement.py writes them) - the XYB-shaped
one, a 2 x 2 x 2 CLUT with type-2 para M curves, and two of sRGB para A curves around a 17^3 and a 33^3 16-bit CLUT - each in
both interpolations: k_tagged with icc_lut_px for the linear slots, k_icc_encode around the same pixel for the RGB8 ones.
Beside them, from the same run, what section 22 measured: the matrix/TRC ingest (k_tagged with icc_px) and the colour-table
gather (k_lut_apply, here with an identity table: the gather's cost does not depend on what the table holds).  The pixels
are uniformly random, the worst case for the CLUT's locality: neighbouring pixels of a photograph mostly share a cell.  The
phases run in the printed order with a synchronise between them, one warm-up call first, and the last line printed is the plan
as JSON in the form profiles/icc_ingest_medians.py reads.  No counters: collect those in a run of their own.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/icc_lut_ingest_timing.py > out/plan.txt
    python3 profiles/icc_ingest_medians.py out out/plan.txt"""
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

L = ce.lib()
rng = np.random.default_rng(1)
plan = []
W, H, N = 768, 512, 54


def clut_profile(g: int) -> bytes:
    return LR.lut_profile(LR.mab_tag(R.curv_tag(), a=R.SRGB_PARA, clut=((g, g, g), LR._xyz_clut((g, g, g)), 2)), name=f"CLUT {g}")


PROFILES = (("2x2x2 + para (XYB)", LR.fixtures()["xyb"]), ("17^3 CLUT", clut_profile(17)), ("33^3 CLUT", clut_profile(33)))
with ce.Context(0) as ctx:
    rgb8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    b8, lin = ce.Batch(ctx, W, H, 1, N), ctx.batch_linear(W, H, 1, N)
    p3 = ce.IccProfile(ctx, R.fixtures()["p3"])
    lut = ce.ColorTable(ctx, ce.ColorTable.identity_cube())
    handles = []
    # (label, kernel in the trace: every word is in its name, bytes per pixel the kernel must move besides the CLUT, call on slot i)
    phases = []
    for label, profile in PROFILES:
        for interp, word in ((ce.ICC_CLUT_TRILINEAR, "trilinear"), (ce.ICC_CLUT_TETRAHEDRAL, "tetrahedral")):
            h = ce.IccLutProfile(ctx, profile, interpolation=interp)
            handles.append(h)
            phases.append((f"lut {label} {word} RGB8 -> linear slot", "k_tagged< icc_lut_px<", 3 + 12, lambda i, h=h: lin.set_test_icc(i, 0, rgb8, 8, h)))
            phases.append((f"lut {label} {word} RGB8 -> RGB8 slot", "k_icc_encode< icc_lut_px<", 3 + 3, lambda i, h=h: b8.set_test_icc(i, 0, rgb8, 8, h)))
    phases += [
        ("yardstick matrix/TRC icc RGB8 -> linear slot", "k_tagged< icc_px<", 3 + 12, lambda i: lin.set_test_icc(i, 0, rgb8, 8, p3)),
        ("yardstick matrix/TRC icc RGB8 -> RGB8 slot", "k_icc_encode< icc_px<", 3 + 3, lambda i: b8.set_test_icc(i, 0, rgb8, 8, p3)),
        ("yardstick table gather RGB8 -> RGB8 slot", "k_lut_apply", 3 + 4 + 3, lambda i: b8.set_test_lut(i, 0, rgb8, ce.PIXEL_RGB8, lut)),
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
    for b in (b8, lin):
        b.close()
    for h in handles:
        h.close()
    lut.close()
    p3.close()
print(json.dumps(plan))
