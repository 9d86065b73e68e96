"""Kernel timing of the resampler: 54 resident 768x512 pairs (6 references x 9 tests, both slabs
= 60 images per call) to 1/2 (384x256), 3x (2304x1536) and 4/3 (1024x683).  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/resample_timing.py"""
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

wl = importlib.import_module("codec-eval_amd.workloads")
W, H, REFS, PER_REF = 768, 512, 6, 9
with ce.Context(0) as ctx:
    src = ce.Batch(ctx, W, H, REFS, REFS * PER_REF)
    for r in range(REFS):
        ref = wl.make_reference(W, H, 1000 + r)
        src.set_reference(r, ref)
        for k in range(PER_REF):
            src.set_test(r * PER_REF + k, r, wl.distort(ref, 40 + 6 * k))
    for ow, oh in ((384, 256), (2304, 1536), (1024, 683)):
        dst = ce.Batch(ctx, ow, oh, REFS, REFS * PER_REF)
        for _ in range(3):
            src.resample_pairs_into(dst, REFS, REFS * PER_REF)
        ctx.synchronize()
        t = time.perf_counter()
        for _ in range(20):
            src.resample_pairs_into(dst, REFS, REFS * PER_REF)
        ctx.synchronize()
        ms = (time.perf_counter() - t) / 20 * 1e3
        moved = (REFS + REFS * PER_REF) * 3 * (W * H + 2 * ow * H + ow * oh)  # read source, write + read the middle image, write the result
        print(f"{W}x{H} -> {ow}x{oh}: {ms:.3f} ms per call of 60 images (host clock), {moved / 1e6:.1f} MB the passes must move, "
              f"{moved / ms / 1e9:.3f} TB/s")
        dst.close()
    src.close()
