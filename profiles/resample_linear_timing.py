"""Kernel timing of the float resampler: 54 resident 768x512 linear pairs (6 references x 9 tests, both
slabs = 60 images per call) to 1/2 (384x256) and 4/3 (1024x683), then the same images as RGB8 through the fixed-point
resampler on the same pixel counts as the yardstick (resample_h / resample_v).  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/resample_linear_timing.py
then python3 profiles/resample_linear_medians.py out for the per-dispatch medians of each (kernel, grid)."""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

wl = importlib.import_module("codec-eval_amd.workloads")
W, H, REFS, PER_REF = 768, 512, 6, 9
N = REFS + REFS * PER_REF
SHAPES = ((384, 256), (1024, 683))
with ce.Context(0) as ctx:
    t0 = ce.srgb_table(8, 0)
    for linear, bpp in ((True, 12), (False, 3)):
        src = ce.Batch(ctx, W, H, REFS, REFS * PER_REF, linear=linear)
        for r in range(REFS):
            ref = np.asarray(wl.make_reference(W, H, 1000 + r), np.uint8).reshape(H, W, 3)
            src.set_reference(r, t0[ref] * np.float32(4.0) if linear else ref)
            for k in range(PER_REF):
                test = np.asarray(wl.distort(ref, 40 + 6 * k), np.uint8).reshape(H, W, 3)
                src.set_test(r * PER_REF + k, r, t0[test] * np.float32(4.0) if linear else test)
        for ow, oh in SHAPES:
            dst = ce.Batch(ctx, ow, oh, REFS, REFS * PER_REF, linear=linear)
            for _ in range(3):
                src.resample_pairs_into(dst, REFS, REFS * PER_REF)
            ctx.synchronize()
            t = time.perf_counter()
            for _ in range(20):
                src.resample_pairs_into(dst, REFS, REFS * PER_REF)
            ctx.synchronize()
            ms = (time.perf_counter() - t) / 20 * 1e3
            h_bytes = N * bpp * (W * H + ow * H)    # horizontal pass: read the source, write the image between the passes
            v_bytes = N * bpp * (ow * H + ow * oh)  # vertical pass: read it, write the result
            print(f"{'linear' if linear else 'rgb8'} {W}x{H} -> {ow}x{oh}: {ms:.3f} ms per call of {N} images (host clock); the passes must move "
                  f"{h_bytes / 1e6:.1f} MB (horizontal, two dispatches of {REFS} and {REFS * PER_REF} images) + {v_bytes / 1e6:.1f} MB (vertical): "
                  f"{(h_bytes + v_bytes) / ms / 1e9:.3f} TB/s")
            dst.close()
        src.close()
