"""Kernel timing of the image heuristics: one 768x512 image per call, then 250 resident 512x512
references in one call.  Run under  rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/heuristics_timing.py"""
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

wl = importlib.import_module("codec-eval_amd.workloads")
with ce.Context(0) as ctx:
    one = wl.make_reference(768, 512, 1000)
    for _ in range(5):
        ctx.image_heuristics(one, 768, 512)
    t = time.perf_counter()
    for _ in range(50):
        ctx.image_heuristics(one, 768, 512)
    print(f"one 768x512 image per call: {(time.perf_counter() - t) / 50 * 1e3:.3f} ms per call (host clock, upload included)")
    refs = [wl.make_reference(512, 512, 3000 + i) for i in range(250)]
    b = ce.Batch(ctx, 512, 512, 250, 1)
    for i, r in enumerate(refs):
        b.set_reference(i, r)
    for _ in range(3):
        b.image_heuristics(0, 250)
    t = time.perf_counter()
    for _ in range(20):
        b.image_heuristics(0, 250)
    print(f"250 x 512x512 references per call: {(time.perf_counter() - t) / 20 * 1e3:.3f} ms per call (host clock)")
    b.close()
