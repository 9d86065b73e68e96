"""Kernel timing of the gain-map ingest against the CICP and the HLG ingest of the same images in the
same run: images of 768x512 into the test slot of a linear batch by ce_batch_set_test_gainmap (k_gainmap) - an sRGB RGB8
base with a single-channel map of a quarter of its size each way (an Ultra HDR JPEG), the same with a three-channel map,
with a three-channel map of the base's own size, and a Display P3 RGB16 base at depth 10 (the primaries matrix) - and as
the yardsticks the same bases through ce_batch_set_test_cicp (k_tagged with cicp_px) and the RGB16 one through
ce_batch_set_test_hlg (k_tagged with hlg_px, the other ingest that works in f64).  All sources are host images: only the
kernels are compared.  The times are the library's own device events around each launch (ce_prof_*: one kernel at a time),
read per profiler name; each phase runs ROUNDS times, interleaved with the others, after one warm-up call, and the mean per
dispatch of every round is printed with the median over the rounds and the bytes the kernel must move over it.  The last
line is the result as JSON.  No counters, and no threshold: a measurement.
    python3 profiles/gainmap_ingest_timing.py"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

L = ce.lib()
rng = np.random.default_rng(1)
W, H, N, ROUNDS = 768, 512, 40, 5
with ce.Context(0) as ctx:
    rgb8 = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    rgb10 = rng.integers(0, 1024, (H, W, 3)).astype(np.uint16)
    meta = dict(gain_min=0.0, gain_max=3.0, gamma=1.0, base_headroom=0.0, alternate_headroom=3.0)
    quarter1 = ce.GainMap(rng.integers(0, 256, (H // 4, W // 4, 1)).astype(np.uint8), **meta)
    quarter3 = ce.GainMap(rng.integers(0, 256, (H // 4, W // 4, 3)).astype(np.uint8), **meta)
    full3 = ce.GainMap(rng.integers(0, 256, (H, W, 3)).astype(np.uint8), **meta)
    srgb, p3_10 = ce.ColourDescription.SRGB, ce.ColourDescription.DISPLAY_P3.with_depth(10)
    hlg10 = ce.HlgDescription.BT2100_HLG
    b = ctx.batch_linear(W, H, 1, 1)
    # (label, the launch's profiler name, bytes per pixel the kernel must move, call)
    phases = [
        ("gainmap RGB8 sRGB, map 1ch 1/16", "gainmap_rgb8_1", 3 + 12 + 1 / 16, lambda: b.set_test_gainmap(0, 0, rgb8, srgb, quarter1)),
        ("gainmap RGB8 sRGB, map 3ch 1/16", "gainmap_rgb8_3", 3 + 12 + 3 / 16, lambda: b.set_test_gainmap(0, 0, rgb8, srgb, quarter3)),
        ("gainmap RGB8 sRGB, map 3ch full", "gainmap_rgb8_3", 3 + 12 + 3, lambda: b.set_test_gainmap(0, 0, rgb8, srgb, full3)),
        ("gainmap RGB16 P3 depth 10, map 1ch 1/16", "gainmap_rgb16_1_m", 6 + 12 + 1 / 16, lambda: b.set_test_gainmap(0, 0, rgb10, p3_10, quarter1)),
        ("yardstick cicp RGB8 sRGB", "cicp_rgb8", 3 + 12, lambda: b.set_test_cicp(0, 0, rgb8, srgb)),
        ("yardstick cicp RGB16 P3 depth 10", "cicp_rgb16_m", 6 + 12, lambda: b.set_test_cicp(0, 0, rgb10, p3_10)),
        ("yardstick hlg RGB16 BT.2020 depth 10", "hlg_rgb16_m", 6 + 12, lambda: b.set_test_hlg(0, 0, rgb10, hlg10)),
    ]
    for _, _, _, call in phases:
        call()  # first use: staging allocations, table upload, code object load
    assert L.hipDeviceSynchronize() == 0
    ctx.prof_enable(True)
    per_round = {label: [] for label, _, _, _ in phases}
    for _ in range(ROUNDS):
        for label, name, _, call in phases:
            ctx.prof_reset()
            for _ in range(N):
                call()
            assert L.hipDeviceSynchronize() == 0
            n, ms = ctx.prof_stats()[name]
            assert n == N, (label, name, n)
            per_round[label].append(ms / n * 1e3)
    ctx.prof_enable(False)
    b.close()
result = []
for label, name, bytes_per_px, _ in phases:
    us = per_round[label]
    med, mb = statistics.median(us), bytes_per_px * W * H / 1e6
    print(f"{W}x{H} {label} [{name}]: per dispatch {', '.join(f'{u:.2f}' for u in us)} us over {ROUNDS} rounds of {N}; median {med:.2f} us, "
          f"{mb:.3f} MB = {mb / med * 1e3:.0f} GB/s, {W * H / med / 1e3:.2f} Gpx/s")
    result.append({"label": label, "kernel": name, "us_per_dispatch": us, "median_us": med, "mb": mb})
print(json.dumps(result))
