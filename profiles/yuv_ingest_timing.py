"""Kernel timing of the Y'CbCr ingest: 54 images of 768x512 from DEVICE planes into the test slots
of a resident batch - 8-bit 4:2:0 planar with TRIANGLE, then NEAREST, then NV12 (TRIANGLE), then P010 into a deep 10 / 10
batch - and, as the yardstick on the same pixel count, 54 RGBA8 images through ingest_rgba8 and 54 RGBA16 images through
ingest_deep_rgba16 (host sources: only their kernels are compared).  The phases run in this order with a synchronise
between them, so the dispatches of one kernel name split by start time.  Run under
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/yuv_ingest_timing.py"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

W, H, N = 768, 512, 54
CW, CH = W // 2, H // 2
L = ce.lib()


def device_copy(a: np.ndarray) -> int:
    p = C.c_void_p()
    assert L.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
    assert L.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p.value


rng = np.random.default_rng(1)
with ce.Context(0) as ctx:
    y8, cb8, cr8 = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (CH, CW), (CH, CW)))
    nv = np.ascontiguousarray(np.stack([cb8, cr8], -1).reshape(CH, W))
    y10, c10 = ((rng.integers(0, 1024, s).astype(np.uint16) << 6) for s in ((H, W), (CH, W)))
    d = {k: device_copy(v) for k, v in dict(y8=y8, cb8=cb8, cr8=cr8, nv=nv, y10=y10, c10=c10).items()}
    i420 = lambda mode: ce.YuvImage([d["y8"], d["cb8"], d["cr8"]], upsample=mode, memory=ce.MEM_DEVICE, pitches=[W, CW, CW])
    nv12 = ce.YuvImage([d["y8"], d["nv"]], layout=ce.YUV_SEMIPLANAR, memory=ce.MEM_DEVICE, pitches=[W, W])
    p010 = ce.YuvImage([d["y10"], d["c10"]], layout=ce.YUV_SEMIPLANAR, matrix=ce.YUV_BT2020, range=ce.YUV_LIMITED, depth=10,
                       msb_aligned=True, memory=ce.MEM_DEVICE, pitches=[2 * W, 2 * W])
    rgba8 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    rgba16 = rng.integers(0, 1024, (H, W, 4)).astype(np.uint16)
    b8, b10 = ce.Batch(ctx, W, H, 1, N), ce.Batch(ctx, W, H, 1, N, depths=(10, 10))
    px = W * H
    phases = [
        ("yuv420_8 TRIANGLE", b8, lambda k: b8.set_test_yuv(k, 0, i420(ce.CHROMA_TRIANGLE)), 1.5 + 3),
        ("yuv420_8 NEAREST", b8, lambda k: b8.set_test_yuv(k, 0, i420(ce.CHROMA_NEAREST)), 1.5 + 3),
        ("yuv420_8 NV12", b8, lambda k: b8.set_test_yuv(k, 0, nv12), 1.5 + 3),
        ("yuv420_16_deep P010", b10, lambda k: b10.set_test_yuv(k, 0, p010), 3 + 6),
        ("ingest_rgba8", b8, lambda k: b8.set_test_fmt(k, 0, rgba8, ce.PIXEL_RGBA8), 4 + 3),
        ("ingest_deep_rgba16", b10, lambda k: b10.set_test_fmt(k, 0, rgba16, ce.PIXEL_RGBA16), 8 + 6),
    ]
    for name, batch, fill, bytes_per_px in phases:
        fill(0)  # first use: staging allocations, code object load
        assert L.hipDeviceSynchronize() == 0
        t = time.perf_counter()
        for k in range(N):
            fill(k)
        assert L.hipDeviceSynchronize() == 0
        ms = (time.perf_counter() - t) * 1e3
        print(f"{name}: {N} images in {ms:.3f} ms (host clock, submission included), {bytes_per_px} B/px = {bytes_per_px * px / 1e6:.2f} MB per image")
    b8.close(), b10.close()
    for p in d.values():
        L.hipFree(C.c_void_p(p))
