"""Kernel timing of the tensor ingest: 54 resident 768x512 images of a device tensor into the test
slots of a batch in one call - f32 planar -> u8, f16 planar -> u8, u8 planar -> u8, f32 planar -> linear - 23 calls each
(3 of them warm-up).  Each phase runs another instantiation of k_tensor, so the kernel trace tells them apart.  Run under
rocprofv3 --kernel-trace --stats --output-format csv -d out -- python3 profiles/tensor_ingest_timing.py"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import codec_eval_amd as ce  # noqa: E402

N, W, H, CALLS = 54, 768, 512, 23
L = ce.lib()


def device_copy(a):
    p = C.c_void_p()
    assert L.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
    assert L.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
    return p


with ce.Context(0) as ctx:
    rng = np.random.default_rng(1)
    x = rng.uniform(-0.1, 1.1, (N, 3, H, W)).astype(np.float32)
    sources = {"f32": (x, ce.DTYPE_F32), "f16": (x.astype(np.float16), ce.DTYPE_F16), "u8": (rng.integers(0, 256, x.shape).astype(np.uint8), ce.DTYPE_U8)}
    strides = (3 * H * W, H * W, W, 1)
    refs = list(range(N))
    for name, linear in (("f32", False), ("f16", False), ("u8", False), ("f32", True)):
        a, dtype = sources[name]
        p = device_copy(a)
        batch = ctx.batch_linear(W, H, N, N) if linear else ce.Batch(ctx, W, H, N, N)
        image = ce.TensorImage(p.value, strides, N, H, W, dtype, ce.MEM_DEVICE)
        for _ in range(CALLS):
            batch.set_test_tensor(0, refs, image)
        assert L.hipDeviceSynchronize() == 0
        moved = N * W * H * 3 * (a.itemsize + (4 if linear else 1))
        print(f"{name} planar -> {'linear' if linear else 'u8'}: {CALLS} calls of {N} images, {moved / 1e6:.1f} MB read + written per call")
        batch.close()
        L.hipFree(p)
