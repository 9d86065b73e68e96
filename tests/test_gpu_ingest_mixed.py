"""One batch filled through every ingest route in turn.  The per-route files fill a batch through one route at a time; what
the routes share - the ordering rule of slot writes and the two wide staging pairs (ce_ingest.cpp) - shows only when a route
meets a pair that another route sized or left busy.  The expected content of a slot is what the route's own leaf conversion
returns for the same input, uploaded through the plain route into a second batch; the two slabs must agree in every bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_restatement as Y  # noqa: E402
from test_gpu_yuv_ingest import image, read_slab  # noqa: E402
from test_gpu_yuv_linear import device_planes  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 23, 9  # w * h is no multiple of 4: the slots of a slab are not 16-byte aligned


def planes(rng, sub, depth):
    """random Y, Cb, Cr of a W x H image at `depth` bits"""
    dt = np.uint8 if depth == 8 else np.uint16
    cw, ch = Y.chroma_size(W, H, sub)
    draw = lambda rows, cols: rng.integers(0, 1 << depth, (rows, cols)).astype(dt)
    return draw(H, W), draw(ch, cw), draw(ch, cw)


def test_rgb8_batch_through_every_route(ce, gpu_ctx):
    """Test slots 0 .. 7: plain RGB8, _fmt RGBA8, _yuv host 4:2:0, _yuv device, _over with two backgrounds (two slots), _lut
    with the identity table, _fmt RGBA8 again.  The wide staging pairs go 0 (_fmt), 1 (_yuv), 0 (_over), 1 (_lut), 0 (_fmt):
    each is taken while still busy, by another route than the one that used it last."""
    rng = np.random.default_rng(2309)
    rgb = lambda: rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgba = lambda: rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    keep = []
    ref, plain, fmt_a, over, lut_in, fmt_b = rgb(), rgb(), rgba(), rgba(), rgba(), rgba()
    yuv_host = image(ce, *planes(rng, Y.SUB_420, 8), Y.SUB_420, Y.PLANAR, 3, rng)
    yuv_dev = device_planes(ce, image(ce, *planes(rng, Y.SUB_420, 8), Y.SUB_420, Y.SEMIPLANAR, 1, rng), keep)
    bgs = [(255, 255, 255), (12, 200, 77)]
    table = ce.ColorTable(gpu_ctx, ce.ColorTable.identity_cube())
    mixed, direct = ce.Batch(gpu_ctx, W, H, 1, 8), ce.Batch(gpu_ctx, W, H, 1, 8)
    try:
        want = [plain, fmt_a[..., :3], gpu_ctx.yuv_to_rgb8(yuv_host, W, H), gpu_ctx.yuv_to_rgb8(yuv_dev, W, H)]
        want += [gpu_ctx.composite_rgba8(over, W, H, bg) for bg in bgs]
        want += [lut_in[..., :3], fmt_b[..., :3]]
        mixed.set_reference(0, ref)
        mixed.set_test(0, 0, plain)
        mixed.set_test_fmt(1, 0, fmt_a, ce.PIXEL_RGBA8)
        mixed.set_test_yuv(2, 0, yuv_host)
        mixed.set_test_yuv(3, 0, yuv_dev)
        mixed.set_test_over(4, [0, 0], over, ce.PIXEL_RGBA8, bgs)
        mixed.set_test_lut(6, 0, lut_in, ce.PIXEL_RGBA8, table)
        mixed.set_test_fmt(7, 0, fmt_b, ce.PIXEL_RGBA8)
        direct.set_reference(0, ref)
        for i, img in enumerate(want):
            direct.set_test(i, 0, np.ascontiguousarray(img))
        n = W * H * 3
        got, exp = read_slab(ce, mixed.test_slab, 8 * n), read_slab(ce, direct.test_slab, 8 * n)
        for i in range(8):
            assert np.array_equal(got[i * n:(i + 1) * n], exp[i * n:(i + 1) * n]), f"test slot {i}"
        assert np.array_equal(read_slab(ce, mixed.reference_slab, n), read_slab(ce, direct.reference_slab, n))
    finally:
        mixed.close()  # waits for the device: the planes in `keep` are free to go
        direct.close()
        table.close()
        keep.clear()


def test_linear_batch_through_every_route_twice(ce, gpu_ctx):
    """Test slots 0 .. 5 and again 6 .. 11: _fmt RGB_F32, _cicp RGB16 PQ / BT.2020, _hlg RGBA16, _yuv_cicp host 10-bit 4:2:2,
    _yuv_cicp device, _yuv_hlg host semiplanar.  Every route but the device planes takes a wide staging pair, so over the
    two rounds each pair is reused by every route while the previous one's conversion may still run."""
    rng = np.random.default_rng(923)
    pq = ce.ColourDescription(ce.PRIMARIES_BT2020, ce.TRANSFER_PQ, 10, 203.0)
    hlg = ce.HlgDescription()  # BT.2020 primaries, 10 bits, 1000 nits
    keep, fills, want = [], [], []
    for _ in range(2):
        f32 = rng.random((H, W, 3), np.float32)
        rgb16 = rng.integers(0, 1024, (H, W, 3)).astype(np.uint16)
        rgba16 = rng.integers(0, 1024, (H, W, 4)).astype(np.uint16)
        y422 = image(ce, *planes(rng, Y.SUB_422, 10), Y.SUB_422, Y.PLANAR, 2, rng, depth=10)
        y422_dev = device_planes(ce, image(ce, *planes(rng, Y.SUB_422, 10), Y.SUB_422, Y.PLANAR, 4, rng, depth=10), keep)
        y420_semi = image(ce, *planes(rng, Y.SUB_420, 10), Y.SUB_420, Y.SEMIPLANAR, 2, rng, depth=10)
        want += [f32, gpu_ctx.cicp_to_linear(rgb16, W, H, pq), gpu_ctx.hlg_to_linear(rgba16, W, H, hlg), gpu_ctx.yuv_to_linear(y422, W, H, pq),
                 gpu_ctx.yuv_to_linear(y422_dev, W, H, pq), gpu_ctx.yuv_hlg_to_linear(y420_semi, W, H, hlg)]
        fills += [lambda b, i, a=f32: b.set_test_fmt(i, 0, a, ce.PIXEL_RGB_F32), lambda b, i, a=rgb16: b.set_test_cicp(i, 0, a, pq),
                  lambda b, i, a=rgba16: b.set_test_hlg(i, 0, a, hlg), lambda b, i, a=y422: b.set_test_yuv_cicp(i, 0, a, pq),
                  lambda b, i, a=y422_dev: b.set_test_yuv_cicp(i, 0, a, pq), lambda b, i, a=y420_semi: b.set_test_yuv_hlg(i, 0, a, hlg)]
    ref = rng.random((H, W, 3), np.float32)
    mixed, direct = gpu_ctx.batch_linear(W, H, 1, 12), gpu_ctx.batch_linear(W, H, 1, 12)
    try:
        mixed.set_reference(0, ref)
        for i, fill in enumerate(fills):
            fill(mixed, i)
        direct.set_reference(0, ref)
        for i, img in enumerate(want):
            direct.set_test_fmt(i, 0, np.ascontiguousarray(img, np.float32), ce.PIXEL_RGB_F32)
        n = W * H * 12
        got, exp = read_slab(ce, mixed.test_slab, 12 * n), read_slab(ce, direct.test_slab, 12 * n)
        for i in range(12):
            assert np.array_equal(got[i * n:(i + 1) * n], exp[i * n:(i + 1) * n]), f"test slot {i}"
        assert np.array_equal(read_slab(ce, mixed.reference_slab, n), read_slab(ce, direct.reference_slab, n))
    finally:
        mixed.close()  # waits for the device: the planes in `keep` are free to go
        direct.close()
        keep.clear()
