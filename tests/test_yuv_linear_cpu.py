"""The parts of the fused Y'CbCr + CICP ingest that need no device (include/ce_metrics.h: ce_batch_set_*_yuv_cicp,
ce_yuv_to_linear): the composed restatement on cases worked out by hand, the Python binding's struct
layout and the argument checks that return before any device call, and ImageData.yuv's new keywords."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import yuv_linear_cases as L  # noqa: E402
import yuv_restatement as Y  # noqa: E402


def test_gray_full_range_linear_transfer_is_v_over_255():
    """4:0:0, full range, 8 bits, D = 8: KY = 65536, so R = G = B = (65536 y + 32768) >> 16 = y; transfer 8 is y / 255."""
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    got = L.composed(y, None, None, 16, 16, Y.SUB_400, Y.BT709, Y.FULL, Y.TRIANGLE, 8, False, 1, 8, 8)
    want = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32).reshape(16, 16)
    assert got.dtype == np.float32 and got.shape == (16, 16, 3)
    for c in range(3):
        assert np.array_equal(got[..., c].view(np.uint32), want.view(np.uint32))


def test_limited_range_pq_white_is_the_last_table_entry():
    """10-bit limited range: Y = 940, Cb = Cr = 512 is white.  KY = rint(1023 / 876 * 65536) = 76533 and
    (76533 * 876 + 32768) >> 16 = 1023, so at c.depth = 10 every channel is table[1023] = 10000 / 203 nits-ratio; black
    (Y = 64) is table[0] = 0; and the MSB-aligned form (P010: v << 6) reads the same."""
    k = Y.coefficients(Y.BT2020, Y.LIMITED, 10, 10)
    assert k[0] == 76533 and (k[0] * (940 - 64) + 32768) >> 16 == 1023
    table = R.transfer_table(16, 10, 203.0)
    assert table[1023] == np.float32(10000.0 / float(np.float32(203.0)))
    y = np.array([[940, 64], [940, 64]], np.uint16)
    c = np.full((2, 2), 512, np.uint16)
    for msb in (False, True):
        sh = 6 if msb else 0
        got = L.composed(y << sh, c << sh, c << sh, 2, 2, Y.SUB_444, Y.BT2020, Y.LIMITED, Y.TRIANGLE, 10, msb, 1, 16, 10)
        assert np.array_equal(got[:, 0].view(np.uint32), np.full((2, 3), table[1023]).view(np.uint32))
        assert np.array_equal(got[:, 1], np.zeros((2, 3), np.float32))
    # with BT.2020 primaries white stays white to f32 rounding (the matrix rows sum to 1) and is the separately rounded sum
    got = L.composed(y, c, c, 2, 2, Y.SUB_444, Y.BT2020, Y.LIMITED, Y.TRIANGLE, 10, False, 9, 16, 10)
    m, t = R.colour_matrix(9), table[1023]
    want = np.array([(m[i, 0] * t + m[i, 1] * t) + m[i, 2] * t for i in range(3)], np.float32)
    assert np.array_equal(got[0, 0].view(np.uint32), want.view(np.uint32)) and np.allclose(want, t, rtol=1e-6)


def test_the_grid_depth_matters_between_code_points():
    """c.depth = 16 keeps what the matrix produces between the samples' code points: a limited-range 8-bit ramp lands on
    k / 255 through a depth-8 grid and within half such a step of that, but not on it, through a depth-16 one."""
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    a = L.composed(y, None, None, 16, 16, Y.SUB_400, Y.BT709, Y.LIMITED, Y.TRIANGLE, 8, False, 1, 8, 8)
    b = L.composed(y, None, None, 16, 16, Y.SUB_400, Y.BT709, Y.LIMITED, Y.TRIANGLE, 8, False, 1, 8, 16)
    on_grid = lambda v: np.array_equal(v, (np.rint(v.astype(np.float64) * 255.0) / 255.0).astype(np.float32))
    assert on_grid(a) and not on_grid(b) and np.abs(a - b).max() <= 0.5 / 255.0 + 1e-6


def test_binding_layout_and_checks_that_need_no_device(ce):
    assert C.sizeof(ce.CeYuvImage) == 88 and C.sizeof(ce.CeColour) == 16
    lib = ce.lib()
    yuv_p, col_p = C.POINTER(ce.CeYuvImage), C.POINTER(ce.CeColour)
    assert lib.ce_batch_set_reference_yuv_cicp.argtypes == [C.c_void_p, C.c_uint32, yuv_p, col_p]
    assert lib.ce_batch_set_test_yuv_cicp.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, yuv_p, col_p]
    assert lib.ce_yuv_to_linear.argtypes == [C.c_void_p, yuv_p, col_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
    img, _keep = ce.YuvImage([np.zeros((2, 2), np.uint8)] * 3, subsampling=ce.YUV_444)._c()
    col = ce.ColourDescription(1, 13, 8)._c()
    out = np.zeros(12, np.float32)
    # a null handle is refused before anything is touched
    assert lib.ce_batch_set_reference_yuv_cicp(None, 0, C.byref(img), C.byref(col)) == ce.CE_ERR_INVALID_ARG
    assert lib.ce_batch_set_test_yuv_cicp(None, 0, 0, C.byref(img), C.byref(col)) == ce.CE_ERR_INVALID_ARG
    assert lib.ce_yuv_to_linear(None, C.byref(img), C.byref(col), 2, 2, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
    for name in ("set_reference_yuv_cicp", "set_test_yuv_cicp"):
        assert callable(getattr(ce.Batch, name))
    assert callable(ce.Context.yuv_to_linear)


def test_imagedata_yuv_defaults_are_unchanged_and_the_new_keywords(ce):
    S = importlib.import_module("codec-eval_amd.session")
    w, h = 10, 6
    rng = np.random.default_rng(3)
    y, cb, cr = Y.random_planes(rng, w, h, Y.SUB_420)
    old = S.ImageData.yuv([y, cb, cr], w, h)
    assert old.yuv_image.depth == 8 and not old.yuv_image.msb_aligned and old.colour is None and old.depth == 0 and not old.in_linear_light
    assert np.array_equal(old.to_rgb8_vec().reshape(h, w, 3), Y.yuv_to_rgb(y, cb, cr, w, h, Y.SUB_420))
    y10, cb10, cr10 = Y.random_planes(rng, w, h, Y.SUB_420, 10, True)
    with pytest.raises(TypeError, match="2-D uint8 planes"):
        S.ImageData.yuv([y10, cb10, cr10], w, h)
    with pytest.raises(TypeError):
        S.ImageData.yuv([y, cb, cr], w, h, depth=10)
    with pytest.raises(ValueError):
        S.ImageData.yuv([y10, cb10, cr10], w, h, depth=16)
    with pytest.raises(TypeError):  # keyword-only
        S.ImageData.yuv([y10, cb10, cr10], w, h, ce.YUV_420, ce.YUV_PLANAR, ce.YUV_BT601, ce.YUV_FULL, ce.CHROMA_TRIANGLE, 10)
    deep = S.ImageData.yuv([y10, cb10, cr10], w, h, matrix=ce.YUV_BT2020, range=ce.YUV_LIMITED, depth=10, msb_aligned=True)
    assert deep.yuv_image.depth == 10 and deep.yuv_image.msb_aligned and not deep.in_linear_light
    assert np.array_equal(deep.to_rgb8_vec().reshape(h, w, 3), Y.yuv_to_rgb(y10, cb10, cr10, w, h, Y.SUB_420, Y.BT2020, Y.LIMITED, Y.TRIANGLE, 10, 8, True))
    srgb = S.ImageData.yuv([y, cb, cr], w, h, colour=ce.ColourDescription.SRGB)
    assert not srgb.in_linear_light and np.array_equal(srgb.to_rgb8_vec(), old.to_rgb8_vec())
    hdr = S.ImageData.yuv([y10, cb10, cr10], w, h, matrix=ce.YUV_BT2020, range=ce.YUV_LIMITED, depth=10, msb_aligned=True,
                          colour=ce.ColourDescription.BT2020_PQ)
    assert hdr.in_linear_light and hdr.colour == ce.ColourDescription.BT2020_PQ.with_depth(10)
    with pytest.raises(ce.MetricCalculation, match="no RGB8 form"):
        hdr.to_rgb8_vec()
