"""The anchors of the SSIM / MS-SSIM map restatement (tests/msssim_map_restatement.py; include/ce_metrics.h:
ce_batch_msssim_map), which the host build of the kernel and the device are compared with element by
element: what it gives on identical images and on a pattern against its inverse, that its values are the very integers the
score restatement sums, its shapes, its cells and its counts."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as K  # noqa: E402
import msssim_map_cases as MK  # noqa: E402
import msssim_map_restatement as R  # noqa: E402
import msssim_restatement as M  # noqa: E402

import codec_eval_amd as ce  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_identical_images_give_zero_everywhere():
    rng = np.random.default_rng(3)
    img16 = rng.integers(0, 1 << 16, (163, 161, 3)).astype(np.uint16)
    for img, depth, levels, level in ((img16, 16, 5, 0), (img16, 16, 5, 3), (K.pair(43, 27, 8)[0], 8, 1, 0)):
        for what in ("ssim", "cs"):
            m = R.full_map(img, img.copy(), depth, levels, level, what)
            assert m.dtype == np.uint32 and not m.any()
            assert R.over(m, [0, 1, R.U32_MAX]).tolist() == [[0, 0, 0]] * 3
            assert not R.cells(m, 16).any()


@pytest.mark.parametrize("w,h,depth,levels", [(176, 163, 8, 5), (171, 171, 8, 5), (192, 256, 16, 5), (43, 27, 8, 1)], ids=lambda v: str(v))
def test_the_map_sums_to_the_scores_integers(w, h, depth, levels):
    """n * 2^32 - map.sum() == ssim_q (cs_q): nothing saturates on this content, every q lies in (0.54 * 2^32, 2^32)"""
    want = K.expected(w, h, depth, levels)
    for level in range(levels):
        q = MK.level_q(w, h, depth, levels, level)
        assert q.shape[2:] == tuple(d - 10 for d in M.levels_of(w, h, levels)[level][::-1])
        assert int(q.min()) > 0.54 * R.Q32 and int(q.max()) <= R.Q32
        for what, key in (("ssim", "ssim_q"), ("cs", "cs_q")):
            m = MK.expected(w, h, depth, levels, level, what)
            for c in range(3):
                assert want["n"][level] * R.Q32 - sum(int(v) for v in m[c].sum(axis=1, dtype=np.uint64)) == want[key][level][c], (level, what, c)


def test_the_smallest_image_has_one_position():
    ref, test = K.pair(11, 11, 8)
    m = R.full_map(ref, test, 8, 1, 0)
    assert m.shape == (3, 1, 1)
    for block in MK.BLOCKS:
        assert np.array_equal(R.cells(m, block), m)
    assert MK.expected(176, 163, 8, 5, 4).shape == (3, 1, 1)


def test_a_checkerboard_against_its_inverse_saturates():
    w, h = 43, 27
    a, b = K.checkerboard(w, h)
    q = R.level_q(a, b, 8, 1, 0)
    assert int(q[0].max()) <= 0  # qs: SSIM is nowhere positive
    m = R.full_map(a, b, 8, 1, 0)
    n = (w - 10) * (h - 10)
    assert (m == R.U32_MAX).all()
    assert R.over(m, [0, R.Q32 // 2, R.U32_MAX - 1, R.U32_MAX]).tolist() == [[n, n, n, 0]] * 3
    assert (R.cells(m, 64) == R.U32_MAX).all() and R.cells(m, 64).shape == (3, 1, 1)
    # the ends of the value: q = 2^32 and above give 0, q = 1 gives 2^32 - 1 unsaturated, q = 0 and below saturate
    assert R.value(np.array([R.Q32 + 5, R.Q32, R.Q32 - 1, 1, 0, -7], np.int64)).tolist() == [0, 0, 1, R.U32_MAX, R.U32_MAX, R.U32_MAX]


@pytest.mark.parametrize("w,h", [(171, 171), (43, 27)], ids=lambda v: str(v))
def test_cell_maxima_are_the_maxima_of_the_maps_cells(w, h):
    levels = 5 if w > 160 else 1
    m = MK.expected(w, h, 8, levels, 0)
    vh, vw = m.shape[1:]
    for block in MK.BLOCKS:
        got = MK.expected(w, h, 8, levels, 0, "ssim", block)
        assert got.shape == (3, -(-vh // block), -(-vw // block))
        for c in range(3):
            for cy in range(got.shape[1]):
                for cx in range(got.shape[2]):
                    assert got[c, cy, cx] == m[c, cy * block:(cy + 1) * block, cx * block:(cx + 1) * block].max(), (block, c, cy, cx)


def test_a_patch_is_found_by_the_cell_maxima():
    w, h, x0, y0 = 171, 171, 100, 60
    ref, test = MK.patched(w, h, x0, y0)
    m = R.full_map(ref, test, 8, 5, 0)
    far = np.ones(m.shape[1:], bool)
    far[max(y0 - 10, 0):y0 + 6, max(x0 - 10, 0):x0 + 6] = False  # positions whose window does not meet the patch
    assert not m[:, far].any() and m.max() > R.Q32 // 2
    cells = R.cells(m, 16)
    for c in range(3):
        cy, cx = np.unravel_index(np.argmax(cells[c]), cells[c].shape)
        # the cell holds a position whose 11 x 11 window meets the patch
        assert y0 - 10 < (cy + 1) * 16 and cy * 16 < y0 + 6 and x0 - 10 < (cx + 1) * 16 and cx * 16 < x0 + 6, (c, cy, cx)
    counts = R.over(m, [0])
    assert all(0 < int(counts[c, 0]) <= 16 * 16 for c in range(3))


def test_library_surface():
    L = ce.lib()
    for name in ("ce_batch_msssim_map", "ce_eval_pair_msssim_map", "ce_eval_pair_msssim_map_deep"):
        assert name in ce.ABI_SYMBOLS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
    assert "#define CE_MSSSIM_MAP_MAX_THRESHOLDS 8\n" in header and ce.MSSSIM_MAP_MAX_THRESHOLDS == 8
    assert "enum { CE_MSSSIM_MAP_SSIM = 0, CE_MSSSIM_MAP_CS = 1 };" in header
    assert ce.MSSSIM_Q32 == 1 << 32 == R.Q32
    assert callable(ce.Batch.ms_ssim_maps) and callable(ce.Context.ms_ssim_map)


def test_no_result_without_a_device():
    """Nothing is computed on the CPU: on a host without a device no context can be made (CE_ERR_BACKEND), and without a
    context or a batch the calls refuse and leave their outputs alone."""
    L = ce.lib()
    img = np.zeros((11, 11, 3), np.uint8)
    m, thr, cnt = np.full(3, 77, np.uint32), np.array([0], np.uint32), np.full(3, 77, np.uint64)
    assert L.ce_batch_msssim_map(None, 0, 1, 1, 0, 0, 1, m.ctypes.data, 3, thr.ctypes.data, 1, cnt.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim_map(None, img.ctypes.data, img.nbytes, img.ctypes.data, img.nbytes, 11, 11, 1, 0, 0, 1, m.ctypes.data, 3,
                                     thr.ctypes.data, 1, cnt.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim_map_deep(None, img.ctypes.data, 2 * img.nbytes, img.ctypes.data, 2 * img.nbytes, 8, 11, 11, 1, 0, 0, 1,
                                          m.ctypes.data, 3, thr.ctypes.data, 1, cnt.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert np.all(m == 77) and np.all(cnt == 77)
    if ce.device_count() > 0:
        return  # the rest is what a host without a device does
    with pytest.raises(ce.CodecEvalError) as e:
        ce.Context(0).ms_ssim_map(img, img, 11, 11, 1)
    assert e.value.status == ce.CE_ERR_BACKEND
