"""The Delta E ITP maps without a device (include/ce_metrics.h: ce_batch_delta_e_itp_map, ce_eval_pair_delta_e_itp_map; DESIGN.md
section 20): the numpy restatement (tests/delta_e_itp_map_restatement.py) on cases worked out by hand - identical images, a grey
pair one code apart, one differing pixel and the cell it lands in, the thresholds around its value, the pair of imaginary
colours that saturates the map - and the library's surface: both calls exported and bound, the limit of eight thresholds, and
no way to a result on a host without a device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_e_itp_map_restatement as M  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402

import codec_eval_amd as ce  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIX = [(10, 80.0), (16, 80.0), (10, 203.0), (16, 203.0), (10, 10000.0), (16, 10000.0)]


def grey_codes(lo, hi, white=203.0, depth=10):
    """Two grey values inside the intervals of codes lo and hi."""
    t = F.thresholds(depth, white)
    return (t[lo - 1] + t[lo]) / 2, (t[hi - 1] + t[hi]) / 2


@pytest.mark.parametrize("depth,white", [(10, 80.0), (12, 203.0), (16, 10000.0)])
def test_identical_images_give_zeros(depth, white):
    rng = np.random.default_rng(7)
    img = (rng.random((9, 7, 3), np.float32) * np.float32(30.0) - np.float32(1.0)).astype(np.float32)
    m = M.full_map(img, img.copy(), depth, white)
    assert m.dtype == np.uint32 and m.shape == (9, 7) and not m.any()
    assert not M.block_max(m, 8).any() and M.block_max(m, 8).shape == (2, 1)
    assert M.over(m, [0, 1, ce.DELTA_E_ITP_Q20, M.U32_MAX]).tolist() == [0, 0, 0, 0]


def test_grey_pair_one_code_apart():
    """A grey that moves by one 10-bit code moves I by 1 / 1023 and leaves T and P alone: 720 / 1023 in every pixel."""
    a, b = grey_codes(500, 501)
    m = M.full_map(np.full((5, 6, 3), a, np.float32), np.full((5, 6, 3), b, np.float32), 10, 203.0)
    want = int(np.rint(720.0 / 1023.0 * 2.0 ** 20))
    assert want == 738001 and np.all(m == want)
    assert np.all(M.block_max(m, 4) == want) and M.block_max(m, 4).shape == (2, 2)
    assert M.over(m, [want - 1, want]).tolist() == [30, 0]


def test_one_differing_pixel_lands_in_one_cell():
    w, h, y, x = 70, 37, 33, 65  # the last cell row and the last cell column at B = 8, both clipped by the image
    a, b = grey_codes(300, 340)
    ref = np.full((h, w, 3), a, np.float32)
    test = ref.copy()
    test[y, x] = b
    m = M.full_map(ref, test, 10, 203.0)
    k = int(m[y, x])
    assert k > 0 and int(m.astype(np.int64).sum()) == k
    for block, shape in ((8, (5, 9)), (64, (1, 2))):
        cells = M.block_max(m, block)
        assert cells.shape == shape
        want = np.zeros(shape, np.uint32)
        want[y // block, x // block] = k
        assert np.array_equal(cells, want)
    assert M.over(m, [0, k - 1, k]).tolist() == [1, 1, 0]
    assert np.array_equal(M.block_max(m, 1), m)


@pytest.mark.parametrize("depth,white", SIX)
def test_saturation(depth, white):
    """k needs 33 bits for this pair of imaginary colours inside +-CE_LINEAR_MAX; the map holds 2^32 - 1."""
    ref, test = M.saturating_pixels(white)
    _, k = F.pixel_q20(ref.reshape(1, 1, 3), test.reshape(1, 1, 3), depth, white)
    print(f"depth {depth} white {white}: k = {int(k[0, 0])}, Delta E ITP {int(k[0, 0]) / 2 ** 20:.1f}")
    assert (1 << 32) < int(k[0, 0]) < (1 << 33)
    if (depth, white) == (10, 80.0):
        assert int(k[0, 0]) == 6861206437
    m = M.full_map(ref.reshape(1, 1, 3), test.reshape(1, 1, 3), depth, white)
    assert m.dtype == np.uint32 and int(m[0, 0]) == M.U32_MAX
    assert M.over(m, [M.U32_MAX, M.U32_MAX - 1]).tolist() == [0, 1]


def test_library_surface():
    L = ce.lib()
    for name in ("ce_batch_delta_e_itp_map", "ce_eval_pair_delta_e_itp_map"):
        assert name in ce.ABI_SYMBOLS and hasattr(L, name)
    header = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
    assert "#define CE_DELTA_E_ITP_MAX_THRESHOLDS 8\n" in header and ce.DELTA_E_ITP_MAX_THRESHOLDS == 8
    assert ce.DELTA_E_ITP_Q20 == 1 << 20
    assert callable(ce.Batch.delta_e_itp_maps) and callable(ce.Context.delta_e_itp_map)


def test_no_result_without_a_device():
    """Nothing is computed on the CPU: on a host without a device no context can be made (CE_ERR_BACKEND), and without a
    context or a batch both calls refuse and leave their outputs alone."""
    L = ce.lib()
    img = np.zeros((2, 2, 3), np.float32)
    m, thr, cnt = np.full(4, 77, np.uint32), np.array([0], np.uint32), np.full(1, 77, np.uint64)
    assert L.ce_batch_delta_e_itp_map(None, 0, 1, 10, 203.0, 1, m.ctypes.data, 4, thr.ctypes.data, 1, cnt.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_delta_e_itp_map(None, img.ctypes.data, img.nbytes, img.ctypes.data, img.nbytes, 2, 2, 10, 203.0, 1, m.ctypes.data, 4,
                                          thr.ctypes.data, 1, cnt.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert np.all(m == 77) and cnt[0] == 77
    if ce.device_count() > 0:
        return  # the rest is what a host without a device does
    with pytest.raises(ce.CodecEvalError) as e:
        ce.Context(0).delta_e_itp_map(img, img, 2, 2)
    assert e.value.status == ce.CE_ERR_BACKEND
