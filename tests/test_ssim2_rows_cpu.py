"""SSIMULACRA2's row pass without a GPU: the shim of ssim2_rows_shim.py (which the GPU tests compare the device's
row-blurred streams with) is the first half of the oracle's blur - its row pass followed by the oracle's column pass is
ceo_ssim2_blur_plane in blur mode 1, bit for bit, for each of the five streams."""
import numpy as np
import pytest

import ssim2_rows_shim as S


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.Shim(tmp_path_factory.mktemp("ssim2_rows_shim"))


@pytest.mark.parametrize("w,h", [(8, 8), (1, 9), (9, 1), (31, 33), (65, 17), (129, 65)])
def test_row_pass_then_column_pass_is_the_oracle_blur(shim, oracle, workloads, w, h):
    ref = workloads.make_reference(w, h, 40 + w)
    t = workloads.distort(ref, 45)
    xa = S.xyb_pyramid(oracle, ref, w, h, 0)
    xb = S.xyb_pyramid(oracle, t, w, h, 0)
    for c in range(3):
        a, b = xa[c], xb[c]
        rows = shim.row_streams(a, b)
        assert rows.shape == (S.STREAMS, h, w) and rows.dtype == np.float32
        for s, src in enumerate((a, b, a * a, b * b, a * b)):
            want = oracle.ssim2_blur_plane(src, 1)
            got = shim.col_pass(rows[s])
            assert got.tobytes() == want.tobytes(), (w, h, c, s)


def test_xyb_pyramid_halves_with_ceiling(oracle, workloads):
    w, h = 129, 65
    ref = workloads.make_reference(w, h, 3)
    assert [S.xyb_pyramid(oracle, ref, w, h, s).shape for s in range(4)] == [(3, 65, 129), (3, 33, 65), (3, 17, 33), (3, 9, 17)]
    assert S.xyb_pyramid(oracle, ref, w, h, 0).tobytes() == oracle.ssim2_xyb_positive(oracle.ssim2_linear_planar(ref, w, h)).tobytes()
