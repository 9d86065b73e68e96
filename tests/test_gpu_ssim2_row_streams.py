"""SSIMULACRA2's row pass on the device (ssim2.hip, k_ssim2_hblur_lds): at every scale, the five row-blurred streams
{a, b, a*a, b*b, a*b} of each XYB channel are the oracle's row pass (tests/cpp/ssim2_rows_shim.c) bit for bit.  The
shapes put the scales on the kernel's edges: HB_ROWS = 32-row blocks, 32-column chunks over a pitch of 32 * ceil(w / 32)
+ 32, level 0's launch of its own and the merged launch of levels 1..5."""
import numpy as np
import pytest

import ssim2_rows_shim as S

pytestmark = pytest.mark.gpu

# (w, h): the scales' sizes, halved with ceiling while at least 8 x 8
ROW_SHAPES = [
    (8, 8),  # the minimum: level 0 only
    (127, 31),  # 127 x 31, 64 x 16, 32 x 8: 32k - 1 / 32k columns; 31 rows
    (129, 65),  # 129 x 65, 65 x 33, 33 x 17, 17 x 9: 32k + 1 columns; 65 / 33 rows
    (130, 64),  # 130 x 64, 65 x 32, 33 x 16, 17 x 8: 32k + 2 columns; 64 / 32 rows
    (96, 33),  # 96 x 33, 48 x 17, 24 x 9: 32k columns; 33 rows
    (63, 130),  # 63 x 130, 32 x 65, 16 x 33, 8 x 17: 32k - 1 / 32k columns; a one-chunk level
    (31, 32),  # 31 x 32, 16 x 16, 8 x 8: 32k - 1 columns and a block that ends on the last row
    (125, 128),  # 125 x 128, 63 x 64, 32 x 32, 16 x 16, 8 x 8: the same edges at scale 1 (merged launch)
    (257, 260),  # 257 x 260 .. 9 x 9: all six scales, 32k + 1 columns at 257 / 129 / 65 / 33
]


def scale_sizes(w, h):
    out = []
    while w >= 8 and h >= 8 and len(out) < 6:
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.Shim(tmp_path_factory.mktemp("ssim2_rows_shim"))


def _first_difference(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size == 0:
        return None
    s, y, x = bad[0].tolist()
    return {"values": len(bad), "first": [s, y, x], "got": float(got[s, y, x]), "want": float(want[s, y, x])}


def _batch(ce, ctx, ref, tests, w, h):
    b = ce.Batch(ctx, w, h, 1, len(tests))
    b.set_reference(0, ref)
    for i, t in enumerate(tests):
        b.set_test(i, 0, t)
    return b


def _check_scale(b, shim, oracle, ref, t, w, h, s, where):
    xa, xb = S.xyb_pyramid(oracle, ref, w, h, s), S.xyb_pyramid(oracle, t, w, h, s)
    for c in range(3):
        got = b.debug_planes(s, 4, c)
        want = shim.row_streams(xa[c], xb[c])
        assert got.shape == want.shape, (where, s, c, got.shape, want.shape)
        diff = _first_difference(got, want)
        assert diff is None, (where, s, c, diff)


@pytest.mark.parametrize("w,h", ROW_SHAPES)
def test_row_streams_are_the_oracle_row_pass(gpu_ctx, ce, oracle, workloads, shim, w, h):
    """The streams of every scale s, first with the pyramid stopped after s + 1 scales (scale 0 reads u8 and has a launch
    of its own), then in one run of all scales (the merged launch of scales 1..5).  ce_debug_ssim2_planes reads pair 0,
    so the batch is built once with each of its two distorted images (4:4:4, 4:2:0) in that slot."""
    ref = workloads.make_reference(w, h, 800 + w + h)
    tests = [workloads.distort(ref, 40), workloads.distort(ref, 80, True)]
    sizes = scale_sizes(w, h)
    for k, order in enumerate((tests, tests[::-1])):
        b = _batch(ce, gpu_ctx, ref, order, w, h)
        try:
            for s in range(len(sizes)):
                b.debug_limit_scales(s + 1)
                b.run(len(order), ce.MetricConfig.ssimulacra2_only())
                _check_scale(b, shim, oracle, ref, order[0], w, h, s, (w, h, "test", k, "limit", s + 1))
        finally:
            b.close()
        b = _batch(ce, gpu_ctx, ref, order, w, h)
        try:
            b.run(len(order), ce.MetricConfig.ssimulacra2_only())
            for s in range(len(sizes)):
                _check_scale(b, shim, oracle, ref, order[0], w, h, s, (w, h, "test", k, "all scales"))
        finally:
            b.close()
