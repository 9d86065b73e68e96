"""The plane-domain scores' definition (include/ce_metrics.h: ce_yuv_plane_fidelity) without a device: the
numpy restatement (tests/plane_fidelity_restatement.py) against values worked out by hand, against the SSIM / MS-SSIM
restatement it is built from, on the sample rule and on the level rule of the chroma planes; and the result struct's layout as
the binding declares it."""
import ctypes as C
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_restatement as M  # noqa: E402
import plane_fidelity_cases as K  # noqa: E402
import plane_fidelity_restatement as P  # noqa: E402

Q = 1 << 32


def constant(w, h, sub, v, dtype=np.uint8):
    return [np.full((ph, pw), v, dtype) for pw, ph in P.plane_sizes(w, h, sub)]


def test_constant_100_against_110_is_the_references_psnr_on_every_plane():
    """mse = 100 on every plane: 10 log10(65025 / 100) = 28.1308036086791 (the reference's own PSNR test value); the overall
    figure is the same mse, and the weighted one (6 a + a + a) / 8"""
    got = P.plane_fidelity(constant(24, 18, P.SUB_420, 100), constant(24, 18, P.SUB_420, 110), 8, P.SUB_420, 0)
    want = 10.0 * math.log10(255.0 * 255.0 / 100.0)
    assert abs(want - 28.1308036086791) < 1e-12
    assert got["psnr"] == [want] * 3 and got["psnr_overall"] == want
    assert got["psnr_weighted"] == ((6.0 * want + want) + want) / 8.0
    assert got["sse"] == [100 * 24 * 18, 100 * 12 * 9, 100 * 12 * 9] and got["n"] == [24 * 18, 12 * 9, 12 * 9] and got["n_planes"] == 3
    assert got["n_levels"] == [0, 0, 0] and all(math.isnan(v) for v in got["ssim"] + got["ms_ssim"])
    gray = P.plane_fidelity(constant(24, 18, P.SUB_400, 100), constant(24, 18, P.SUB_400, 110), 8, P.SUB_400, 0)
    assert gray["n_planes"] == 1 and gray["sse"] == [43200, 0, 0] and gray["n"] == [432, 0, 0]
    assert gray["psnr"][0] == want == gray["psnr_overall"] and math.isnan(gray["psnr"][1]) and math.isnan(gray["psnr"][2])
    assert math.isnan(gray["psnr_weighted"])


def test_identical_pair_is_infinite_and_every_position_scores_one():
    ref = list(K.planes(321, 321, P.SUB_420, 8)[0])
    got = P.plane_fidelity(ref, ref, 8, P.SUB_420, 5)
    assert got["psnr"] == [math.inf] * 3 and got["psnr_overall"] == math.inf and got["psnr_weighted"] == math.inf and got["sse"] == [0, 0, 0]
    assert got["n_levels"] == [5, 5, 5]
    for p in range(3):
        for l in range(5):
            assert got["ssim_q"][p][l] == got["cs_q"][p][l] == got["n_pos"][p][l] * Q > 0
    assert got["ssim"] == [1.0] * 3 and got["ms_ssim"] == [1.0] * 3


def test_444_planes_are_the_channels_of_the_rgb_definition():
    w, h = 176, 163
    ref, test = K.planes(w, h, P.SUB_444, 8)
    got = P.plane_fidelity(list(ref), list(test), 8, P.SUB_444, 5)
    want = M.msssim(np.stack(ref, axis=-1), np.stack(test, axis=-1), 8, 5)
    for p in range(3):
        assert got["ssim_q"][p] == [want["ssim_q"][l][p] for l in range(5)] and got["cs_q"][p] == [want["cs_q"][l][p] for l in range(5)]
        assert got["n_pos"][p] == want["n"] and got["ssim"][p] == want["ssim_rgb"][p] and got["ms_ssim"][p] == want["ms_ssim_rgb"][p]


def test_the_sample_rule_shifts_msb_aligned_samples_and_clamps_low_aligned_ones():
    rng = np.random.default_rng(5)
    v = rng.integers(0, 1024, (9, 7)).astype(np.uint16)
    assert np.array_equal(P.sample(v << 6, 10, True), v) and np.array_equal(P.sample((v << 6) | 63, 10, True), v)
    assert np.array_equal(P.sample(v << 6, 10, True), (v << 6) >> 6)
    over = np.array([[0, 1023, 1024, 4095, 65535]], np.uint16)
    assert P.sample(over, 10).tolist() == [[0, 1023, 1023, 1023, 1023]] and P.sample(over, 12).tolist() == [[0, 1023, 1024, 4095, 4095]]
    assert K.stored([v], 10, True)[0].dtype == np.uint16 and np.array_equal(P.sample(K.stored([v], 10, True)[0], 10, True), v)


def test_the_level_rule_of_the_chroma_planes():
    got = {n: P.n_levels_of(*n, P.SUB_420, 5 if min(n) > 160 else 1) for n in [(20, 20), (21, 22), (161, 161), (320, 320), (321, 321)]}
    assert got == {(20, 20): [1, 0, 0], (21, 22): [1, 1, 1], (161, 161): [5, 1, 1], (320, 320): [5, 1, 1], (321, 321): [5, 5, 5]}
    assert P.n_levels_of(321, 321, P.SUB_420, 0) == [0, 0, 0] and P.n_levels_of(321, 321, P.SUB_400, 5) == [5, 0, 0]
    assert P.n_levels_of(322, 161, P.SUB_422, 5) == [5, 5, 5] and P.n_levels_of(320, 161, P.SUB_422, 5) == [5, 1, 1]
    # refused: levels outside {0, 1, 5}, a luma plane too small for them, an empty image
    assert P.n_levels_of(160, 400, P.SUB_444, 5) is None and P.n_levels_of(10, 400, P.SUB_444, 1) is None
    assert P.n_levels_of(400, 400, P.SUB_444, 3) is None and P.n_levels_of(0, 4, P.SUB_444, 0) is None
    assert P.plane_sizes(5, 3, P.SUB_420) == [(5, 3), (3, 2), (3, 2)] and P.plane_sizes(5, 3, P.SUB_422) == [(5, 3), (3, 3), (3, 3)]


def test_struct_layout_and_the_symbol(ce):
    s = ce.CePlaneScores
    assert C.sizeof(s) == 512
    assert [(f[0], getattr(s, f[0]).offset) for f in s._fields_] == [
        ("sse", 0), ("n", 24), ("psnr", 48), ("psnr_weighted", 72), ("psnr_overall", 80), ("ssim", 88), ("ms_ssim", 112), ("ssim_q", 136),
        ("cs_q", 256), ("n_pos", 376), ("n_levels", 496), ("n_planes", 508)]
    assert "ce_yuv_plane_fidelity" in ce.ABI_SYMBOLS
    # without a context there is nothing to write a reason to and nothing to run on
    out = s()
    img = ce.CeYuvImage()
    assert ce.lib().ce_yuv_plane_fidelity(None, 16, 16, C.byref(img), 1, C.byref(img), 1, None, 0, C.byref(out)) == ce.CE_ERR_INVALID_ARG
