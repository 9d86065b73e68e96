"""VIFp's definition (include/ce_metrics.h: ce_yuv_plane_vif) without a device: the window literals
against numpy's formula, the fixed-sequence logarithm against np.log, the numpy restatement (tests/plane_vif_restatement.py) on
anchors worked out beforehand and against a plain transcription of the MATLAB text, that the shared content takes every
exceptional branch, the size rule, and the result struct's layout as the binding declares it."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_vif_cases as VK  # noqa: E402
import plane_vif_restatement as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted({(w, h, sub, depth) for w, h, sub, depth, _, _ in VK.SHAPES})


def test_window_literals_equal_numpys_formula_bit_for_bit(ce):
    header = open(os.path.join(ROOT, "codec-eval_amd", "csrc", "plane_vif_kernel.h")).read()
    for scale, n in enumerate(V.TAPS, 1):
        want = V.window(n)
        got = ce.vif_window(scale)
        assert got.dtype == np.float64 and got.shape == (n,) and got.tobytes() == want.tobytes(), scale
        assert np.array_equal(want, want[::-1]) and abs(want.sum() - 1.0) < 1e-15
        body = re.search(r"kVifG%d\[%d\] = \{(.*?)\}" % (n, n // 2 + 1), header, flags=re.S).group(1)
        assert [float(v) for v in re.findall(r"[0-9.]+", body)] == want[:n // 2 + 1].tolist(), scale  # the text itself: repr round-trips
    # the tile the case list's two edge shapes are built on is the kernel's
    assert re.search(r"kVifTileW = (\d+), kVifTileH = (\d+);", header).groups() == (str(VK.TILE_W), str(VK.TILE_H))
    out = np.zeros(17)
    for scale in (0, 5):
        assert ce.lib().ce_vif_window(scale, out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert ce.lib().ce_vif_window(1, None) == ce.CE_ERR_INVALID_ARG


def test_ln_fixed_is_within_1e_14_relative_of_np_log_on_every_a_and_b_of_the_cases():
    worst = 0.0
    for w, h, sub, depth in CASES:
        ref, test = VK.planes(w, h, sub, depth)
        for p in range(len(ref)):
            if not V.scale_sizes(*ref[p].shape[::-1]):
                continue
            for t in V.plane_scales(ref[p], test[p], depth):
                for v in (t["a"], t["b"]):
                    assert (v >= 1.0).all() and np.isfinite(v).all()
                    want = np.log(v)
                    err = np.abs(V.ln_fixed(v) - want)
                    assert (err <= 1e-14 * want).all(), (w, h, sub, depth, p, float((err / np.maximum(want, 1e-300)).max()))
                    worst = max(worst, float((err[want > 0] / want[want > 0]).max(initial=0.0)))
    print(f"ln_fixed against np.log: worst relative error {worst:.3g}")
    assert V.ln_fixed(np.array([1.0]))[0] == 0.0 and V.ln_fixed(np.array([2.0]))[0] == 0.6931471805599453
    # the text of the device's header is hlg_pow's first half
    mine = open(os.path.join(ROOT, "codec-eval_amd", "csrc", "ln_fixed.h")).read()
    theirs = open(os.path.join(ROOT, "codec-eval_amd", "csrc", "hlg_pixel.h")).read()
    body = theirs[theirs.index("    uint64_t bits;", theirs.index("double hlg_pow(")):theirs.index("    const double ln_m")]
    assert body in mine


def luma(ref, test, depth=8):
    return V.plane_vif([np.asarray(ref)], [np.asarray(test)], depth, V.SUB_400)


def test_anchors_identity_shift_constant_inversion_and_contrast_stretch():
    base = K.planes(93, 67, V.SUB_400, 8)[0][0].astype(np.int64)
    ref = 64 + 2 * (base // 4)  # 64 .. 190, even: room to shift and to stretch without clipping
    same = luma(ref, ref)
    assert abs(same["vifp"][0] - 1.0) < 1e-8 and all(abs(v - 1.0) < 1e-8 for v in same["vif_scale"][0])  # g = 1 - 1e-10 / s1
    shifted = luma(ref, ref + 40)
    assert abs(shifted["vifp"][0] - 1.0) < 1e-8
    assert same["n_pos"][0] == [77 * 51, 35 * 22, 16 * 9, 7 * 4] and same["ran"] == [1, 0, 0] and same["n_planes"] == 1
    assert math.isnan(same["vifp"][1]) and same["num_q"][1] == [0] * 4
    constant = luma(ref, np.full(ref.shape, 117))
    inverted = luma(ref, 255 - ref)
    for got in (constant, inverted):
        assert got["num_q"][0] == [0, 0, 0, 0] and min(got["den_q"][0]) > 0 and got["vifp"][0] == 0.0
    assert inverted["branches"][0][0]["g_negative"] + inverted["branches"][0][0]["s1_small"] >= inverted["n_pos"][0][0]
    stretched = luma(ref, 128 + 3 * (ref - 128) // 2)
    assert (3 * (ref - 128) % 2 == 0).all() and stretched["vifp"][0] > 1.0
    # a reference with nothing to lose: 1.0 by this library's choice
    flat = luma(np.full((41, 41), 90), np.full((41, 41), 93))
    assert flat["den_q"][0] == [0] * 4 and flat["vifp"][0] == 1.0 and flat["vif_scale"][0] == [1.0] * 4
    # the same content at 10 bits, samples times 4: the same integers (x = v * 2^(8 - d) is exact)
    noisy = K.planes(93, 67, V.SUB_400, 8)[1][0].astype(np.int64)
    assert luma(ref * 4, noisy * 4, 10)["num_q"] == luma(ref, noisy)["num_q"]


def vifp_matlab(ref, dist):
    """vifp_mscale.m transcribed plainly: a 2-D window (fspecial('gaussian', N, N / 5)), filter2(..., 'valid') and log10"""
    def filter2(win, p):
        n = win.shape[0]
        oh, ow = p.shape[0] - n + 1, p.shape[1] - n + 1
        out = np.zeros((oh, ow))
        for i in range(n):
            for j in range(n):
                out += win[i, j] * p[i:i + oh, j:j + ow]
        return out

    sigma_nsq, eps = 2.0, 1e-10
    ref, dist = ref.astype(np.float64), dist.astype(np.float64)
    num = den = 0.0
    for scale in range(1, 5):
        n = 2 ** (4 - scale + 1) + 1
        y, x = np.mgrid[-(n - 1) / 2:(n - 1) / 2 + 1, -(n - 1) / 2:(n - 1) / 2 + 1]
        win = np.exp(-(x * x + y * y) / (2.0 * (n / 5.0) ** 2))
        win /= win.sum()
        if scale > 1:
            ref, dist = filter2(win, ref)[::2, ::2], filter2(win, dist)[::2, ::2]
        mu1, mu2 = filter2(win, ref), filter2(win, dist)
        sigma1_sq = filter2(win, ref * ref) - mu1 * mu1
        sigma2_sq = filter2(win, dist * dist) - mu2 * mu2
        sigma12 = filter2(win, ref * dist) - mu1 * mu2
        sigma1_sq[sigma1_sq < 0] = 0
        sigma2_sq[sigma2_sq < 0] = 0
        g = sigma12 / (sigma1_sq + eps)
        sv_sq = sigma2_sq - g * sigma12
        g[sigma1_sq < eps] = 0
        sv_sq[sigma1_sq < eps] = sigma2_sq[sigma1_sq < eps]
        sigma1_sq[sigma1_sq < eps] = 0
        g[sigma2_sq < eps] = 0
        sv_sq[sigma2_sq < eps] = 0
        sv_sq[g < 0] = sigma2_sq[g < 0]
        g[g < 0] = 0
        sv_sq[sv_sq <= eps] = eps
        num += float(np.sum(np.log10(1 + g * g * sigma1_sq / (sv_sq + sigma_nsq))))
        den += float(np.sum(np.log10(1 + sigma1_sq / sigma_nsq)))
    return num / den


@pytest.mark.parametrize("w,h", [(41, 41), (42, 57), (93, 67)])
def test_a_plain_transcription_of_the_matlab_text_agrees(w, h):
    """Each quantised term errs by at most 2^-25 nat, so the two sums by at most 2^-25 n_total each and their ratio (vifp <= about
    1 here) by at most 2^-24 n_total / den_nats; 1e-12 covers the two summation orders"""
    ref, test = VK.planes(w, h, V.SUB_400, 8)
    got = luma(ref[0], test[0])
    n_total, den_nats = sum(got["n_pos"][0]), sum(got["den_q"][0]) / 2.0 ** 24
    want = vifp_matlab(ref[0], test[0])
    bound = 2.0 ** -24 * n_total / den_nats + 1e-12
    print(f"{w} x {h}: restatement {got['vifp'][0]!r} transcription {want!r} gap {abs(got['vifp'][0] - want):.3g} bound {bound:.3g}")
    assert abs(got["vifp"][0] - want) <= bound


def test_the_shared_content_takes_every_branch_at_scale_1_and_no_luma_denominator_is_zero():
    """A condition on the content, not a measurement: a run that never took a branch must not pass for equal"""
    taken = dict.fromkeys(V.BRANCHES, 0)
    for w, h, sub, depth in CASES:
        want = VK.expected(w, h, sub, depth)
        assert min(want["den_q"][0]) > 0 and want["ran"][0] == 1, (w, h, sub, depth)
        for p in range(want["n_planes"]):
            if want["ran"][p]:
                for k in V.BRANCHES:
                    taken[k] += want["branches"][p][0][k]
    print("positions at scale 1 over the cases:", taken)
    assert all(v > 0 for v in taken.values()), taken
    full = VK.expected(131, 99, V.SUB_420, 8)
    assert full["ran"] == [1, 1, 1] and all(full["branches"][0][0][k] > 0 for k in V.BRANCHES), full["branches"][0][0]
    assert VK.expected(41, 41, V.SUB_420, 8)["ran"] == [1, 0, 0] and VK.expected(82, 82, V.SUB_420, 8)["ran"] == [1, 1, 1]
    assert VK.expected(41, 41, V.SUB_400, 8)["n_pos"][0] == [625, 81, 9, 1]


def test_the_size_rule_40_refuses_and_41_runs():
    assert V.scale_sizes(40, 41) == [] and V.scale_sizes(41, 40) == [] and V.scale_sizes(40, 400) == []
    assert V.scale_sizes(41, 41) == [(41, 41), (17, 17), (7, 7), (3, 3)]
    assert V.scale_sizes(42, 57) == [(42, 57), (17, 25), (7, 11), (3, 5)]
    with pytest.raises(AssertionError):
        luma(np.zeros((41, 40), np.uint8), np.zeros((41, 40), np.uint8))
    # a chroma plane of 40 x 41 does not run beside a luma that does
    ref, test = K.planes(80, 82, V.SUB_420, 8)
    got = V.plane_vif(list(ref), list(test), 8, V.SUB_420)
    assert got["ran"] == [1, 0, 0] and got["n_pos"][1] == [0] * 4 and math.isnan(got["vif_scale"][2][3])


def test_struct_layout_and_the_symbols(ce):
    s = ce.CePlaneVifScores
    assert C.sizeof(s) == 424
    assert [(f[0], getattr(s, f[0]).offset) for f in s._fields_] == [
        ("num_q", 0), ("den_q", 96), ("n_pos", 192), ("vif_scale", 288), ("vifp", 384), ("ran", 408), ("n_planes", 420)]
    header = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
    body = re.search(r"typedef struct ce_plane_vif_scores \{(.*?)\} ce_plane_vif_scores;\s*/\* (\d+) bytes \*/", header, flags=re.S)
    fields = [re.split(r"[ \*]", f.strip())[-1].split("[")[0] for f in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if f.strip()]
    assert fields == [f[0] for f in s._fields_] and int(body.group(2)) == 424
    assert "ce_yuv_plane_vif" in ce.ABI_SYMBOLS and "ce_vif_window" in ce.ABI_SYMBOLS
    assert C.sizeof(ce.CePlaneHvsScores) == 176 and C.sizeof(ce.CePlaneScores) == 512
    # without a context there is nothing to write a reason to and nothing to run on
    out = s()
    img = ce.CeYuvImage()
    assert ce.lib().ce_yuv_plane_vif(None, 64, 64, C.byref(img), 1, C.byref(img), 1, None, C.byref(out)) == ce.CE_ERR_INVALID_ARG
