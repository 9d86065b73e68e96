"""SSIM / MS-SSIM without a device (include/ce_metrics.h: ce_msssim_window, ce_msssim_levels, ce_msssim_scores; DESIGN.md section
27): the library's pure host functions against the header's literals and geometry, the numpy restatement
(tests/msssim_restatement.py) on cases whose result is known by hand, and the restatement against an independent float64
implementation in torch - conv2d with the same window, avg_pool2d(2, padding = size % 2), plain means."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as K  # noqa: E402
import msssim_restatement as M  # noqa: E402

Q = 1 << 32


def test_window_is_the_literals_symmetric_and_numpys_formula_to_an_ulp(ce):
    g = ce.msssim_window()
    assert g.dtype == np.float64 and g.shape == (11,)
    literals = [0.00102838008447911, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002, 0.2130055377112537,
                0.26601172486179436]
    assert g[:6].tolist() == literals and g.tolist() == M.G.tolist()
    assert np.array_equal(g, g[::-1])
    e = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    formula = e / e.sum()
    assert np.all(np.abs(g - formula) <= np.spacing(formula))
    assert abs(g.sum() - 1.0) <= 4 * np.finfo(np.float64).eps
    assert ce.lib().ce_msssim_window(None) == ce.CE_ERR_INVALID_ARG


def test_level_geometry_on_odd_and_even_sizes(ce):
    assert ce.msssim_levels(161, 161) == [(161, 161), (81, 81), (41, 41), (21, 21), (11, 11)]
    assert ce.msssim_levels(176, 163) == [(176, 163), (88, 82), (44, 41), (22, 21), (11, 11)]
    assert ce.msssim_levels(11, 75, 1) == [(11, 75)]
    for w, h, lv in ((161, 161, 5), (176, 163, 5), (163, 176, 5), (161, 200, 5), (192, 256, 5), (400, 399, 5), (11, 11, 1), (12, 11, 1)):
        assert ce.msssim_levels(w, h, lv) == M.levels_of(w, h, lv)
    n, lw, lh = np.zeros(1, np.uint32), np.zeros(5, np.uint32), np.zeros(5, np.uint32)
    L = ce.lib()
    for w, h, lv in ((160, 500, 5), (500, 160, 5), (10, 11, 1), (11, 10, 1), (200, 200, 0), (200, 200, 2), (200, 200, 6)):
        assert M.levels_of(w, h, lv) is None
        assert L.ce_msssim_levels(w, h, lv, n.ctypes.data, lw.ctypes.data, lh.ctypes.data) == ce.CE_ERR_INVALID_ARG, (w, h, lv)
        assert L.ce_last_error(None) != b""
    assert L.ce_msssim_levels(200, 200, 5, None, lw.ctypes.data, lh.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_msssim_levels(200, 200, 5, n.ctypes.data, None, lh.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_msssim_levels(200, 200, 5, n.ctypes.data, lw.ctypes.data, None) == ce.CE_ERR_INVALID_ARG


def test_struct_layout_and_symbols(ce):
    S = ce.CeMsssimScores
    assert C.sizeof(S) == 352
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("ms_ssim", 0), ("ssim", 8), ("ms_ssim_rgb", 16), ("ssim_rgb", 40),
                                                                  ("ssim_q", 64), ("cs_q", 184), ("n", 304), ("n_levels", 344), ("reserved", 348)]
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ce_metrics.h")).read()
    assert "} ce_msssim_scores;         /* 352 bytes */" in text
    for name in ("ce_batch_msssim", "ce_eval_pair_msssim", "ce_eval_pair_msssim_deep", "ce_msssim_window", "ce_msssim_levels"):
        assert name in ce.ABI_SYMBOLS and hasattr(ce.lib(), name)


@pytest.mark.parametrize("depth", [8, 16])
def test_identical_images_score_exactly_one(depth):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 1 << depth, (163, 161, 3)).astype(np.uint8 if depth == 8 else np.uint16)  # noise over the whole range
    f = M.msssim(img, img.copy(), depth, 5)
    assert f["n"] == [(w - 10) * (h - 10) for w, h in M.levels_of(161, 163, 5)]
    for l in range(5):
        assert f["ssim_q"][l] == [f["n"][l] * Q] * 3 and f["cs_q"][l] == [f["n"][l] * Q] * 3
    assert f["ssim"] == 1.0 and f["ms_ssim"] == 1.0 and f["ssim_rgb"] == [1.0] * 3 and f["ms_ssim_rgb"] == [1.0] * 3


def test_eleven_by_eleven_is_one_window():
    ref, test = K.pair(11, 11, 8)
    f = M.msssim(ref, test, 8, 1)
    assert f["n"] == [1, 0, 0, 0, 0] and f["n_levels"] == 1 and math.isnan(f["ms_ssim"])
    w2 = np.outer(M.G, M.G)
    for c in range(3):
        x, y = ref[:, :, c].astype(np.float64), test[:, :, c].astype(np.float64)
        mx, my = (w2 * x).sum(), (w2 * y).sum()
        sxx, syy, sxy = (w2 * x * x).sum() - mx * mx, (w2 * y * y).sum() - my * my, (w2 * x * y).sum() - mx * my
        c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        s = (2 * mx * my + c1) / (mx * mx + my * my + c1) * (2 * sxy + c2) / (sxx + syy + c2)
        assert abs(f["ssim_q"][0][c] / Q - s) <= 1e-9 and abs(f["ssim_rgb"][c] - s) <= 1e-9
        assert f["ssim_rgb"][c] == f["ssim_q"][0][c] / Q  # one position: the mean is the value


def test_checkerboard_against_its_inverse_has_negative_structure_and_ms_ssim_zero():
    a, b = K.checkerboard(192, 176)
    f = M.msssim(a, b, 8, 5)
    for l in range(3):
        assert all(v < 0 for v in f["cs_q"][l]), (l, f["cs_q"][l])
    assert f["ms_ssim"] == 0.0 and f["ms_ssim_rgb"] == [0.0] * 3
    assert f["ssim"] < 0


def torch_msssim(ref, test, depth, levels):
    """pytorch_msssim's computation in float64 with the header's window: -> (ssim_rgb, ms_ssim_rgb)"""
    import torch
    import torch.nn.functional as F

    L = float((1 << depth) - 1)
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    g = torch.tensor(M.G, dtype=torch.float64)
    x = torch.from_numpy(np.ascontiguousarray(ref.transpose(2, 0, 1)).astype(np.float64))[None]
    y = torch.from_numpy(np.ascontiguousarray(test.transpose(2, 0, 1)).astype(np.float64))[None]

    def blur(p):
        p = F.conv2d(p, g.reshape(1, 1, 11, 1).repeat(3, 1, 1, 1), groups=3)
        return F.conv2d(p, g.reshape(1, 1, 1, 11).repeat(3, 1, 1, 1), groups=3)

    ssims, css = [], []
    for l in range(levels):
        mx, my = blur(x), blur(y)
        sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
        cs = (2 * sxy + c2) / (sxx + syy + c2)
        s = (2 * mx * my + c1) / (mx * mx + my * my + c1) * cs
        ssims.append(s.mean(dim=(0, 2, 3)).numpy()), css.append(cs.mean(dim=(0, 2, 3)).numpy())
        if l + 1 < levels:
            pad = [d % 2 for d in x.shape[2:]]
            x, y = F.avg_pool2d(x, 2, padding=pad), F.avg_pool2d(y, 2, padding=pad)
    ms = None
    if levels == 5:
        vals = np.stack([np.maximum(v, 0.0) for v in css[:4]] + [np.maximum(ssims[4], 0.0)])
        ms = np.prod(vals ** np.array(M.WT)[:, None], axis=0)
    return ssims[0], ms


@pytest.mark.parametrize("w,h,depth", [(161, 161, 8), (176, 163, 8), (161, 200, 16), (192, 256, 10)])
def test_restatement_agrees_with_an_independent_float64_implementation(w, h, depth):
    """The restatement rounds every per-position value to 2^-32, an error of at most 2^-33 in a level's mean; with level means
    above 0.35 on this content (asserted) the product of the five powers moves by less than 1e-9."""
    ref, test = K.pair(w, h, depth)
    f = K.expected(w, h, depth)
    ssim, ms = torch_msssim(ref, test, depth, 5)
    means = [f["cs_q"][l][c] / Q / f["n"][l] for l in range(4) for c in range(3)] + [f["ssim_q"][4][c] / Q / f["n"][4] for c in range(3)]
    assert min(means) > 0.35, min(means)
    d1 = max(abs(f["ssim_rgb"][c] - ssim[c]) for c in range(3))
    d2 = max(abs(f["ms_ssim_rgb"][c] - ms[c]) for c in range(3))
    print(f"{w} x {h} depth {depth}: ssim {f['ssim']!r} ms_ssim {f['ms_ssim']!r}; apart from torch {d1:.2e} (SSIM) {d2:.2e} (MS-SSIM)")
    assert d1 <= 1e-9 and d2 <= 1e-9
    assert abs(f["ssim"] - ssim.mean()) <= 1e-9 and abs(f["ms_ssim"] - ms.mean()) <= 1e-9
    assert 0.35 < f["ms_ssim"] < 1.0 and f["ssim"] < f["ms_ssim"]
