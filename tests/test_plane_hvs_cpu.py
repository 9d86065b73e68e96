"""PSNR-HVS / PSNR-HVS-M's definition (include/ce_metrics.h: ce_yuv_plane_hvs) without a device: the numpy
restatement (tests/plane_hvs_restatement.py) on the anchors worked out beforehand, its tables against JPEG's and against the
published CSFCof / MaskCof entries, its DCT literals against 30 digits and against the device header's text, its DCT against
an independent one, the block counts, the mask's two special cases, that the shared content takes every branch, and the
result struct's layout as the binding declares it."""
import ctypes as C
import io
import math
import os
import re
import sys
from decimal import Decimal, getcontext

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_hvs_cases as HK  # noqa: E402
import plane_hvs_restatement as H  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def total(q):
    return q[0] + (q[1] << 32)


def test_black_against_white_block_and_identical_images():
    """One 8 x 8 block, all 0 against all 255: only DC differs, by 8 * 255, so both sums are rint((2040 * csf[0][0])^2 * 2^20) and
    there is no AC energy to mask with"""
    a, b = np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8)
    got = H.plane_hvs([a], [b], 8, H.SUB_400, 8)
    assert total(got["hvs_q"][0]) == total(got["hvsm_q"][0]) == 11289420915398 and got["hvs_q"][0] == [11289420915398 & 0xffffffff, 11289420915398 >> 32]
    assert got["n_blocks"] == [1, 0, 0] and got["n_planes"] == 1 and got["step"] == 8
    assert abs(got["psnr_hvs"][0] - -4.1281) < 5e-5 and got["psnr_hvsm"][0] == got["psnr_hvs"][0]
    assert math.isnan(got["psnr_hvs"][1]) and math.isnan(got["psnr_hvsm"][2])
    ref = list(HK.planes(93, 67, H.SUB_420, 8)[0])
    same = H.plane_hvs(ref, ref, 8, H.SUB_420, 7)
    assert same["hvs_q"] == same["hvsm_q"] == [[0, 0]] * 3 and same["psnr_hvs"] == same["psnr_hvsm"] == [math.inf] * 3
    assert same["n_blocks"] == [117, 24, 24]


def test_the_metric_is_homogeneous_in_the_sample_scale():
    """8-bit content against the same content times 257 at 16 bits (the restatement only: the device takes no 16-bit planes)"""
    ref, test = HK.planes(93, 67, H.SUB_400, 8)
    a = H.plane_hvs(list(ref), list(test), 8, H.SUB_400, 8)
    b = H.plane_hvs([ref[0].astype(np.int64) * 257], [test[0].astype(np.int64) * 257], 16, H.SUB_400, 8)
    assert abs(a["psnr_hvs"][0] - b["psnr_hvs"][0]) < 1e-9 and abs(a["psnr_hvsm"][0] - b["psnr_hvsm"][0]) < 1e-9
    assert 20 < a["psnr_hvs"][0] < a["psnr_hvsm"][0] < 60


def test_tables_are_annex_k_and_the_published_coefficients():
    assert H.Q.shape == (8, 8) and H.Q.dtype == np.int64
    # the entries of CSFCof / MaskCof as published, to their six decimals
    for q, csf, mc in ((16, 1.608443, 0.390625), (11, 2.339554, 0.826446), (10, 2.573509, 1.000000), (24, 1.072295, 0.173611), (61, 0.421887, 0.026874)):
        k, l = np.argwhere(H.Q == q)[0]
        assert round(float(H.CSF[k, l]), 6) == csf and round(float(H.MC[k, l]), 6) == mc, q
    assert H.Q[0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61] and H.Q[7, 7] == 99 and H.Q[1, 0] == 12
    assert np.array_equal(H.CSF, 25.73509 / H.Q) and np.array_equal(H.MC, 100.0 / (H.Q * H.Q))
    # the launcher's and the host test program's copies
    for path in ("codec-eval_amd/csrc/plane_hvs.hip", "tests/cpp/plane_hvs_kernel_host.cpp"):
        text = open(os.path.join(ROOT, path)).read()
        body = re.search(r"kAnnexK\[64\] = \{(.*?)\}", text, flags=re.S).group(1)
        assert [int(v) for v in re.findall(r"\d+", body)] == H.Q.reshape(-1).tolist(), path
    try:
        from PIL import Image
    except ImportError:
        return  # that one comparison needs Pillow
    buf = io.BytesIO()
    Image.new("L", (8, 8)).save(buf, "JPEG", quality=50)
    assert list(Image.open(io.BytesIO(buf.getvalue())).quantization[0]) == H.Q.reshape(-1).tolist()


def test_dct_literals_are_the_nearest_doubles_and_the_header_has_the_same_text():
    getcontext().prec = 50

    def atan_inv(n):
        x = Decimal(1) / n
        s = t = x
        k = 1
        while abs(t) > Decimal(10) ** -45:
            t = -t / (n * n)
            k += 2
            s += t / k
        return s

    pi = 4 * (4 * atan_inv(5) - atan_inv(239))  # Machin
    assert str(pi)[:32] == "3.141592653589793238462643383279"

    def cos(x):
        s = t = Decimal(1)
        k = 0
        while abs(t) > Decimal(10) ** -45:
            k += 2
            t = -t * x * x / (k * (k - 1))
            s += t
        return s

    want = [(Decimal(1) / 8).sqrt()] + [cos(m * pi / 16) / 2 for m in range(1, 8)]
    for m in range(8):
        g = H.G[m]
        assert g == float(want[m]), m  # Decimal -> float rounds to nearest
        ulp = Decimal(math.ulp(g))
        assert abs(Decimal(g) - want[m]) <= ulp / 2 and abs(Decimal(g) - want[m]) < Decimal(10) ** -16, m
    header = open(os.path.join(ROOT, "codec-eval_amd", "csrc", "plane_hvs_kernel.h")).read()
    body = header[header.index("constexpr double hvs_g(int m)"):]
    body = body[:body.index("}")]
    assert re.findall(r"0x1\.[0-9a-f]+p-\d", body) == H.G_TEXT
    # the folding gives the cosines themselves
    for k in range(1, 8):
        for j in range(8):
            # half an ulp of a value under 1 / 2
            assert abs(Decimal(float(H.T[k][j])) - cos((2 * j + 1) * k * pi / 16) / 2) <= Decimal(2) ** -54, (k, j)
    assert (H.T[0] == H.G[0]).all() and np.allclose(H.T @ H.T.T, np.eye(8), atol=1e-15)


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_the_direct_dct_against_an_independent_one(depth):
    L = (1 << depth) - 1
    z = np.random.default_rng(depth).integers(0, L + 1, (200, 8, 8))
    got = H.dct2(z)
    # extended precision, matrix form
    n = np.arange(8, dtype=np.longdouble)
    Tm = np.cos((2 * n[None, :] + 1) * n[:, None] * np.longdouble(math.pi) / 16) / 2
    Tm[0] = np.sqrt(np.longdouble(1) / 8)
    ref = np.einsum("kr,nrc,lc->nkl", Tm, z.astype(np.longdouble), Tm)
    assert float(np.abs(got - ref).max()) <= 1e-11 * (L / 255)
    try:
        import scipy.fft
    except ImportError:
        return
    assert float(np.abs(got - scipy.fft.dctn(z.astype(np.float64), axes=(1, 2), norm="ortho")).max()) <= 1e-11 * (L / 255)


def test_block_counts_for_every_step():
    want = {(8, 8): [1] * 8, (9, 8): [2, 1, 1, 1, 1, 1, 1, 1], (15, 16): [72, 20, 9, 6, 4, 4, 4, 2], (93, 67): [5160, 1290, 580, 330, 216, 150, 117, 88]}
    for (w, h), counts in want.items():
        for step in range(1, 9):
            assert H.n_blocks_of(w, h, step) == counts[step - 1], (w, h, step)
            assert len(H.blocks_of(np.zeros((h, w), np.uint8), step)) == counts[step - 1]
    assert H.n_blocks_of(7, 100, 1) == H.n_blocks_of(100, 7, 8) == 0
    b = H.blocks_of(np.arange(15 * 16).reshape(16, 15), 7)
    assert b[1, 0, 0] == 7 and b[0, 7, 7] == 7 * 15 + 7  # (x, y) = (7, 0) second; rows are the plane's rows


def test_a_flat_block_has_no_mask_and_one_sample_gives_it_one():
    """A flat block has I(block) = 0 and pop = 0 whatever the division would say.  With one sample changed its AC energy and
    its I are positive - the block's and one quadrant's - so that side has a mask and the flat side none: M is the changed side's"""
    flat = np.full((8, 8), 100, np.int64)
    one = flat.copy()
    one[2, 5] = 140
    b = H.plane_blocks(flat, one, 8, 8)
    assert b["mask_a"][0] == 0.0 and b["mask_b"][0] > 0.0 and b["M"][0] == b["mask_b"][0] and np.isfinite(b["M"][0])
    I_whole, I_quad = 64 * (63 * 100 * 100 + 140 * 140) - (63 * 100 + 140) ** 2, 16 * (15 * 100 * 100 + 140 * 140) - (15 * 100 + 140) ** 2
    assert H.spread(one[None])[0] == I_whole and H.spread(one[None, :4, 4:])[0] == I_quad and H.spread(one[None, 4:, 4:])[0] == 0
    m = float(b["mask_b"][0] * 32.0) ** 2 / ((63.0 * I_quad) / (15.0 * I_whole))
    assert abs(m - float((((b["D_b"][0] ** 2) * H.MC).sum() - b["D_b"][0, 0, 0] ** 2 * H.MC[0, 0]))) < 1e-9 * m
    assert b["n_below"] > 0 and (b["q_hvsm"] <= b["q_hvs"]).all() and b["q_hvsm"][0, 0, 0] == b["q_hvs"][0, 0, 0] > 0
    both = H.plane_blocks(flat, flat + 3, 8, 8)
    assert both["M"][0] == 0.0 and both["n_unmasked"] == 1 and np.array_equal(both["q_hvs"], both["q_hvsm"])


def test_the_shared_content_takes_every_branch():
    """A condition on the content, not a measurement: on the planes the kernel tests score, coefficients under the mask's
    threshold, coefficients at or over it, and blocks without a mask all occur - a run that never took a branch must not pass
    for equal"""
    for w, h, sub, depth, step in ((93, 67, H.SUB_420, 8, 8), (93, 67, H.SUB_420, 8, 7), (93, 67, H.SUB_420, 10, 8), (93, 67, H.SUB_420, 12, 7)):
        ref, test = HK.planes(w, h, sub, depth)
        for p in range(3):
            b = H.plane_blocks(ref[p], test[p], depth, step)
            assert b["n_below"] > 0 and b["n_at_or_above"] > 0 and b["n_unmasked"] > 0, (w, h, depth, step, p, b["n_below"], b["n_at_or_above"], b["n_unmasked"])
    want = HK.expected(93, 67, H.SUB_420, 8, 8)
    assert want["n_blocks"] == [88, 20, 20]
    for p in range(3):
        assert 25 < want["psnr_hvs"][p] < want["psnr_hvsm"][p] < 60  # masked above unmasked, as the paper has it


def test_the_noisy_pattern_workload_of_the_definition():
    """A 93 x 67 smooth pattern plus noise against itself plus noise of sigma 4: the block counts of steps 8 / 7 / 4 / 1, PSNR-HVS
    near white noise's 10 log10(255^2 / 16) = 36.1 dB (the CSF weights average near 1), PSNR-HVS-M some 6 - 8 dB above it, and
    both branches of the threshold"""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:67, 0:93].astype(np.float64)
    s = 128 + 60 * np.sin(xx / 9) * np.cos(yy / 7) + 20 * np.sin((xx + yy) / 31)
    ref = np.clip(np.rint(s + rng.normal(0, 6, s.shape)), 0, 255).astype(np.int64)
    test = np.clip(np.rint(ref + rng.normal(0, 4, s.shape)), 0, 255).astype(np.int64)
    for step, n in ((8, 88), (7, 117), (4, 330), (1, 5160)):
        got = H.plane_hvs([ref], [test], 8, H.SUB_400, step)
        b = H.plane_blocks(ref, test, 8, step)
        assert got["n_blocks"][0] == n
        assert 35.5 < got["psnr_hvs"][0] < 37.0 and 41.5 < got["psnr_hvsm"][0] < 44.5, (step, got["psnr_hvs"][0], got["psnr_hvsm"][0])
        assert b["n_below"] > 0 and b["n_at_or_above"] > 0


def test_struct_layout_and_the_symbol(ce):
    s = ce.CePlaneHvsScores
    assert C.sizeof(s) == 176
    assert [(f[0], getattr(s, f[0]).offset) for f in s._fields_] == [
        ("hvs_q", 0), ("hvsm_q", 48), ("n_blocks", 96), ("psnr_hvs", 120), ("psnr_hvsm", 144), ("n_planes", 168), ("step", 172)]
    header = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
    body = re.search(r"typedef struct ce_plane_hvs_scores \{(.*?)\} ce_plane_hvs_scores;\s*/\* (\d+) bytes \*/", header, flags=re.S)
    fields = [re.split(r"[ \*]", f.strip())[-1].split("[")[0] for f in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if f.strip()]
    assert fields == [f[0] for f in s._fields_] and int(body.group(2)) == 176
    assert "ce_yuv_plane_hvs" in ce.ABI_SYMBOLS and C.sizeof(ce.CePlaneScores) == 512
    # without a context there is nothing to write a reason to and nothing to run on
    out = s()
    img = ce.CeYuvImage()
    assert ce.lib().ce_yuv_plane_hvs(None, 16, 16, C.byref(img), 1, C.byref(img), 1, None, 8, C.byref(out)) == ce.CE_ERR_INVALID_ARG
