"""GMSD's definition (include/ce_metrics.h: ce_yuv_plane_gmsd) without a device: the numpy restatement
(tests/plane_gmsd_restatement.py) on values worked out by hand, its constant at the three depths, its invariance when samples
and depth scale together, the restatement against an independent transcription of the paper's MATLAB code as remembered
(scipy's convolve2d in full mode, cropped as MATLAB's 'same' crops), that the shared content reaches q = 2^32 and drives q low,
the result struct's layout as the binding declares it, and the tile constants the cases assume."""
import ctypes as C
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_gmsd_cases as GK  # noqa: E402
import plane_gmsd_restatement as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO32 = 1 << 32


def test_a_single_sample_and_an_identical_pair():
    """A 1 x 1 plane has one position whose every neighbour is outside: both gradients are 0 on both sides, so g = K / K"""
    got = G.plane_gmsd([np.array([[7]])], [np.array([[200]])], 8, G.SUB_400)
    assert got["n_pos"] == [1, 0, 0] and got["sum_q"] == [TWO32, 0, 0] and got["sum_q2"][0] == [0, 1] and got["max_dis"] == [0, 0, 0]
    assert got["gmsd"][0] == 0.0 and got["gmsm"][0] == 1.0 and math.isnan(got["gmsd"][1]) and math.isnan(got["gmsm"][2]) and got["n_planes"] == 1
    for depth in (8, 10, 12):
        ref = list(GK.planes(93, 67, G.SUB_420, depth)[0])
        same = G.plane_gmsd(ref, ref, depth, G.SUB_420)
        assert same["n_pos"] == [47 * 34, 24 * 17, 24 * 17] and same["n_planes"] == 3
        for p in range(3):
            n = same["n_pos"][p]
            assert same["sum_q"][p] == n * TWO32 and same["sum_q2"][p] == [0, n] and same["max_dis"][p] == 0
            assert same["gmsd"][p] == 0.0 and same["gmsm"][p] == 1.0


def test_a_flat_test_against_a_one_step_edge_by_hand():
    """8 x 8 at 8 bits: the reference is 100 in columns 0 - 3 and 120 in columns 4 - 7, the test 100 everywhere.  S is 4 x 4: the
    reference's columns are 400 400 480 480, the test's 400.  With zeros outside the grid a flat image still has a gradient
    along the border: 3 * 400 = 1200 across an edge, 2 * 400 = 800 both ways in a corner."""
    ref = np.full((8, 8), 100, np.int64)
    ref[:, 4:] = 120
    test = np.full((8, 8), 100, np.int64)
    assert G.sums_2x2(ref).tolist() == [[400, 400, 480, 480]] * 4 and G.sums_2x2(test).tolist() == [[400] * 4] * 4
    a_ref, a_test = G.magnitude2(ref), G.magnitude2(test)
    # the test: interior 0, edges 1200^2, corners 2 * 800^2
    assert a_test.tolist() == [[1280000, 1440000, 1440000, 1280000], [1440000, 0, 0, 1440000], [1440000, 0, 0, 1440000],
                               [1280000, 1440000, 1440000, 1280000]]
    # the reference, rows 1 and 2: left edge 0 - 3 * 400; then 1200 - 1440 twice; right edge 1440 - 0; no vertical gradient
    assert a_ref[1].tolist() == a_ref[2].tolist() == [1200 ** 2, 240 ** 2, 240 ** 2, 1440 ** 2]
    # rows 0 and 3: Gx from two rows, Gy the one row inside: corner (800, 800), then (800 - 960, 1280), (800 - 960, 1360), (960, 960)
    assert a_ref[0].tolist() == a_ref[3].tolist() == [2 * 800 ** 2, 160 ** 2 + 1280 ** 2, 160 ** 2 + 1360 ** 2, 2 * 960 ** 2]
    g, q = G.similarity(ref, test, 8)
    K = 24480
    # interior: the test is flat there, so g = K / (240^2 + K) = 17 / 57
    assert Fraction(K, 240 ** 2 + K) == Fraction(17, 57)
    assert q[1, 1] == q[1, 2] == q[2, 1] == q[2, 2] == round(Fraction(17 * TWO32, 57)) == 1280955158
    # left edge: both sides 1200 across, g = 1; right edge: 1440 against 1200
    assert q[1, 0] == q[2, 0] == TWO32
    right = Fraction(2 * 1440 * 1200 + K, 1440 ** 2 + 1200 ** 2 + K)
    assert q[1, 3] == q[2, 3] == round(right * TWO32)
    # the left corners are the same on both sides; the right ones 2 * 960^2 against 2 * 800^2: the roots' product is 2 * 960 * 800
    assert q[0, 0] == q[3, 0] == TWO32
    corner = Fraction(2 * 2 * 960 * 800 + K, 2 * 960 ** 2 + 2 * 800 ** 2 + K)
    assert abs(int(q[0, 3]) - round(corner * TWO32)) <= 1 and q[0, 3] == q[3, 3]  # sqrt(2) twice: not exact in f64
    got = G.plane_gmsd([ref], [test], 8, G.SUB_400)
    qs = [int(x) for x in q.reshape(-1)]
    assert got["sum_q"][0] == sum(qs) and got["sum_q2_int"][0] == sum(x * x for x in qs) and got["n_pos"][0] == 16
    assert got["max_dis"][0] == TWO32 - 1280955158
    mean = Fraction(sum(qs), 16 * TWO32)
    var = Fraction(sum(x * x for x in qs), 16 * TWO32 ** 2) - mean ** 2
    assert abs(got["gmsd"][0] - math.sqrt(var)) < 1e-15 and abs(got["gmsm"][0] - float(mean)) < 1e-15 and 0.2 < got["gmsd"][0] < 0.4


def test_the_constant_and_the_scale_invariance():
    assert [G.k_of(d) for d in (8, 10, 12)] == [24480, 391680, 6266880] and G.k_of(8) == 144 * 170
    ref, test = GK.planes(93, 67, G.SUB_400, 8)
    _, q8 = G.similarity(ref[0], test[0], 8)
    for d in (10, 12):
        _, qd = G.similarity(ref[0].astype(np.int64) << (d - 8), test[0].astype(np.int64) << (d - 8), d)
        assert np.array_equal(q8, qd), d


def matlab_gmsd(y1, y2):
    """The paper's code as remembered, on 8-bit-scaled float images: conv2(.., 'same') is the full convolution from row and
    column ceil((k - 1) / 2) on, which is 1 for the 2 x 2 and for the 3 x 3 kernel.  -> (quality map, its std2 with N)"""
    from scipy.signal import convolve2d

    def conv2_same(y, k):
        full = convolve2d(y, k, mode="full")
        r0, c0 = (k.shape[0] - 1 + 1) // 2, (k.shape[1] - 1 + 1) // 2
        return full[r0:r0 + y.shape[0], c0:c0 + y.shape[1]]

    T = 170.0
    dx = np.array([[1, 0, -1], [1, 0, -1], [1, 0, -1]], np.float64) / 3.0
    dy = dx.T
    ave = np.ones((2, 2)) / 4.0
    y1, y2 = conv2_same(y1, ave)[0::2, 0::2], conv2_same(y2, ave)[0::2, 0::2]
    g1 = np.sqrt(conv2_same(y1, dx) ** 2 + conv2_same(y1, dy) ** 2)
    g2 = np.sqrt(conv2_same(y2, dx) ** 2 + conv2_same(y2, dy) ** 2)
    qmap = (2.0 * g1 * g2 + T) / (g1 ** 2 + g2 ** 2 + T)
    return qmap, float(np.std(qmap))


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("kind", [GK.NOISY, GK.FLAT_TEST])
def test_the_restatement_against_a_transcription_of_the_matlab_code(depth, kind):
    w, h, sub = 93, 67, G.SUB_420
    ref, test = GK.planes(w, h, sub, depth, 0, kind)
    want = GK.expected(w, h, sub, depth, 0, None, kind)
    for p in range(3):
        scale = 2.0 ** (8 - depth)
        qmap, std = matlab_gmsd(ref[p].astype(np.float64) * scale, test[p].astype(np.float64) * scale)
        g, q = G.similarity(ref[p], test[p], depth)
        assert qmap.shape == q.shape
        float_forms = float(np.abs(g - qmap).max())
        quantised = float(np.abs(q.astype(np.float64) / 4294967296.0 - qmap).max())
        print(f"depth {depth} kind {kind} plane {p}: float forms differ by {float_forms:.3g}, quantised by {quantised:.3g}, "
              f"gmsd {want['gmsd'][p]!r} std {std!r}")
        assert quantised <= 2.0 ** -33 + 4e-15, (p, quantised)
        assert abs(want["gmsd"][p] - std) <= 2.0 ** -32, (p, want["gmsd"][p], std)
        assert abs(want["gmsm"][p] - float(qmap.mean())) <= 2.0 ** -32


def test_the_shared_content_reaches_one_and_goes_low():
    """A condition on the content, not a measurement: on the planes the kernel tests score, the flat patch gives positions
    with q = 2^32 on every plane and the noise of 4 % of L moves the smallest g well off 1 without emptying it (0.5 .. 0.99);
    the flat test drives g under 0.1"""
    for depth in (8, 10, 12):
        ref, test = GK.planes(93, 67, G.SUB_420, depth)
        flat = GK.planes(93, 67, G.SUB_420, depth, 0, GK.FLAT_TEST)[1]
        for p in range(3):
            g, q = G.similarity(ref[p], test[p], depth)
            # the patch is samples (8 .. 23, 8 .. 31), positions (4 .. 11, 4 .. 15) of S: the 6 x 10 whose neighbours all lie in
            # it are flat on both sides; a position outside it reaches 2^32 only where the two gradients happen to agree
            ones = int((q == TWO32).sum())
            assert (q[5:11, 5:15] == TWO32).all() and 60 <= ones <= 70 and 0.5 < float(g.min()) < 0.99, (depth, p, ones, float(g.min()))
            g, q = G.similarity(ref[p], flat[p], depth)
            assert float(g.min()) < 0.1 and int(q.min()) >= 1, (depth, p, float(g.min()))
        want = GK.expected(93, 67, G.SUB_420, depth)
        assert all(0.0 < want["gmsd"][p] < 0.1 and 0.9 < want["gmsm"][p] < 1.0 for p in range(3))


def test_struct_layout_and_the_symbol(ce):
    s = ce.CePlaneGmsdScores
    assert C.sizeof(s) == 160
    assert [(f[0], getattr(s, f[0]).offset) for f in s._fields_] == [
        ("sum_q", 0), ("sum_q2", 24), ("n_pos", 72), ("gmsd", 96), ("gmsm", 120), ("max_dis", 144), ("n_planes", 156)]
    header = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
    body = re.search(r"typedef struct ce_plane_gmsd_scores \{(.*?)\} ce_plane_gmsd_scores;\s*/\* (\d+) bytes \*/", header, flags=re.S)
    fields = [re.split(r"[ \*]", f.strip())[-1].split("[")[0] for f in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if f.strip()]
    assert fields == [f[0] for f in s._fields_] and int(body.group(2)) == 160
    assert "ce_yuv_plane_gmsd" in ce.ABI_SYMBOLS and hasattr(ce.lib(), "ce_yuv_plane_gmsd")
    assert "as remembered" in header[header.index("GMSD of a decoder's"):header.index("typedef struct ce_plane_gmsd_scores")]
    # without a context there is nothing to write a reason to and nothing to run on
    out = s()
    img = ce.CeYuvImage()
    assert ce.lib().ce_yuv_plane_gmsd(None, 16, 16, C.byref(img), 1, C.byref(img), 1, None, C.byref(out)) == ce.CE_ERR_INVALID_ARG
    one = ce.PlaneGmsdScores.from_c(out)
    assert one.sum_q2_int == (0, 0, 0) and one.n_planes == 0


def test_the_tile_constants_are_the_headers():
    header = open(os.path.join(ROOT, "codec-eval_amd", "csrc", "plane_gmsd_kernel.h")).read()
    m = re.search(r"constexpr uint32_t kGmsdTileW = (\d+), kGmsdTileH = (\d+);", header)
    assert (int(m.group(1)), int(m.group(2))) == (GK.TW, GK.TH)
    # every shape the issue names for the tile is there
    shapes = [(s[0], s[1]) for s in GK.SHAPES]
    for wh in ((2 * GK.TW, 2 * GK.TH), (2 * GK.TW - 1, 2 * GK.TH - 1), (2 * GK.TW + 1, 2 * GK.TH + 1), (4 * GK.TW + 2, 2)):
        assert wh in shapes
