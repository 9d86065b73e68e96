"""The float resampler's definition (tests/resample_linear_restatement.py; include/ce_metrics.h: ce_resample_linear; DESIGN.md
section 17) pinned from outside the project and by hand, with no device:
  - against the installed Pillow's Image.resize on mode "F" images, bit for bit, on 5 shapes x 8 ratios x 4 filters (skipped
    where Pillow is missing), and the same restatement with `/ fs` in place of Pillow's `* (1.0 / fs)` must miss at least one;
  - against outputs of Pillow recorded in tests/golden/resample_linear_pillow.npz (make_resample_linear_golden.py) for the
    three filters whose weights use no libm call;
  - hand-derived cases: the checkerboard, constants, one pixel, the clamp;
  - the host table ce_build_resample_table_f64 (ce_tables.cpp), dumped by the stand-alone program of
    tests/cpp/resample_f32_kernel_host.cpp, equals the restatement's weights to the bit on the 19 named axis pairs of
    test_resample_kernel_host_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_f32_host as H  # noqa: E402
import resample_linear_restatement as RL  # noqa: E402
from test_resample_kernel_host_cpu import TABLE_AXES  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_restatement_equals_live_pillow_and_the_division_variant_does_not():
    pytest.importorskip("PIL")
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_resample_linear_golden import pillow_resize

    cases = divided_differs = 0
    for si, (w, h) in enumerate(RL.PILLOW_SHAPES):
        img = RL.content(w, h, seed=si)
        for num, den in RL.CASE_RATIOS:
            ow, oh = RL.scaled(w, num, den), RL.scaled(h, num, den)
            for f in RL.FILTERS:
                want = bits(pillow_resize(img, ow, oh, f))
                assert np.array_equal(bits(RL.resample(img, ow, oh, f, clamp=False)), want), (w, h, ow, oh, f)
                assert np.array_equal(bits(RL.resample(img, ow, oh, f)), want), (w, h, ow, oh, f)  # the clamp is not reached here
                if not np.array_equal(bits(RL.resample(img, ow, oh, f, clamp=False, reciprocal=False)), want):
                    assert num < den, (w, h, ow, oh, f)  # fs = 1 when enlarging: the two are the same operation
                    divided_differs += 1
                cases += 1
    assert cases == 160
    assert divided_differs >= 1  # what the reciprocal is for


def test_restatement_equals_recorded_pillow():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    g = np.load(os.path.join(HERE, "golden", "resample_linear_pillow.npz"))
    n = 0
    for i in range(3):
        img = g[f"in_{i}"]
        h, w = img.shape[:2]
        assert np.array_equal(bits(img), bits(RL.content(w, h, seed=i)))
        for num, den in RL.CASE_RATIOS:
            for f in (RL.BOX, RL.BILINEAR, RL.BICUBIC):
                got = RL.resample(img, RL.scaled(w, num, den), RL.scaled(h, num, den), f)
                assert np.array_equal(bits(got), bits(g[f"out_{i}_{num}_{den}_{f}"])), (i, num, den, f)
                n += 1
    assert n == 72 and len(g.files) == 75


def test_checkerboard_halves_to_exactly_half_under_box():
    y, x = np.mgrid[0:16, 0:24]
    img = np.repeat(((x + y) & 1).astype(np.float32)[..., None], 3, axis=2)
    out = RL.resample(img, 12, 8, RL.BOX)
    assert out.shape == (8, 12, 3) and (out == np.float32(0.5)).all()
    # the 8-bit route averages sRGB code values instead: 0 / 255 -> code 128, which is 0.2158 in linear light
    assert abs(((128 / 255 + 0.055) / 1.055) ** 2.4 - 0.2158) < 1e-4


@pytest.mark.parametrize("value", [0.7, 125.0, -3.25, 1.0e-3])
def test_constant_image_stays_constant_to_the_bit(value):
    # the weights of an output sample sum to 1 within a few ulp of f64 and the input is an f32: the f64 sum lies within
    # ~ksize * 2^-52 (relative) of that f32, far inside its rounding interval, so every filter returns it exactly
    w, h = 21, 13
    img = np.full((h, w, 3), value, np.float32)
    for num, den in RL.CASE_RATIOS:
        for f in RL.FILTERS:
            out = RL.resample(img, RL.scaled(w, num, den), RL.scaled(h, num, den), f)
            assert (bits(out) == bits(np.float32(value))).all(), (value, num, den, f)


def test_one_pixel_to_any_size():
    img = np.array([[[0.25, -2.0, 125.0]]], np.float32)
    for ow, oh in ((1, 1), (5, 3), (1, 7), (64, 1)):
        for f in RL.FILTERS:
            out = RL.resample(img, ow, oh, f)
            assert out.shape == (oh, ow, 3) and np.array_equal(bits(out), bits(np.broadcast_to(img, (oh, ow, 3)))), (ow, oh, f)


def test_lanczos_overshoot_is_clamped_to_linear_max():
    img = np.zeros((4, 32, 3), np.float32)
    img[:, 16:] = 1023.0
    free = RL.resample(img, 48, 4, RL.LANCZOS3, clamp=False)
    out = RL.resample(img, 48, 4, RL.LANCZOS3)
    assert free.max() > RL.LINEAR_MAX and free.min() < 0.0  # ringing on both sides of the edge
    assert out.max() == np.float32(RL.LINEAR_MAX) and out.min() == free.min()
    inside = np.abs(free) <= RL.LINEAR_MAX
    assert np.array_equal(bits(out[inside]), bits(free[inside]))
    # equal sizes are a copy: not clamped
    big = np.full((2, 2, 3), 5000.0, np.float32)
    assert np.array_equal(bits(RL.resample(big, 2, 2)), bits(big))


def test_host_table_equals_the_restatement_weights(tmp_path):
    assert len(TABLE_AXES) == 19
    exe = H.build(tmp_path)
    jobs = [(a, b, f) for a, b in TABLE_AXES for f in RL.FILTERS]
    rd, _ = H.run(exe, tmp_path, [f"table {a} {b} {f}" for a, b, f in jobs], b"")
    for n_in, n_out, filt in jobs:
        H.check_table(rd, n_in, n_out, filt)
    assert rd.pos == rd.raw.size
    # the reciprocal shows in the table itself: with the division some weights differ in their last bits
    ours = [w for _, ws in RL.taps(512, 171, RL.BILINEAR) for w in ws]
    divided = [w for _, ws in RL.taps(512, 171, RL.BILINEAR, reciprocal=False) for w in ws]
    assert len(ours) == len(divided) and ours != divided
