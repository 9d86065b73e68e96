"""CPU checks of the viewing simulation: the resampler's restatement (tests/resample_restatement.py) on hand-derived cases,
against Pillow's recorded outputs (tests/golden/resample_pillow.npz) and, where PIL is installed, against Pillow itself;
codec-eval_amd/viewing.py against every number src/viewing.rs's own tests and doc examples pin (transcribed as data);
the ABI's enum values and the refusals that need no device."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_restatement as R  # noqa: E402

V = importlib.import_module("codec-eval_amd.viewing")
Mode, VC, presets = V.SimulationMode, V.ViewingCondition, V.presets


# ---- the restatement on cases derived by hand ------------------------------------------------------------------------
def test_box_two_to_one_is_the_rounded_mean():
    # scale 2, support 1: taps {2xx, 2xx + 1}, both weight 1/2 = 2^21: (2^21 + 2^21 (a + b)) >> 22 = (a + b + 1) >> 1
    assert R.taps(8, 4, R.BOX) == [(2 * x, [1 << 21, 1 << 21]) for x in range(4)]
    img = R.content(16, 10, "noise")
    a = img.astype(np.int32)
    got = R.resample(img, 8, 5, R.BOX)
    hor = (a[:, 0::2] + a[:, 1::2] + 1) >> 1
    assert np.array_equal(got, ((hor[0::2] + hor[1::2] + 1) >> 1).astype(np.uint8))
    assert np.array_equal(R.resample(img, 8, 10, R.BOX), hor.astype(np.uint8))


@pytest.mark.parametrize("filt", R.FILTERS)
def test_equal_size_is_identity(filt):
    img = R.content(23, 17, "noise")
    assert np.array_equal(R.resample(img, 23, 17, filt), img)


@pytest.mark.parametrize("filt", R.FILTERS)
def test_constant_image_stays_constant(filt):
    # the integer weights of a sample sum to 2^22 up to their rounding; |sum - 2^22| <= taps / 2 and v * that is far below 2^21
    for v in (0, 1, 127, 200, 255):
        img = np.full((12, 20, 3), v, np.uint8)
        for num, den in R.CASE_RATIOS:
            out = R.resample(img, R.scaled(20, num, den), R.scaled(12, num, den), filt)
            assert out.min() == v and out.max() == v, (filt, num, den, v)


def test_lanczos_overshoot_clips_at_a_step():
    row = np.zeros((1, 16, 3), np.uint8)
    row[:, 8:] = 255
    out = R.resample(row, 32, 1, R.LANCZOS3)[0, :, 0]
    raw = [((1 << 21) + sum(k * int(row[0, xmin + i, 0]) for i, k in enumerate(ks))) >> 22 for xmin, ks in R.taps(16, 32, R.LANCZOS3)]
    assert min(raw) < 0 and max(raw) > 255  # the kernel's negative lobes ring below 0 and above 255 ...
    assert np.array_equal(out, np.clip(raw, 0, 255))  # ... and the output is clipped, not wrapped
    assert out.min() == 0 and out.max() == 255 and out[raw.index(min(raw))] == 0 and out[raw.index(max(raw))] == 255


def test_taps_stay_inside_the_image_and_sum_to_one():
    for n_in, n_out in ((768, 256), (512, 683), (9, 27), (301, 100), (8, 3), (5, 1), (1, 7)):
        for filt in R.FILTERS:
            for xmin, ks in R.taps(n_in, n_out, filt):
                assert 0 <= xmin and len(ks) >= 1 and xmin + len(ks) <= n_in
                assert abs(sum(ks) - (1 << 22)) <= len(ks)


# ---- against Pillow ------------------------------------------------------------------------------------------------
def test_restatement_equals_pillows_recorded_outputs():
    z = np.load(os.path.join(ROOT, "tests", "golden", "resample_pillow.npz"))
    outs = [k for k in z.files if k.startswith("out_")]
    assert len(outs) == 3 * 8 * 4
    for key in outs:
        i, num, den, filt = (int(v) for v in key.split("_")[1:])
        img = z[f"in_{i}"]
        want = z[key]
        got = R.resample(img, want.shape[1], want.shape[0], filt)
        assert (R.scaled(img.shape[1], num, den), R.scaled(img.shape[0], num, den)) == (want.shape[1], want.shape[0])
        assert np.array_equal(got, want), key


def test_restatement_equals_live_pillow_on_the_384_cases():
    Image = pytest.importorskip("PIL.Image")
    pil = {R.BOX: Image.BOX, R.BILINEAR: Image.BILINEAR, R.BICUBIC: Image.BICUBIC, R.LANCZOS3: Image.LANCZOS}
    cases, max_acc = 0, [0]
    for w, h in R.CASE_SHAPES:
        for kind in ("noise", "pattern"):
            img = R.content(w, h, kind)
            for num, den in R.CASE_RATIOS:
                ow, oh = R.scaled(w, num, den), R.scaled(h, num, den)
                for filt in R.FILTERS:
                    want = np.asarray(Image.fromarray(img).resize((ow, oh), pil[filt]))
                    got = R.resample(img, ow, oh, filt, max_acc if w * h <= 100 * 76 else None)
                    assert np.array_equal(got, want), (w, h, kind, num, den, filt)
                    cases += 1
    assert cases == 384
    assert max_acc[0] < 2 ** 31  # the int32 accumulator never wraps


# ---- viewing.py against src/viewing.rs's tests and doc examples -------------------------------------------------------
def test_round_is_half_away_from_zero():
    assert [V.rust_round(x) for x in (0.5, 1.5, 2.5, -0.5, -2.5, 85.49, 85.5)] == [1, 2, 3, -1, -3, 85, 86]


def test_constructors_and_effective_ppd():
    d = VC.desktop()
    assert (d.acuity_ppd, d.browser_dppx, d.image_intrinsic_dppx, d.ppd) == (40.0, None, None, None)
    assert VC.laptop().acuity_ppd == 60.0 and VC.smartphone().acuity_ppd == 90.0 and VC.default() == d and VC.new(70.0).acuity_ppd == 70.0
    assert d.effective_ppd() == 40.0
    assert d.with_browser_dppx(2.0).with_image_intrinsic_dppx(2.0).effective_ppd() == 40.0
    assert d.with_browser_dppx(2.0).with_image_intrinsic_dppx(1.0).effective_ppd() == 20.0
    assert d.with_browser_dppx(1.0).with_image_intrinsic_dppx(2.0).effective_ppd() == 80.0
    assert d.with_browser_dppx(2.0).with_image_intrinsic_dppx(1.0).with_ppd_override(100.0).effective_ppd() == 100.0
    assert d.srcset_ratio() == 1.0
    assert d.with_browser_dppx(2.0).with_image_intrinsic_dppx(1.0).srcset_ratio() == 0.5
    assert d.with_browser_dppx(1.0).with_image_intrinsic_dppx(2.0).srcset_ratio() == 2.0


# (condition, mode) -> scale_factor, target_width, target_height, adjusted_ppd, requires_upscale, requires_downscale:
# test_simulation_accurate_undersized / _oversized, test_simulation_downsample_only_undersized / _oversized
UNDER = VC.new(40.0).with_browser_dppx(2.0).with_image_intrinsic_dppx(1.0)
OVER = VC.new(40.0).with_browser_dppx(1.0).with_image_intrinsic_dppx(2.0)
SIMULATION_CASES = [
    (UNDER, Mode.Accurate, (0.5, 500, 400, 20.0, True, False)),
    (OVER, Mode.Accurate, (2.0, 2000, 1600, 80.0, False, True)),
    (UNDER, Mode.DownsampleOnly, (1.0, 1000, 800, 20.0, False, False)),
    (OVER, Mode.DownsampleOnly, (2.0, 2000, 1600, 80.0, False, True)),
]


@pytest.mark.parametrize("cond,mode,want", SIMULATION_CASES)
def test_simulation_params_fields(cond, mode, want):
    p = cond.simulation_params(1000, 800, mode)
    assert (p.scale_factor, p.target_width, p.target_height, p.adjusted_ppd, p.requires_upscale, p.requires_downscale) == want


def test_simulation_params_helpers_and_thresholds():
    P = V.SimulationParams
    up, down = P(0.5, 500, 400, 20.0, True, False), P(2.0, 2000, 1600, 80.0, False, True)
    assert up.requires_scaling() and up.downscale_only_factor() == 0.5
    assert down.requires_scaling() and down.downscale_only_factor() == 1.0
    at = lambda ppd: P(1.0, 1000, 800, ppd, False, False)  # noqa: E731
    assert V.REFERENCE_PPD == 40.0
    assert [at(p).threshold_multiplier() for p in (40.0, 80.0, 20.0, 70.0)] == [1.0, 2.0, 0.5, 1.75]
    assert not at(40.0).requires_scaling()
    assert at(40.0).adjust_dssim_threshold(0.0003) == 0.0003
    assert at(70.0).adjust_dssim_threshold(0.0003) == 0.0003 * 1.75 and abs(at(70.0).adjust_dssim_threshold(0.0003) - 0.000525) < 1e-12
    assert at(70.0).adjust_butteraugli_threshold(1.0) == 1.75
    # SSIMULACRA2: higher is better; 90 stays 90 at the reference, falls at 80 PPD, rises at 20 PPD and is clamped to [0, 100]
    assert at(40.0).adjust_ssimulacra2_threshold(90.0) == 90.0
    assert at(80.0).adjust_ssimulacra2_threshold(90.0) == 90.0 - 10.0 * 0.5 == 85.0
    assert at(20.0).adjust_ssimulacra2_threshold(90.0) == 100.0  # 90 + 10 * (2 - 1): at the clamp
    assert at(10.0).adjust_ssimulacra2_threshold(90.0) == 100.0  # 90 + 10 * 3 = 120, clamped
    assert at(4000.0).adjust_ssimulacra2_threshold(10.0) == 0.0  # 10 - 90 * 0.99 < 0, clamped
    assert abs(at(70.0).adjust_ssimulacra2_threshold(90.0) - (90.0 - 10.0 * (1.0 - 1.0 / 1.75))) < 1e-12  # ~85.7
    # test_metric_acceptable
    lap = at(70.0)
    assert lap.dssim_acceptable(0.0004, 0.0003) and not lap.dssim_acceptable(0.0006, 0.0003)
    assert lap.butteraugli_acceptable(1.5, 1.0) and not lap.butteraugli_acceptable(1.75, 1.0)
    assert lap.ssimulacra2_acceptable(86.0, 90.0) and not lap.ssimulacra2_acceptable(84.0, 90.0)
    # the doc examples of simulation_params and threshold_multiplier
    p = VC.desktop().with_browser_dppx(2.0).with_image_intrinsic_dppx(1.0).simulation_params(1000, 800, Mode.DownsampleOnly)
    assert p.scale_factor == 1.0 and p.adjusted_ppd < 40.0
    assert abs(VC.new(40.0).simulation_params(1000, 800, Mode.Accurate).threshold_multiplier() - 1.0) < 0.01
    assert VC.new(70.0).simulation_params(1000, 800, Mode.Accurate).threshold_multiplier() > 1.5
    assert VC.new(70.0).simulation_params(1000, 800, Mode.Accurate).adjust_dssim_threshold(0.0003) > 0.0003


# name -> (acuity, browser dppx, intrinsic dppx), src/viewing.rs:507-605
PRESETS = {
    "native_desktop": (40.0, 1.0, 1.0), "native_laptop": (70.0, 2.0, 2.0), "native_phone": (95.0, 3.0, 3.0),
    "srcset_1x_on_phone": (95.0, 3.0, 1.0), "srcset_1x_on_laptop": (70.0, 2.0, 1.0), "srcset_2x_on_phone": (95.0, 3.0, 2.0),
    "srcset_2x_on_desktop": (40.0, 1.0, 2.0), "srcset_2x_on_laptop_1_5x": (70.0, 1.5, 2.0), "srcset_3x_on_phone": (95.0, 3.0, 3.0),
}
ALL_ORDER = ["srcset_1x_on_phone", "srcset_1x_on_laptop", "native_desktop", "srcset_2x_on_phone", "native_laptop",
             "srcset_2x_on_desktop", "srcset_2x_on_laptop_1_5x", "native_phone"]


def test_presets_values_and_order():
    for name, (acuity, browser, intrinsic) in PRESETS.items():
        c = getattr(presets, name)()
        assert (c.acuity_ppd, c.browser_dppx, c.image_intrinsic_dppx, c.ppd) == (acuity, browser, intrinsic, None), name
        assert c.srcset_ratio() == intrinsic / browser
    assert presets.all() == [getattr(presets, n)() for n in ALL_ORDER]
    ppd = [c.effective_ppd() for c in presets.all()]
    assert ppd == sorted(ppd) and 30.0 < ppd[0] < 35.0 and ppd[1] == 35.0 and ppd[5] == 80.0 and ppd[-1] == 95.0
    assert presets.key() == [presets.native_desktop(), presets.native_laptop(), presets.native_phone()]
    assert presets.baseline() == presets.native_laptop() and presets.demanding() == presets.native_desktop()
    assert [c.effective_ppd() for c in presets.key()] == [40.0, 70.0, 95.0]


def test_displayed_size_divides_where_target_width_multiplies():
    # a 2x image on a 1x display: the reference's target is 2000 x 1600, the pixels it covers are 500 x 400
    p = OVER.simulation_params(1000, 800, Mode.Accurate)
    assert (p.target_width, p.target_height) == (2000, 1600) and p.displayed_size(1000, 800) == (500, 400)
    p = UNDER.simulation_params(1000, 800, Mode.Accurate)
    assert (p.target_width, p.target_height) == (500, 400) and p.displayed_size(1000, 800) == (2000, 1600)
    # DownsampleOnly on an undersized image: scale_factor 1, the image as it is
    assert UNDER.simulation_params(1000, 800, Mode.DownsampleOnly).displayed_size(1000, 800) == (1000, 800)
    assert VC.desktop().simulation_params(77, 33, Mode.Accurate).displayed_size(77, 33) == (77, 33)
    # 768 x 512 under the eight presets, and never below one pixel
    assert [c.simulation_params(768, 512).displayed_size(768, 512) for c in presets.all()] == [
        (2304, 1536), (1536, 1024), (768, 512), (1152, 768), (768, 512), (384, 256), (576, 384), (768, 512)]
    assert presets.srcset_2x_on_desktop().simulation_params(1, 1).displayed_size(1, 1) == (1, 1)
    assert presets.srcset_2x_on_laptop_1_5x().simulation_params(257, 129).displayed_size(257, 129) == (193, 97)  # 192.75, 96.75


# ---- the ABI without a device ----------------------------------------------------------------------------------------
def test_enum_values_and_bindings_follow_the_header(ce):
    text = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
    for name, val in (("BOX", 0), ("BILINEAR", 1), ("BICUBIC", 2), ("LANCZOS3", 3)):
        assert re.search(rf"CE_RESAMPLE_{name}\s*=\s*{val}\b", text)
        assert getattr(ce, "RESAMPLE_" + name) == val == getattr(R, name)
    for fn in ("ce_resample_rgb8", "ce_batch_resample", "ce_batch_resample_pairs"):
        assert fn in ce.ABI_SYMBOLS and hasattr(ce.lib(), fn)
        assert "src/viewing.rs" in text[:text.index(fn + "(")].rsplit("/*", 1)[1]  # each entry cites the reference
    S = importlib.import_module("codec-eval_amd.session")
    cfg = S.EvalConfig("reports")
    assert cfg.simulate_viewing is None and cfg.viewing is None and cfg.resample_filter == ce.RESAMPLE_LANCZOS3
    built = S.EvalConfig.builder().report_dir("r").viewing(presets.baseline()).simulate_viewing(Mode.Accurate).build()
    assert built.simulate_viewing is Mode.Accurate and built.viewing == presets.native_laptop()


def test_refusals_that_need_no_device(ce):
    L = ce.lib()
    a = np.zeros(8 * 8 * 3, np.uint8)
    out = np.zeros(4 * 4 * 3, np.uint8)
    assert L.ce_resample_rgb8(None, a.ctypes.data, a.size, 8, 8, 4, 4, ce.RESAMPLE_LANCZOS3, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_resample(None, None, ce.BATCH_TESTS, 0, 1, ce.RESAMPLE_LANCZOS3) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_resample_pairs(None, None, 1, 1, ce.RESAMPLE_LANCZOS3) == ce.CE_ERR_INVALID_ARG
    assert b"null" in L.ce_last_error(None)
    assert ctypes.sizeof(ctypes.c_int) == 4  # enum ce_resample_filter travels as int
