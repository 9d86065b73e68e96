"""The HLG ingest's host side without a device: the numpy restatement (tests/hlg_restatement.py) against numbers from outside
this code - BT.2100's reference points, BT.2408's 75 % = 203 cd/m2, BT.2100's system gammas, its luminance coefficients, and
numpy.power for hlg_pow - and the library's host builders (ce_hlg_table, ce_hlg_params) against the restatement, to the bit."""
import ctypes as C
import importlib
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import hlg_restatement as H  # noqa: E402

import codec_eval_amd as ce  # noqa: E402


def test_published_points_of_the_grey_scale_at_1000_nits():
    assert H.system_gamma(1000.0) == 1.2
    assert H.grey_nits(0.0) == 0.0
    assert abs(H.grey_nits(1.0) - 1000.0) <= 1e-4
    assert abs(H.grey_nits(0.75) - 203.15) <= 0.05  # BT.2408: HDR reference white, 75 % HLG, is 203 cd/m2
    assert abs(H.grey_nits(0.5) - 1000.0 * (1.0 / 12.0) ** 1.2) <= 1e-9 and abs(H.grey_nits(0.5) - 50.697) <= 1e-3
    assert H.inverse_oetf(0.5) == 1.0 / 12.0


@pytest.mark.parametrize("peak,gamma", [(400.0, 1.0329), (1000.0, 1.2), (2000.0, 1.3264)])
def test_derived_system_gamma(peak, gamma):
    assert abs(H.system_gamma(peak) - gamma) <= 5e-5
    assert H.system_gamma(peak, 1.1) == float(np.float32(1.1))


def test_hlg_pow_against_numpy_power():
    """Relative error <= 1e-13 against numpy.power (itself good to ~1e-16) on a dense log-uniform sample of [2^-40, 2] for
    exponents across [-0.2, 0.6]; exactly 1.0 at exponent 0."""
    rng = np.random.default_rng(2100)
    x = np.concatenate([np.exp2(rng.uniform(-40.0, 1.0, 400000)), np.exp2(np.arange(-40.0, 2.0)), [2.0 ** -40, 2.0, np.sqrt(2.0), np.sqrt(0.5)]])
    worst = 0.0
    for g in np.concatenate([np.linspace(-0.2, 0.6, 33), [H.system_gamma(p) - 1.0 for p in (400.0, 1000.0, 2000.0, 4000.0)]]):
        want = np.power(x, g)
        worst = max(worst, float(np.max(np.abs(H.hlg_pow(x, g) - want) / want)))
    print(f"hlg_pow: worst relative error against numpy.power {worst:.3e}")
    assert worst <= 1e-13
    assert np.all(H.hlg_pow(x, 0.0) == 1.0)


@pytest.mark.parametrize("depth", H.DEPTHS)
def test_table_equals_restatement_with_its_pinned_entries(depth):
    t, want = ce.hlg_table(depth), H.hlg_table(depth)
    assert t.dtype == np.float32 and np.array_equal(t.view(np.uint32), want.view(np.uint32))
    maxv, half = (1 << depth) - 1, 1 << (depth - 1)
    assert t[0] == 0.0 and t[maxv] == np.float32(1.0) and np.all(np.diff(t) > 0)
    assert H.inverse_oetf(1.0) > 1.0 and abs(H.inverse_oetf(1.0) - 1.00000003) < 1e-8  # the f64 value rounds to 1.0f
    # maxv is odd, so x = 1/2 - where the two branches meet at 1/12 - lies between code points half - 1 and half
    assert t[half - 1] < np.float32(1.0 / 12.0) < t[half]
    assert t[half - 1] == np.float32(((half - 1) / maxv) ** 2 / 3.0)


@pytest.mark.parametrize("primaries", H.PRIMARIES)
@pytest.mark.parametrize("peak,gamma,white", [(1000.0, 0.0, 203.0), (400.0, 0.0, 100.0), (4000.0, 0.0, 203.0), (600.0, 1.0, 600.0),
                                              (1000.0, 1.2, 80.0), (2000.0, 0.8, 203.0), (250.0, 1.5, 250.0)])
def test_params_equal_restatement_to_the_bit(primaries, peak, gamma, white):
    got = ce.hlg_params(ce.HlgDescription(primaries, 10, peak, gamma, white))
    want = np.array(H.hlg_params(primaries, peak, gamma, white), np.float64)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)


def test_bt2100_luminance_coefficients():
    kr, kg, kb = H.luminance_coefficients(9)
    assert (round(kr, 4), round(kg, 4), round(kb, 4)) == (0.2627, 0.6780, 0.0593)
    assert tuple(round(v, 4) for v in H.luminance_coefficients(1)) == (0.2126, 0.7152, 0.0722)
    for p in H.PRIMARIES:
        assert abs(sum(H.luminance_coefficients(p)) - 1.0) <= 1e-15
        assert tuple(ce.hlg_params(ce.HlgDescription(p))[:3]) == H.luminance_coefficients(p)


@pytest.mark.parametrize("depth", H.DEPTHS)
def test_identity_case_is_the_table(depth):
    """system_gamma = 1 with peak == white makes k exactly 1.0f: for primaries 1 the output is the table, bit for bit."""
    rng = np.random.default_rng(depth)
    px = rng.integers(0, 1 << depth, (64, 3)).astype(np.uint16)
    px[0] = 0
    px[1] = (1 << depth) - 1
    out = H.to_linear(px, 1, depth, 600.0, 1.0, 600.0)
    assert np.array_equal(out.view(np.uint32), H.hlg_table(depth)[px].view(np.uint32))
    p = H.hlg_params(1, 600.0, 1.0, 600.0)
    assert p[3] == 0.0 and p[4] == 1.0
    assert np.all(H.ootf_scale(H.hlg_table(depth)[px[1:]], p) == np.float32(1.0)) and H.ootf_scale(H.hlg_table(depth)[px[:1]], p)[0] == 0.0


def test_restatement_pixel_rules():
    px = np.array([[0, 0, 0, 9], [2000, 1023, 1023, 0], [512, 512, 512, 1]], np.uint16)  # 2000 > maxv: clamped; alpha dropped
    out = H.to_linear(px, 9, 10)
    assert np.all(out[0] == 0.0)  # ys == 0: the scale is 0, not a power of 0
    assert abs(float(out[1, 0]) - 1000.0 / 203.0) < 1e-4 and np.allclose(out[1], out[1, 0], rtol=1e-5)  # peak white is grey
    nits = 203.0 * out[2].astype(np.float64)
    assert np.all(np.abs(nits - H.grey_nits(512 / 1023.0)) < 1e-3 * nits)
    red = H.to_linear(np.array([[1023, 0, 0]], np.uint16), 9, 10)
    assert red[0, 0] > 0.0 and red[0, 1] < 0.0 and red[0, 2] < 0.0  # BT.2020 red is outside the sRGB gamut


def test_struct_layout_and_presets():
    assert C.sizeof(ce.CeHlg) == 20
    assert [(n, getattr(ce.CeHlg, n).offset) for n, _ in ce.CeHlg._fields_] == [("primaries", 0), ("depth", 4), ("peak_nits", 8),
                                                                               ("system_gamma", 12), ("white_nits", 16)]
    d = ce.HlgDescription()
    assert (d.primaries, d.depth, d.peak_nits, d.system_gamma, d.white_nits) == (9, 10, 1000.0, 0.0, 203.0)
    assert ce.HlgDescription.BT2100_HLG == d and not d.is_srgb
    assert d.with_depth(16) == ce.HlgDescription(9, 16, 1000.0, 0.0, 203.0)
    with pytest.raises(Exception):
        d.depth = 12  # frozen
    hdr = open(os.path.join(ce.INCLUDE_DIR, "ce_metrics.h")).read()
    assert "typedef struct ce_hlg {" in hdr
    for name in ("ce_batch_set_reference_hlg", "ce_batch_set_test_hlg", "ce_hlg_to_linear", "ce_batch_set_reference_yuv_hlg",
                 "ce_batch_set_test_yuv_hlg", "ce_yuv_hlg_to_linear", "ce_hlg_table", "ce_hlg_params"):
        assert name in ce.ABI_SYMBOLS and name + "(" in hdr


def test_host_builders_refuse():
    for depth in (0, 9, 11, 17):
        with pytest.raises(ce.CodecEvalError):
            ce.hlg_table(depth)
    out = np.empty(1024, np.float32)
    assert ce.lib().ce_hlg_table(10, out.ctypes.data, 1023) == ce.CE_ERR_INVALID_ARG
    assert ce.lib().ce_hlg_table(10, None, 1024) == ce.CE_ERR_INVALID_ARG
    bad = dict(primaries=[0, 2, 5, 10], depth=[0, 9, 14], peak_nits=[0.0, -1.0, float("inf"), float("nan")],
               white_nits=[0.0, -203.0, float("inf"), float("nan")], system_gamma=[0.79, 1.61, -1.2, float("nan"), float("inf")])
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ce.CodecEvalError) as e:
                ce.hlg_params(ce.HlgDescription(**{field: v}))
            assert e.value.status == ce.CE_ERR_INVALID_ARG, (field, v)
    for peak in (10.0, 9000.0):  # the derived gamma leaves [0.8, 1.6]: 0.36 and 1.60077
        assert not (0.8 <= H.system_gamma(peak) <= 1.6)
        with pytest.raises(ce.CodecEvalError):
            ce.hlg_params(ce.HlgDescription(peak_nits=peak))
        with pytest.raises(ValueError):
            H.hlg_params(9, peak)
    p = np.empty(5, np.float64)
    assert ce.lib().ce_hlg_params(None, p.ctypes.data_as(C.POINTER(C.c_double))) == ce.CE_ERR_INVALID_ARG
    assert ce.lib().ce_hlg_params(C.byref(ce.HlgDescription()._c()), None) == ce.CE_ERR_INVALID_ARG
    # the CICP builders still refuse transfer 18
    with pytest.raises(ce.CodecEvalError):
        ce.transfer_table(18, 10)


def test_imagedata_accepts_the_description_and_keeps_its_defaults():
    S = importlib.import_module("codec-eval_amd.session")
    for name in ("rgb", "rgba", "rgb16", "rgba16", "yuv"):
        assert inspect.signature(getattr(S.ImageData, name)).parameters["colour"].default is None
    y = inspect.signature(S.ImageData.yuv).parameters
    assert [(k, y[k].default) for k in ("subsampling", "layout", "matrix", "range", "upsample", "depth", "msb_aligned")] == \
        [("subsampling", ce.YUV_420), ("layout", ce.YUV_PLANAR), ("matrix", ce.YUV_BT601), ("range", ce.YUV_FULL), ("upsample", ce.CHROMA_TRIANGLE),
         ("depth", 8), ("msb_aligned", False)]
    hlg = ce.HlgDescription.BT2100_HLG
    a = S.ImageData.rgb16(np.zeros(12, np.uint16), 2, 2, 12, colour=hlg)
    assert a.colour == hlg.with_depth(12) and a.in_linear_light
    b = S.ImageData.rgb(np.zeros(12, np.uint8), 2, 2, colour=hlg)
    assert b.colour.depth == 8 and b.in_linear_light
    with pytest.raises(ce.MetricCalculation, match="no RGB8 form"):
        b.to_rgb8_vec()
    planes = [np.zeros((2, 2), np.uint16), np.zeros((1, 2), np.uint16)]
    c = S.ImageData.yuv(planes, 2, 2, ce.YUV_420, ce.YUV_SEMIPLANAR, ce.YUV_BT2020, ce.YUV_LIMITED, depth=10, msb_aligned=True, colour=hlg)
    assert c.colour == hlg and c.in_linear_light
    plain = S.ImageData.rgb(np.zeros(12, np.uint8), 2, 2)
    assert plain.colour is None and not plain.in_linear_light
