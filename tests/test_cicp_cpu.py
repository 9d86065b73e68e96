"""The CICP ingest's host side without a device: the numpy restatement (tests/cicp_restatement.py) against numbers from
outside this code - ST 2084's published code-value / luminance pairs, BT.2087's BT.2020 -> BT.709 matrix, the Display P3 ->
sRGB matrix - and the library's host builders (ce_transfer_table, ce_colour_matrix, ce_srgb_table) against the restatement,
entry for entry."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402

import codec_eval_amd as ce  # noqa: E402


# 10-bit full-range PQ code values and their luminance (ST 2084 / BT.2100 tables; Dolby's PQ code charts)
@pytest.mark.parametrize("code,nits,rel", [(0, 0.0, 0.0), (1023, 10000.0, 1e-12), (520, 100.2299, 1e-6), (769, 998.93, 1e-5),
                                           (593, 201.03, 1e-4)])
def test_pq_published_points(code, nits, rel):
    got = R.pq_nits(code / 1023.0)
    assert abs(got - nits) <= rel * max(nits, 1.0), (code, got, nits)


def test_pq_f64_definition():
    """The restatement's f64 curve against ST 2084's formula written independently with numpy's f64 power: 1e-9 relative."""
    e = np.arange(1024) / 1023.0
    m1, m2, c1, c2, c3 = 0.1593017578125, 78.84375, 0.8359375, 18.8515625, 18.6875
    p = e ** (1.0 / m2)
    want = 10000.0 * (np.maximum(p - c1, 0.0) / (c2 - c3 * p)) ** (1.0 / m1)
    got = np.array([R.pq_nits(float(x)) for x in e])
    assert np.all(np.abs(got - want) <= 1e-9 * np.maximum(want, 1e-30))
    assert (R.PQ_M1, R.PQ_M2, R.PQ_C1, R.PQ_C2, R.PQ_C3) == (m1, m2, c1, c2, c3)


@pytest.mark.parametrize("depth", R.DEPTHS)
@pytest.mark.parametrize("transfer,white", [(13, 203.0), (8, 203.0), (16, 203.0), (16, 80.0), (16, 10000.0)])
def test_transfer_table_equals_restatement(transfer, white, depth):
    assert np.array_equal(ce.transfer_table(transfer, depth, white), R.transfer_table(transfer, depth, white))


@pytest.mark.parametrize("depth", R.DEPTHS)
def test_srgb_transfer_is_the_rule0_table(depth):
    t = ce.srgb_table(depth, 0)
    assert np.array_equal(ce.transfer_table(13, depth), t)
    assert t[0] == 0.0 and t[-1] == 1.0 and np.all(np.diff(t) > 0)
    p = ce.srgb_table(depth, 1)
    assert p.shape == t.shape and np.max(np.abs(p - t)) < 1e-6 and not np.array_equal(p, t)


def test_srgb_table_8_and_16_share_entries():
    for rule in (0, 1):
        assert np.array_equal(ce.srgb_table(16, rule)[::257], ce.srgb_table(8, rule))


BT2087 = [[1.660491, -0.587641, -0.072850], [-0.124550, 1.132900, -0.008349], [-0.018151, -0.100579, 1.118730]]
P3_TO_SRGB = [[1.224940, -0.224940, 0.0], [-0.042057, 1.042057, 0.0], [-0.019638, -0.078636, 1.098274]]


@pytest.mark.parametrize("primaries,want", [(9, BT2087), (12, P3_TO_SRGB)])
def test_matrices_against_published(primaries, want):
    m = R.colour_matrix_f64(primaries)
    assert np.all(np.abs(m - np.array(want)) <= 1e-6), m
    assert np.array_equal(np.round(m, 4), np.round(np.array(want), 4))
    assert np.all(np.abs(m.sum(axis=1) - 1.0) <= 1e-6)
    assert np.all(np.abs(R.colour_matrix(primaries).astype(np.float64).sum(axis=1) - 1.0) <= 1e-6)


@pytest.mark.parametrize("primaries", R.PRIMARIES)
def test_colour_matrix_equals_restatement(primaries):
    assert np.array_equal(ce.colour_matrix(primaries), R.colour_matrix(primaries))
    if primaries == 1:
        assert np.array_equal(ce.colour_matrix(1), np.eye(3, dtype=np.float32))


def test_host_builders_refuse_other_code_points():
    for bad in (0, 2, 5, 10, 11):
        with pytest.raises(ce.CodecEvalError):
            ce.colour_matrix(bad)
    for bad in (1, 14, 18):  # BT.709 gamma, BT.2020 10-bit gamma, HLG
        with pytest.raises(ce.CodecEvalError):
            ce.transfer_table(bad, 10)
    with pytest.raises(ce.CodecEvalError):
        ce.transfer_table(16, 10, 0.0)
    with pytest.raises(ce.CodecEvalError):
        ce.transfer_table(13, 9)
    with pytest.raises(ce.CodecEvalError):
        ce.srgb_table(8, 2)


def test_struct_layout_and_constants():
    assert C.sizeof(ce.CeColour) == 16
    assert [(n, getattr(ce.CeColour, n).offset) for n, _ in ce.CeColour._fields_] == [("primaries", 0), ("transfer", 4), ("depth", 8),
                                                                                     ("white_nits", 12)]
    assert ce.lib().ce_pixel_bytes(ce.PIXEL_RGB_F32) == 12
    hdr = open(os.path.join(ce.INCLUDE_DIR, "ce_metrics.h")).read()
    assert "CE_PIXEL_RGB_F32 = 7" in hdr and "#define CE_LINEAR_MAX 1024.0f" in hdr
    assert ce.LINEAR_MAX == 1024.0 == float(R.LINEAR_MAX)
    assert ce.ColourDescription.BT2020_PQ == ce.ColourDescription(9, 16, 10, 203.0)
    assert ce.ColourDescription.DISPLAY_P3 == ce.ColourDescription(12, 13, 8) and ce.ColourDescription.SRGB.is_srgb
    assert ce.estimate_batch_bytes_linear(64, 64, 1, 2, ce.MetricConfig.all()) == \
        ce.estimate_batch_bytes(64, 64, 1, 2, ce.MetricConfig.all()) + 9 * 64 * 64 * 3


def test_restatement_pixel_rules():
    px = np.array([[0, 1023, 512, 7], [2000, 100, 1023, 0]], np.uint16)  # 2000 > maxv: clamped
    t = R.transfer_table(16, 10)
    lin = R.to_linear(px, 1, 16, 10)
    assert np.array_equal(lin, np.minimum(t[np.minimum(px[:, :3], 1023)], R.LINEAR_MAX))
    wide = R.to_linear(np.array([[255, 0, 0]], np.uint8), 12, 13, 8)
    assert wide[0, 0] > 1.0 and wide[0, 1] < 0.0 and wide[0, 2] < 0.0  # P3 red is outside the sRGB gamut
    s = R.sanitise(np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 0.25, -0.0], np.float32))
    assert np.array_equal(s[:6], np.array([0, 1024, -1024, 1024, -1024, 0.25], np.float32)) and np.signbit(s[6])
