"""Matrix/TRC ICC profiles on the host, without a device: the library's parser and builders (ce_icc_describe,
ce_icc_build_matrix, ce_icc_build_tables, ce_srgb_encode_thresholds) against the numpy restatement (tests/icc_restatement.py)
to the bit, every refusal kind, the sRGB profiles as the identity on code values, and the restatement itself against
Pillow's lcms2 on random RGB8 pixels."""
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_restatement as R  # noqa: E402

import codec_eval_amd as ce  # noqa: E402

F = R.fixtures()


@pytest.mark.parametrize("name", sorted(F))
def test_describe_reads_what_the_writer_wrote(name):
    p, want = F[name], R.read_profile(F[name])
    d = ce.icc_describe(p)
    assert d.kind == ce.ICC_SUPPORTED and d.reason == ""
    assert d.version == struct.unpack_from(">I", p, 8)[0] and d.version >> 24 in (2, 4)
    assert d.profile_class == int.from_bytes(b"mntr", "big")
    assert [[d.colorants[3 * r + c] for r in range(3)] for c in range(3)] == [list(c) for c in want["colorants"]]
    for got, w in zip(d.curves, want["curves"]):
        if w[0] == "curv":
            assert (got.type, got.count) == (0, len(w[1]))
            if len(w[1]) == 1:
                assert got.params[0] == w[1][0]
            if len(w[1]) >= 2:
                assert struct.unpack_from(f">{len(w[1])}H", p, got.offset) == tuple(w[1])
        else:
            assert (got.type, got.count) == (1, w[1]) and list(got.params[:len(w[2])]) == list(w[2]) and not any(got.params[len(w[2]):])


def test_both_header_versions_are_among_the_fixtures():
    assert {ce.icc_describe(p).version >> 24 for p in F.values()} == {2, 4}


@pytest.mark.parametrize("name", sorted(F))
def test_builders_equal_the_restatement_to_the_bit(name):
    p = F[name]
    assert np.array_equal(ce.icc_matrix(p).view(np.uint32), R.matrix(p).view(np.uint32))
    for depth in R.DEPTHS:
        got, want = ce.icc_tables(p, depth), R.tables(p, depth)
        assert got.shape == want.shape == (3, 1 << depth)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), depth
        assert got.min() >= 0.0 and got.max() <= 1.0


def test_the_canonical_colorants_give_the_identity_exactly():
    for name in ("srgb_para", "srgb_para_v2", "srgb_curv1024"):
        assert np.array_equal(ce.icc_matrix(F[name]), np.eye(3, dtype=np.float32))
    for name in ("p3", "adobe", "prophoto"):
        m = ce.icc_matrix(F[name])
        assert not np.array_equal(m, np.eye(3, dtype=np.float32))
        assert np.allclose(m.sum(axis=1), 1.0, atol=2e-3)  # white stays white, to the colorants' rounding
    # Display P3 -> sRGB, both through D50-adapted colorants, against the D65 matrix of the CICP route
    assert np.allclose(ce.icc_matrix(F["p3"]), ce.colour_matrix(12), atol=2e-3)


@pytest.mark.parametrize("depth", R.DEPTHS)
def test_encode_thresholds(depth):
    t = ce.srgb_encode_thresholds(depth)
    assert t.shape == ((1 << depth) - 1,) and np.array_equal(t.view(np.uint32), R.thresholds(depth).view(np.uint32))
    assert np.all(np.diff(t) > 0) and t[0] > 0.0 and t[-1] < 1.0
    # the encode of the library's own sRGB table is the code itself
    assert np.array_equal(R.encode(ce.srgb_table(depth, 0), depth), np.arange(1 << depth))
    assert R.encode(np.array([np.nan, -1.0, 0.0, 1.0, 7.0, np.inf, -np.inf], np.float32), depth).tolist() == [0, 0, 0, (1 << depth) - 1,
                                                                                                            (1 << depth) - 1, (1 << depth) - 1, 0]


def test_builders_refuse_bad_arguments():
    p = F["p3"]
    out = np.empty(3 << 8, np.float32)
    L = ce.lib()
    assert L.ce_icc_build_tables(p, len(p), 9, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
    assert L.ce_icc_build_tables(p, len(p), 8, out.ctypes.data, out.size - 1) == ce.CE_ERR_INVALID_ARG
    assert L.ce_icc_build_tables(p, len(p), 8, out.ctypes.data, out.size) == ce.CE_OK
    assert L.ce_srgb_encode_thresholds(8, out.ctypes.data, 256) == ce.CE_ERR_INVALID_ARG
    assert L.ce_srgb_encode_thresholds(11, out.ctypes.data, 2047) == ce.CE_ERR_INVALID_ARG
    assert L.ce_icc_describe(None, 0, None) == ce.CE_ERR_INVALID_ARG
    with pytest.raises(ce.CodecEvalError, match="shorter than a header"):
        ce.icc_matrix(b"fake")
    with pytest.raises(ce.CodecEvalError):
        ce.icc_tables(b"fake", 8)


def _retag(profile: bytes, old: bytes, new: bytes) -> bytes:
    """the tag table's entry `old` renamed"""
    n = struct.unpack_from(">I", profile, 128)[0]
    for i in range(n):
        at = 132 + 12 * i
        if profile[at:at + 4] == old:
            return profile[:at] + new + profile[at + 4:]
    raise KeyError(old)


def _set_tag_field(profile: bytes, sig: bytes, field: int, value: int) -> bytes:
    """field 1: the offset, 2: the size of the tag table's entry `sig`"""
    n = struct.unpack_from(">I", profile, 128)[0]
    for i in range(n):
        at = 132 + 12 * i
        if profile[at:at + 4] == sig:
            return profile[:at + 4 * field] + struct.pack(">I", value) + profile[at + 4 * field + 4:]
    raise KeyError(sig)


def refusal_cases():
    p = F["p3"]
    gray = R.write_profile([(b"wtpt", R.xyz_tag((0xF6D6, 0x10000, 0xD32D))), (b"kTRC", R.curv_tag(gamma_u8f8=0x0233))], 4, colour_space=b"GRAY")
    return [
        ("gray", gray, ce.ICC_NOT_RGB_XYZ),
        ("lab_pcs", p[:20] + b"Lab " + p[24:], ce.ICC_NOT_RGB_XYZ),
        ("cmyk", p[:16] + b"CMYK" + p[20:], ce.ICC_NOT_RGB_XYZ),
        ("abstract_class", p[:12] + b"abst" + p[16:], ce.ICC_NOT_RGB_XYZ),
        ("a2b0", _retag(p, b"cprt", b"A2B0"), ce.ICC_LUT_BASED),
        ("a2b1", _retag(p, b"desc", b"A2B1"), ce.ICC_LUT_BASED),
        ("missing_gtrc", _retag(p, b"gTRC", b"xTRC"), ce.ICC_MALFORMED),
        ("missing_bxyz", _retag(p, b"bXYZ", b"bXYy"), ce.ICC_MALFORMED),
        ("offset_past_end", _set_tag_field(p, b"rXYZ", 1, len(p) + 4), ce.ICC_MALFORMED),
        ("unused_tag_past_end", _set_tag_field(p, b"cprt", 1, len(p) + 4), ce.ICC_MALFORMED),
        ("size_past_end", _set_tag_field(p, b"bTRC", 2, len(p)), ce.ICC_MALFORMED),
        ("offset_wraps", _set_tag_field(p, b"rTRC", 1, 0xFFFFFFF0), ce.ICC_MALFORMED),
        ("tag_count_huge", p[:128] + struct.pack(">I", 0x7FFFFFFF) + p[132:], ce.ICC_MALFORMED),
        ("size_field_past_buffer", struct.pack(">I", len(p) + 1) + p[4:], ce.ICC_MALFORMED),
        ("truncated", p[:200], ce.ICC_MALFORMED),
        ("no_acsp", p[:36] + b"xxxx" + p[40:], ce.ICC_MALFORMED),
        ("version_5", p[:8] + b"\x05" + p[9:], ce.ICC_MALFORMED),
        ("xyz_type_wrong", _retag(_retag(p, b"rXYZ", b"tmp_"), b"rTRC", b"rXYZ"), ce.ICC_MALFORMED),
        ("curv_count_huge", F["p3_gamma22"].replace(b"curv\0\0\0\0\0\0\0\x01", b"curv\0\0\0\0\x7f\xff\xff\xff"), ce.ICC_MALFORMED),
        ("curv_count_past_tag", F["p3_gamma22"].replace(b"curv\0\0\0\0\0\0\0\x01", b"curv\0\0\0\0\0\0\0\x09"), ce.ICC_MALFORMED),
        ("para_type_5", p.replace(b"para\0\0\0\0\0\x03", b"para\0\0\0\0\0\x05"), ce.ICC_MALFORMED),
        ("para_type_4_short", p.replace(b"para\0\0\0\0\0\x03", b"para\0\0\0\0\0\x04"), ce.ICC_MALFORMED),
        ("para_type_1_a_zero", R.matrix_trc_profile(R.P3_COLORANTS, R.para_tag(1, (2.4, 0.0, 0.05))), ce.ICC_MALFORMED),
        ("para_type_2_a_zero", R.matrix_trc_profile(R.P3_COLORANTS, (R.SRGB_PARA, R.para_tag(2, (2.4, 0.0, 0.0, 0.1)), R.SRGB_PARA)), ce.ICC_MALFORMED),
        ("empty", b"", ce.ICC_MALFORMED),
        ("fake", b"fake", ce.ICC_MALFORMED),
    ]


@pytest.mark.parametrize("name,profile,kind", refusal_cases(), ids=[c[0] for c in refusal_cases()])
def test_describe_returns_each_refusal_kind(name, profile, kind):
    d = ce.icc_describe(profile)
    assert d.kind == kind and d.reason, (name, d)
    out = np.zeros(9, np.float32)
    assert ce.lib().ce_icc_build_matrix(profile, len(profile), out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    big = np.zeros(3 << 8, np.float32)
    assert ce.lib().ce_icc_build_tables(profile, len(profile), 8, big.ctypes.data, big.size) == ce.CE_ERR_INVALID_ARG
    assert not out.any() and not big.any()


def test_caps_are_the_headers():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ce_metrics.h")).read()
    assert "#define CE_ICC_MAX_PROFILE_BYTES 4194304u" in text and "#define CE_ICC_MAX_CURVE_POINTS 65536u" in text
    # a curv of exactly the cap is read, one more is not; a profile over the size cap is not
    at_cap = R.matrix_trc_profile(R.SRGB_COLORANTS, R.curv_tag(samples=[min(i, 65535) for i in range(65536)]), 2)
    assert ce.icc_describe(at_cap).kind == ce.ICC_SUPPORTED
    over = R.matrix_trc_profile(R.SRGB_COLORANTS, R.curv_tag(samples=[min(i, 65535) for i in range(65537)]), 2)
    assert ce.icc_describe(over).kind == ce.ICC_MALFORMED
    p = F["p3"]
    assert ce.icc_describe(p + b"\0" * (4194304 - len(p))).kind == ce.ICC_SUPPORTED  # trailing bytes behind the size field are not read
    assert ce.icc_describe(p + b"\0" * (4194305 - len(p))).kind == ce.ICC_MALFORMED


@pytest.mark.parametrize("name,depths", [("srgb_para", (8, 10, 12, 16)), ("srgb_para_v2", (8, 10, 12, 16)), ("srgb_curv1024", (8, 10, 12))])
def test_srgb_profiles_map_every_code_to_itself(name, depths):
    for depth in depths:
        v = np.arange(1 << depth).astype(np.uint8 if depth == 8 else np.uint16)
        px = np.stack([v, v, v], axis=-1)
        out = R.to_srgb(px, F[name], depth, depth, tone_tables=ce.icc_tables(F[name], depth))
        assert np.array_equal(out, px), depth


def test_the_1024_point_curve_at_depth_16_has_its_own_precision():
    """A 1024-point u16 curve interpolated at 65536 codes does not land on the f64 sRGB curve: 15 681 codes move, by up to 6.
    That is the profile's precision, kept as it is."""
    v = np.arange(1 << 16).astype(np.uint16)
    out = R.to_srgb(np.stack([v, v, v], axis=-1), F["srgb_curv1024"], 16, 16, tone_tables=ce.icc_tables(F["srgb_curv1024"], 16))
    d = np.abs(out[:, 0].astype(np.int64) - v.astype(np.int64))
    assert int((d > 0).sum()) == 15681 and int(d.max()) == 6


@pytest.mark.parametrize("name", ["p3", "p3_gamma22", "srgb_para"])
def test_restatement_against_lcms2(name):
    """Pillow's lcms2, relative colorimetric, to the writer's sRGB profile: at most 1 code apart and at most 2 % of samples
    differing (measured: P3 0.9 %, P3 with a gamma-2.2 curv 0.8 %, sRGB none)."""
    ImageCms = pytest.importorskip("PIL.ImageCms")
    from PIL import Image

    px = np.random.default_rng(5).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    src, dst = ImageCms.ImageCmsProfile(io.BytesIO(F[name])), ImageCms.ImageCmsProfile(io.BytesIO(F["srgb_para"]))
    got = np.asarray(ImageCms.profileToProfile(Image.fromarray(px), src, dst, renderingIntent=ImageCms.Intent.RELATIVE_COLORIMETRIC))
    want = R.to_srgb(px, F[name], 8, 8, tone_tables=ce.icc_tables(F[name], 8))
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(name, "max", int(d.max()), "differing", float((d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() <= 0.02
    if name == "srgb_para":
        assert d.max() == 0
