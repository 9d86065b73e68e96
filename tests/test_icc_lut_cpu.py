"""LUT-based ICC profiles on the host (include/ce_metrics.h: ce_icc_lut_describe and the ce_icc_lut_build_* functions; DESIGN.md
section 23): the parser against the test-only writer, the builders against the numpy restatement to the bit, every refusal,
the restatement against lcms2, the two CLUT interpolations against hand-derived values, and two fixtures against routes that
are known already - the P3 matrix/TRC profile restated as a LUT, and the jpegli XYB shape on XYB-coded colours."""
import importlib
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hlg_restatement as H  # noqa: E402
import icc_lut_restatement as L  # noqa: E402
import icc_restatement as R  # noqa: E402

ce = importlib.import_module("codec-eval_amd")
F = L.fixtures()
F22 = R.fixtures()
SIG = lambda b: int.from_bytes(b, "big")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- describe and builders ----------------------------------------------------------------------------------------------------

def _same_curve(got, want, profile):
    """a described curve against the reader's"""
    if want[0] == "para":
        k = len(want[2])
        return got.type == 1 and got.count == want[1] and tuple(got.params[:k]) == tuple(want[2]) and not any(got.params[k:])
    samples, div = want[1], want[2]
    if got.type != (0 if div == 65535.0 else 2) or got.count != len(samples):
        return False
    if len(samples) == 1:
        return got.params[0] == samples[0]
    if len(samples) >= 2:
        raw = profile[got.offset:got.offset + len(samples) * (2 if div == 65535.0 else 1)]
        return tuple(struct.unpack(f">{len(samples)}{'H' if div == 65535.0 else 'B'}", raw)) == tuple(samples)
    return True


@pytest.mark.parametrize("name", sorted(F))
def test_describe_returns_what_the_writer_wrote(name):
    p, want = F[name], L.read_profile(F[name])
    d = ce.icc_lut_describe(p)
    assert d.kind == ce.ICC_LUT_SUPPORTED and d.reason == ""
    assert (d.pcs, d.tag, d.tag_type) == (want["pcs"], b"A2B0", want["type"])
    assert p[d.tag_offset:d.tag_offset + 4] == want["type"] and d.version >> 24 in (2, 4) and d.profile_class == SIG(p[12:16])
    stages = (ce.ICC_STAGE_A if want["a"] else 0) | (ce.ICC_STAGE_CLUT if want["clut"] else 0) | (ce.ICC_STAGE_M if want["m"] else 0) | \
        (ce.ICC_STAGE_MATRIX if want["matrix"] else 0) | ce.ICC_STAGE_B
    assert d.stages == stages
    if want["clut"]:
        grid, samples, div = want["clut"]
        assert d.grid == tuple(grid) and d.precision == (2 if div == 65535.0 else 1)
        n = samples.size * d.precision
        assert np.array_equal(np.frombuffer(p[d.clut_offset:d.clut_offset + n], ">u2" if d.precision == 2 else "u1").reshape(-1, 3), samples)
    if want["matrix"]:
        assert d.matrix == tuple(want["matrix"])
    for stage, got in (("a", d.a), ("m", d.m), ("b", d.b)):
        if want[stage]:
            assert all(_same_curve(g, w, p) for g, w in zip(got, want[stage])), stage
    # ce_icc_describe keeps its contract: an A2B tag makes an RGB / XYZ profile LUT-based to it, and it still turns a Lab
    # connection space away before it looks at the tags
    old = ce.icc_describe(p)
    if want["pcs"] == b"XYZ ":
        assert old.kind == ce.ICC_LUT_BASED and "LUT-based" in old.reason
    else:
        assert old.kind == ce.ICC_NOT_RGB_XYZ and old.reason == "the PCS is not XYZ"


@pytest.mark.parametrize("name", sorted(F))
def test_builders_equal_the_restatement_to_the_bit(name):
    p = F[name]
    for depth in R.DEPTHS:
        assert np.array_equal(bits(ce.icc_lut_input_tables(p, depth)), bits(L.input_tables(p, depth))), depth
    want = L.clut_nodes(p)
    got = ce.icc_lut_clut(p)
    assert (got is None) == (want is None)
    if want:
        assert np.array_equal(bits(got), bits(want[1])) and not got[:, 3].any()
    assert np.array_equal(bits(ce.icc_lut_matrix(p)), bits(L.matrix12(p)))
    kinds = {"identity": ce.ICC_LUT_CURVE_IDENTITY, "sampled": ce.ICC_LUT_CURVE_SAMPLED, "power": ce.ICC_LUT_CURVE_POWER}
    for g, w in zip(ce.icc_lut_curves(p), L.curves(p)):
        assert g.kind == kinds[w[0]]
        if w[0] == "sampled":
            assert np.array_equal(bits(g.samples), bits(w[1]))
        if w[0] == "power":
            assert g.ftype == w[1] and np.array_equal(bits(np.array(g.q)), bits(np.array(w[2], np.float64)))
    assert np.array_equal(bits(ce.icc_lut_pcs_matrix()), bits(L.pcs_matrix()))


def test_the_intent_selects_a2b1_and_a2b2_and_falls_back_to_a2b0():
    t0 = L.mab_tag(R.SRGB_PARA)
    t1 = L.mab_tag(R.curv_tag(gamma_u8f8=0x0200))
    p = L.lut_profile(t0, extra=[(b"A2B1", t1)])
    assert [ce.icc_lut_describe(p, i).tag for i in (0, 1, 2)] == [b"A2B0", b"A2B1", b"A2B0"]
    assert ce.icc_lut_curves(p, 1)[3].q[0] == 2.0 and ce.icc_lut_curves(p, 2)[3].ftype == 3
    assert np.array_equal(ce.icc_lut_input_tables(p, 8, 1), L.input_tables(p, 8, 1))
    with pytest.raises(ce.CodecEvalError):
        ce.icc_lut_describe(p, 3)
    only1 = L.lut_profile(t1, sig=b"A2B1")
    assert ce.icc_lut_describe(only1, 1).kind == 0 and ce.icc_lut_describe(only1, 0).kind == ce.ICC_LUT_MALFORMED


def _retagged(profile):
    at = profile.index(b"cprt", 132)
    return profile[:at] + b"A2B0" + profile[at + 4:]


def _patched(profile, tag_rel, data):
    d = ce.icc_lut_describe(profile)
    at = d.tag_offset + tag_rel
    return profile[:at] + data + profile[at + len(data):]


def test_every_refusal_has_its_kind_and_a_reason():
    ident = L._identity_clut((2, 2, 2))
    full = L.mab_tag(R.curv_tag(), a=R.curv_tag(), clut=((2, 2, 2), ident, 2), m=R.curv_tag(), matrix=L._mat_to_pcs(L.SRGB_A))
    ok = L.lut_profile(full)
    assert ce.icc_lut_describe(ok).kind == 0
    cut = L.mab_tag(R.curv_tag(), a=R.curv_tag(), clut=((3, 3, 3), L._identity_clut((3, 3, 3)), 2))
    cut = cut[:struct.unpack_from(">I", cut, 24)[0] + 20 + 100]  # the CLUT header and 100 of its 162 bytes; the A curves went with the rest
    cut = cut[:28] + struct.pack(">I", 32) + cut[32:]  # the A offset onto the B curves, which are still there
    mft = lambda wide, **kw: L.mft_tag(wide, [[0, 255 if not wide else 65535] * (128 if not wide else 1)] * 3, 2, ident, [[0, 255 if not wide else 65535] * (128 if not wide else 1)] * 3, **kw)
    cases = [
        (F22["p3"], ce.ICC_LUT_NOT_LUT, "no A2B tag"),
        (R.write_profile([(b"kTRC", R.curv_tag())], 4, colour_space=b"GRAY"), ce.ICC_LUT_NOT_LUT, "no A2B tag"),
        (L.lut_profile(full, colour_space=b"CMYK"), ce.ICC_LUT_UNSUPPORTED, "not RGB"),
        (L.lut_profile(full, pcs=b"Luv "), ce.ICC_LUT_UNSUPPORTED, "neither XYZ nor Lab"),
        (L.lut_profile(full, profile_class=b"link"), ce.ICC_LUT_UNSUPPORTED, "class"),
        (L.lut_profile(L.mab_tag(R.curv_tag(), channels=(4, 3))), ce.ICC_LUT_UNSUPPORTED, "3 input and 3 output"),
        (L.lut_profile(L.mab_tag(R.curv_tag(), channels=(3, 4))), ce.ICC_LUT_UNSUPPORTED, "3 input and 3 output"),
        (L.lut_profile(mft(True, channels=(4, 3))), ce.ICC_LUT_UNSUPPORTED, "3 input and 3 output"),
        (L.lut_profile(mft(False), b"XYZ "), ce.ICC_LUT_UNSUPPORTED, "mft1 tag with PCS XYZ"),
        (L.lut_profile(L.mab_tag(R.curv_tag(), a=R.curv_tag(), clut=((1, 2, 2), np.zeros((1, 2, 2, 3)), 2))), ce.ICC_LUT_MALFORMED, "grid size"),
        (_patched(L.lut_profile(mft(True)), 10, b"\x01"), ce.ICC_LUT_MALFORMED, "grid size"),
        (_patched(ok, struct.unpack_from(">I", full, 24)[0] + 16, b"\x03"), ce.ICC_LUT_MALFORMED, "precision"),
        (L.lut_profile(cut), ce.ICC_LUT_MALFORMED, "CLUT runs past"),
        (L.lut_profile(mft(True)[:52 + 12 + 40]), ce.ICC_LUT_MALFORMED, "CLUT runs past"),
        (L.lut_profile(mft(True)[:-2]), ce.ICC_LUT_MALFORMED, "output tables run past"),
        (L.lut_profile(mft(False)[:48 + 700], b"Lab "), ce.ICC_LUT_MALFORMED, "input tables run past"),
        (_patched(L.lut_profile(mft(True)), 48, b"\x00\x01"), ce.ICC_LUT_MALFORMED, "table count"),
        (_patched(ok, 12, struct.pack(">I", 0)), ce.ICC_LUT_MALFORMED, "no B curves"),
        (_patched(ok, 12, struct.pack(">I", 8)), ce.ICC_LUT_MALFORMED, "outside the tag"),
        (_patched(ok, 16, struct.pack(">I", len(full) + 1)), ce.ICC_LUT_MALFORMED, "outside the tag"),
        (_patched(ok, 20, struct.pack(">I", 0xFFFFFFF0)), ce.ICC_LUT_MALFORMED, "outside the tag"),
        (_patched(ok, 24, struct.pack(">I", len(full) - 8)), ce.ICC_LUT_MALFORMED, "CLUT header runs past"),
        (_patched(ok, 28, struct.pack(">I", len(full) - 4)), ce.ICC_LUT_MALFORMED, "curve element runs past"),
        (_patched(ok, 16, struct.pack(">I", len(full) - 44)), ce.ICC_LUT_MALFORMED, "matrix runs past"),
        (_patched(ok, 20, struct.pack(">I", 0)), ce.ICC_LUT_MALFORMED, "M curves without a matrix"),
        (_patched(ok, 28, struct.pack(">I", 0)), ce.ICC_LUT_MALFORMED, "A curves without a CLUT"),
        (L.lut_profile(L.mab_tag(R.para_tag(1, (2.0, 0.0, 0.5)))), ce.ICC_LUT_MALFORMED, "a = 0"),
        (L.lut_profile(L.mab_tag(b"para\0\0\0\0\0\5\0\0" + b"\0" * 28)), ce.ICC_LUT_MALFORMED, "function type"),
        (L.lut_profile(L.mab_tag(b"curv\0\0\0\0" + struct.pack(">I", 70000) + b"\0" * 140000)), ce.ICC_LUT_MALFORMED, "CE_ICC_MAX_CURVE_POINTS"),
        (L.lut_profile(L.mab_tag(b"curv\0\0\0\0" + struct.pack(">I", 5000) + b"\0" * 100)), ce.ICC_LUT_MALFORMED, "samples run past"),
        (L.lut_profile(L.mab_tag(b"XYZ \0\0\0\0" + b"\0" * 12)), ce.ICC_LUT_MALFORMED, "neither curv nor para"),
        (L.lut_profile(b"mBA " + full[4:]), ce.ICC_LUT_MALFORMED, "not of type"),
        (L.lut_profile(full[:8]), ce.ICC_LUT_MALFORMED, "under 12 bytes"),
        (_retagged(F22["p3"]), ce.ICC_LUT_MALFORMED, "not of type"),  # the "LUT-based" profiles of the matrix/TRC tests
        (_retagged(F22["srgb_para_v2"]), ce.ICC_LUT_MALFORMED, "not of type"),
        (b"fake", ce.ICC_LUT_MALFORMED, "shorter"),
        (ok[:300], ce.ICC_LUT_MALFORMED, "size field"),
        (ok[:36] + b"xxxx" + ok[40:], ce.ICC_LUT_MALFORMED, "acsp"),
        (ok[:8] + b"\x05" + ok[9:], ce.ICC_LUT_MALFORMED, "version"),
        (ok[:128] + struct.pack(">I", 5000) + ok[132:], ce.ICC_LUT_MALFORMED, "tag table"),
    ]
    for profile, kind, word in cases:
        d = ce.icc_lut_describe(profile)
        assert d.kind == kind and word in d.reason, (d.kind, d.reason, kind, word)
        for build in (lambda: ce.icc_lut_input_tables(profile, 8), lambda: ce.icc_lut_clut(profile), lambda: ce.icc_lut_matrix(profile),
                      lambda: ce.icc_lut_curves(profile)):
            with pytest.raises(ce.CodecEvalError) as e:
                build()
            assert e.value.status == ce.CE_ERR_INVALID_ARG and word in str(e.value)
    big = L.lut_profile(L.mab_tag(R.curv_tag(), a=R.curv_tag(), clut=((66, 66, 66), np.zeros((66, 66, 66, 3)), 1)))
    d = ce.icc_lut_describe(big)
    assert d.kind == ce.ICC_LUT_MALFORMED and "CE_ICC_MAX_CLUT_NODES" in d.reason
    with pytest.raises(ce.CodecEvalError):
        ce.icc_lut_input_tables(F["mab_xyz"], 9)


# ---- agreement with lcms2 ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("mab_xyz", "mab_xyz_v2", "mab_lab", "mft2_lab", "mft2_lab_v4", "mft2_xyz", "mft1_lab", "grid235", "p3_lut"))
def test_restatement_against_lcms2(name):
    """Pillow's lcms2 evaluating the profile itself (Flags.NOOPTIMIZE: no precalculated device link), relative colorimetric, to
    the writer's sRGB profile, against the tetrahedral restatement: at most 1 code apart and at most 2 % of samples differing
    (measured: mAB / XYZ 0.20 % in both header versions, mAB / Lab 0.22 %, mft2 / Lab 0.26 % in a v2 and in a v4 profile - so
    lcms2 decodes mft2's Lab by the legacy encoding in both - mft2 / XYZ 0.59 %, mft1 / Lab 0.17 %, the (2, 3, 5) grid 0.50 %,
    P3 as a LUT 0.17 %)."""
    ImageCms = pytest.importorskip("PIL.ImageCms")
    from PIL import Image

    px = np.random.default_rng(5).integers(0, 256, (256, 256, 3), dtype=np.uint8)
    src, dst = ImageCms.ImageCmsProfile(io.BytesIO(F[name])), ImageCms.ImageCmsProfile(io.BytesIO(F22["srgb_para"]))
    t = ImageCms.buildTransform(src, dst, "RGB", "RGB", renderingIntent=ImageCms.Intent.RELATIVE_COLORIMETRIC, flags=ImageCms.Flags.NOOPTIMIZE)
    got = np.asarray(ImageCms.applyTransform(Image.fromarray(px), t))
    want = L.to_srgb(px, F[name], 8, 8, interpolation=L.TETRAHEDRAL)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(name, "max", int(d.max()), "differing", float((d > 0).mean()))
    assert d.max() <= 1 and (d > 0).mean() <= 0.02


# ---- the two interpolations -------------------------------------------------------------------------------------------------------

# a 2 x 2 x 2 CLUT of one channel whose eight values tell every path apart, by (x, y, z)
CORNERS = {(0, 0, 0): 0.0, (1, 0, 0): 0.5, (0, 1, 0): 0.25, (0, 0, 1): 0.125, (1, 1, 0): 1.0, (1, 0, 1): 0.75, (0, 1, 1): 0.375, (1, 1, 1): 0.875}


def _corner_nodes():
    nodes = np.zeros((8, 4), np.float32)
    for (x, y, z), v in CORNERS.items():
        nodes[x * 4 + y * 2 + z, :3] = v
    return nodes


def test_hand_derived_values_in_each_tetrahedron_and_on_each_tie():
    """c000 + (ca - c000) hi + (cb - ca) mid + (c111 - cb) lo by hand; every number is a dyadic rational, so f32 is exact."""
    want = {
        (0.75, 0.5, 0.25): 0.5 * 0.75 + 0.5 * 0.5 - 0.125 * 0.25,     # x y z: c100, c110
        (0.75, 0.25, 0.5): 0.5 * 0.75 + 0.25 * 0.5 + 0.125 * 0.25,    # x z y: c100, c101
        (0.5, 0.25, 0.75): 0.125 * 0.75 + 0.625 * 0.5 + 0.125 * 0.25,  # z x y: c001, c101
        (0.5, 0.75, 0.25): 0.25 * 0.75 + 0.75 * 0.5 - 0.125 * 0.25,   # y x z: c010, c110
        (0.25, 0.75, 0.5): 0.25 * 0.75 + 0.125 * 0.5 + 0.5 * 0.25,    # y z x: c010, c011
        (0.25, 0.5, 0.75): 0.125 * 0.75 + 0.25 * 0.5 + 0.5 * 0.25,    # z y x: c001, c011
        (0.5, 0.5, 0.25): 0.46875, (0.75, 0.5, 0.5): 0.5625, (0.25, 0.5, 0.5): 0.3125, (0.5, 0.25, 0.5): 0.40625, (0.5, 0.5, 0.5): 0.4375,  # the ties
    }
    assert [want[k] for k in list(want)[:6]] == [0.59375, 0.53125, 0.4375, 0.53125, 0.375, 0.34375]
    a = np.array(list(want), np.float32)
    got = L.clut_interpolate((2, 2, 2), _corner_nodes(), a, L.TETRAHEDRAL)
    assert np.array_equal(got[:, 0], np.array(list(want.values()), np.float32))
    # trilinear at the centre is the mean of the eight corners; along an edge it is the edge's lerp
    tri = L.clut_interpolate((2, 2, 2), _corner_nodes(), np.array([[0.5, 0.5, 0.5], [0.25, 0, 0], [1, 1, 0.5]], np.float32), L.TRILINEAR)
    assert tri[:, 0].tolist() == [sum(CORNERS.values()) / 8, 0.125, 0.9375]


def test_both_interpolations_are_exact_at_nodes():
    rng = np.random.default_rng(2)
    grid = (3, 4, 6)
    nodes = np.zeros((72, 4), np.float32)
    nodes[:, :3] = rng.random((72, 3), np.float32)
    idx = np.stack(np.meshgrid(*[np.arange(g) for g in grid], indexing="ij"), -1).reshape(-1, 3)
    a = (idx / (np.array(grid) - 1.0)).astype(np.float32)
    keep = np.all((a * (np.array(grid, np.float32) - 1)) == idx, axis=1)  # node positions that a float32 input reaches exactly
    assert keep.sum() >= 40
    for interp in (L.TRILINEAR, L.TETRAHEDRAL):
        got = L.clut_interpolate(grid, nodes, a[keep], interp)
        assert np.array_equal(got, nodes[:, :3][keep]), interp  # the last node of an axis included: cell g - 2 with f = 1


def test_trilinear_and_tetrahedral_on_decoupled_and_on_affine_cluts():
    """Where output channel k depends on axis k alone both are c000 + (c1 - c000) f of that axis - the other differences are
    exact zeros - so they agree bit for bit; on an affine CLUT whose channels mix the axes the sums are associated differently
    and agree within rounding only: three products and three sums of values below 1, a few units of 2^-24."""
    rng = np.random.default_rng(3)
    grid = (4, 5, 3)
    h = [np.sort(rng.random(g).astype(np.float32)) for g in grid]
    idx = np.stack(np.meshgrid(*[np.arange(g) for g in grid], indexing="ij"), -1).reshape(-1, 3)
    nodes = np.zeros((60, 4), np.float32)
    for k in range(3):
        nodes[:, k] = h[k][idx[:, k]]
    a = rng.random((20000, 3), np.float32)
    a[:100] = np.round(a[:100] * 4) / 4  # ties and cell borders
    tri, tet = L.clut_interpolate(grid, nodes, a, L.TRILINEAR), L.clut_interpolate(grid, nodes, a, L.TETRAHEDRAL)
    assert np.array_equal(bits(tri), bits(tet))
    pos = idx / (np.array(grid) - 1.0)
    affine = np.zeros((60, 4), np.float32)
    affine[:, :3] = (pos @ np.array([[0.2, 0.3, 0.1], [0.1, 0.1, 0.5], [0.4, 0.2, 0.2]]) + 0.05).astype(np.float32)
    tri, tet = L.clut_interpolate(grid, affine, a, L.TRILINEAR), L.clut_interpolate(grid, affine, a, L.TETRAHEDRAL)
    worst = float(np.abs(tri.astype(np.float64) - tet).max())
    print("affine CLUT: trilinear - tetrahedral, max", worst, "differing", float((tri != tet).mean()))
    assert 0.0 < worst <= 8 * 2.0 ** -24


# ---- fixtures against known routes ------------------------------------------------------------------------------------------------

def test_the_p3_profile_restated_as_a_lut_against_the_matrix_trc_route():
    """sRGB para A curves, an identity 2 x 2 x 2 CLUT, the P3 colorants over (1 + 32767 / 32768) as the matrix: the P3 matrix/TRC
    fixture through another arithmetic.  The matrix entries are rounded to s15Fixed16, 2^-17 each at most; that is at most
    3 * 2^-17 * 2 in an XYZ component and, through inv(A) (largest absolute row sum 5.25), 2.4e-4 in linear light.  Measured
    on every code of depths 8 and 16, in grey and along each axis, with either interpolation: 4.33e-5."""
    worst = 0.0
    for depth, dt in ((8, np.uint8), (16, np.uint16)):
        v = np.arange(1 << depth)
        for pat in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1)):
            px = np.stack([v * k for k in pat], -1).astype(dt)
            want = R.to_linear(px, F22["p3"], depth).astype(np.float64)
            for interp in (L.TRILINEAR, L.TETRAHEDRAL):
                worst = max(worst, float(np.abs(L.to_linear(px, F["p3_lut"], depth, interp) - want).max()))
    print("P3 as a LUT against the matrix/TRC route: max abs difference", worst)
    assert worst <= 2.4e-4
    codes = (L.to_srgb(np.stack([np.arange(256)] * 3, -1).astype(np.uint8), F["p3_lut"], 8).astype(int)
             - R.to_srgb(np.stack([np.arange(256)] * 3, -1).astype(np.uint8), F22["p3"], 8).astype(int))
    assert np.abs(codes).max() <= 1


def test_the_xyb_shaped_profile_brings_xyb_coded_colours_back_to_linear_srgb():
    """4096 seeded sRGB colours, XYB-coded by the writer's constants into 16-bit samples.  A sample is off by at most 2^-17 of
    its range: up to 6.5e-6 in Y and B (their scales are 1.18 and 1.5), so 1.3e-5 in a cube root g <= 0.87, 3 g^2 dg = 3e-5 in a
    mixed value, and through the inverse opsin matrix (largest absolute row sum 21.2, its entries themselves rounded to 2^-17)
    6.4e-4; the bound asserted is 1e-3.  Measured: 5.6e-4 with either interpolation."""
    rng = np.random.default_rng(7)
    srgb = rng.integers(0, 256, (4096, 3))
    lin = np.array([[R._srgb_eotf(v / 255.0) for v in row] for row in srgb])
    coded = L.xyb_encode(lin)
    assert coded.min() > 0.0 and coded.max() < 1.0
    codes = np.rint(coded * 65535.0).astype(np.uint16)
    for interp in (L.TRILINEAR, L.TETRAHEDRAL):
        worst = float(np.abs(L.to_linear(codes, F["xyb"], 16, interp) - lin).max())
        print("XYB round trip: max abs error", worst)
        assert worst <= 1e-3
    d = ce.icc_lut_describe(F["xyb"])
    assert d.stages == 31 and d.grid == (2, 2, 2) and all(c.type == 1 and c.count == 2 for c in d.m)


def test_hlg_pow_over_the_bases_and_exponents_of_post_clut_curves():
    """hlg_pow is documented for g in [-0.4, 0.6]; the curves here raise to 1/3 .. 3.  Against numpy.power over bases in
    [2^-40, 2]: measured 2.2e-14 relative at most, seven orders below the float32 rounding that follows.  The bound: |g ln x|
    <= 3 * 40 * ln 2 = 83.2 there, one rounding of which is 83.2 * 2^-52 = 1.85e-14 of the result, on top of hlg_pow's own
    5e-15: 2.4e-14."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for g in (1 / 3, 0.45, 1 / 2.2, 1.0, 1.1, 1.5, 1.8, 1.9, 2.0, 2.2, 2.4, 3.0):
        x = np.concatenate([np.exp2(rng.uniform(-40, 1, 80000)), [0.04045, 0.45, 1.0, 2.0, (0.04045 + 0.055) / 1.055]])
        worst = max(worst, float(np.abs(H.hlg_pow(x, g) / np.power(x, g) - 1.0).max()))
    print("hlg_pow against numpy.power: max relative error", worst)
    assert worst <= 2.4e-14
    # the rules around it: zero and negative bases, and the range rule
    assert L.icc_pow(np.array([0.0, -1.0, 1e-310]), 2.0).tolist() == [0.0, 0.0, 0.0]
    assert L.icc_pow(np.array([0.0]), 0.0).tolist() == [1.0] and np.isinf(L.icc_pow(np.array([0.0]), -1.0)[0])
    assert L.icc_pow(np.array([1e-30, 1e30]), 20.0).tolist() == [0.0, np.inf] and L.icc_pow(np.array([1e-30, 1e30]), -20.0).tolist() == [np.inf, 0.0]
    assert L.icc_pow(np.array([4.0]), 0.5).tolist() == [2.0]
