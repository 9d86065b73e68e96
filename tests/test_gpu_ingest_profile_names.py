"""The names the ingest launches report to the profiler (Context.prof_stats).  profiles/*.py and the tables of DESIGN.md
sections 13 - 25 are keyed on them, and each one also says which kernel the launcher's ladder picked: format or sample size
and subsampling, the slot's kind, the pixel (a colour description, an ICC profile of either flavour, a gain map), blended over a
background or not, with a matrix or without.  The names are written out or composed here from their grammar, never read from
the library.  One 17 x 9 image goes down every route - 17 x 9 is the smallest shape that takes
the cropped group, the odd height's last row and a one-pixel tail at once - and after each image exactly one launch must
have been added, under the name written out below."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_lut_restatement as LR  # noqa: E402
import icc_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 17, 9

# (format's dtype, channels) -> the names without and with a primaries matrix, by route
PACKED = (
    (np.uint8, 3, ("cicp_rgb8", "cicp_rgb8_m"), ("hlg_rgb8", "hlg_rgb8_m")),
    (np.uint8, 4, ("cicp_rgba8", "cicp_rgba8_m"), ("hlg_rgba8", "hlg_rgba8_m")),
    (np.uint16, 3, ("cicp_rgb16", "cicp_rgb16_m"), ("hlg_rgb16", "hlg_rgb16_m")),
    (np.uint16, 4, ("cicp_rgba16", "cicp_rgba16_m"), ("hlg_rgba16", "hlg_rgba16_m")),
)

# (subsampling, semiplanar, bits of a sample as stored) -> integer RGB into an RGB8 batch and into a deep one, linear light
# through a CICP description without and with a matrix, the same through an HLG description
PLANES = (
    ("444", False, 8, "yuv444_8", "yuv444_8_deep", "yuv444_8_lin", "yuv444_8_lin_m", "yuv444_8_hlg", "yuv444_8_hlg_m"),
    ("444", True, 8, "yuv444_8", "yuv444_8_deep", "yuv444_8_lin", "yuv444_8_lin_m", "yuv444_8_hlg", "yuv444_8_hlg_m"),
    ("422", False, 8, "yuv422_8", "yuv422_8_deep", "yuv422_8_lin", "yuv422_8_lin_m", "yuv422_8_hlg", "yuv422_8_hlg_m"),
    ("422", True, 8, "yuv422_8", "yuv422_8_deep", "yuv422_8_lin", "yuv422_8_lin_m", "yuv422_8_hlg", "yuv422_8_hlg_m"),
    ("420", False, 8, "yuv420_8", "yuv420_8_deep", "yuv420_8_lin", "yuv420_8_lin_m", "yuv420_8_hlg", "yuv420_8_hlg_m"),
    ("420", True, 8, "yuv420_8", "yuv420_8_deep", "yuv420_8_lin", "yuv420_8_lin_m", "yuv420_8_hlg", "yuv420_8_hlg_m"),
    ("400", False, 8, "yuv400_8", "yuv400_8_deep", "yuv400_8_lin", "yuv400_8_lin_m", "yuv400_8_hlg", "yuv400_8_hlg_m"),
    ("444", False, 16, "yuv444_16", "yuv444_16_deep", "yuv444_16_lin", "yuv444_16_lin_m", "yuv444_16_hlg", "yuv444_16_hlg_m"),
    ("444", True, 16, "yuv444_16", "yuv444_16_deep", "yuv444_16_lin", "yuv444_16_lin_m", "yuv444_16_hlg", "yuv444_16_hlg_m"),
    ("422", False, 16, "yuv422_16", "yuv422_16_deep", "yuv422_16_lin", "yuv422_16_lin_m", "yuv422_16_hlg", "yuv422_16_hlg_m"),
    ("422", True, 16, "yuv422_16", "yuv422_16_deep", "yuv422_16_lin", "yuv422_16_lin_m", "yuv422_16_hlg", "yuv422_16_hlg_m"),
    ("420", False, 16, "yuv420_16", "yuv420_16_deep", "yuv420_16_lin", "yuv420_16_lin_m", "yuv420_16_hlg", "yuv420_16_hlg_m"),
    ("420", True, 16, "yuv420_16", "yuv420_16_deep", "yuv420_16_lin", "yuv420_16_lin_m", "yuv420_16_hlg", "yuv420_16_hlg_m"),
    ("400", False, 16, "yuv400_16", "yuv400_16_deep", "yuv400_16_lin", "yuv400_16_lin_m", "yuv400_16_hlg", "yuv400_16_hlg_m"),
)


def yuv_image(ce, rng, sub, semi, bits):
    """random planes of a W x H image: u8 samples, or 10-bit ones in u16"""
    subsampling = {"444": ce.YUV_444, "422": ce.YUV_422, "420": ce.YUV_420, "400": ce.YUV_400}[sub]
    cw = W if sub == "444" else (W + 1) // 2
    ch = (H + 1) // 2 if sub == "420" else H
    dt, depth = (np.uint8, 8) if bits == 8 else (np.uint16, 10)
    plane = lambda rows, cols: rng.integers(0, 1 << depth, (rows, cols)).astype(dt)  # noqa: E731
    planes = [plane(H, W)]
    if sub != "400":
        planes += [plane(ch, 2 * cw)] if semi else [plane(ch, cw), plane(ch, cw)]
    return ce.YuvImage(planes, subsampling=subsampling, layout=ce.YUV_SEMIPLANAR if semi else ce.YUV_PLANAR, depth=depth), depth


FMT = {(np.uint8, 3): "rgb8", (np.uint8, 4): "rgba8", (np.uint16, 3): "rgb16", (np.uint16, 4): "rgba16"}
SLOTS = ("lin", "u8", "u16")  # a linear batch, an RGB8 batch, a deep batch
GREY = [(0.25, 0.5, 0.125)]


def test_every_ingest_route_reports_one_launch_under_its_name(ce):
    ctx = ce.Context(0)  # its own context: the profiler's counters are the context's
    rng = np.random.default_rng(179)
    linear, rgb8, deep = ctx.batch_linear(W, H, 1, 1), ce.Batch(ctx, W, H, 1, 1), ctx.batch_deep(W, H, 1, 1, 16, 16)
    # matrix/TRC profiles without and with a matrix, one LUT profile under both interpolations: (handle, name stem, name suffix)
    matrix_trc = [(ce.IccProfile(ctx, R.fixtures()[name]), "icc", suffix) for name, suffix in (("srgb_para", ""), ("p3", "_m"))]
    lut = [(ce.IccLutProfile(ctx, LR.fixtures()["mab_xyz"], 0, interpolation), stem, "")
           for interpolation, stem in ((LR.TRILINEAR, "icc_lut_tri"), (LR.TETRAHEDRAL, "icc_lut_tet"))]
    seen = []
    try:
        ctx.prof_enable(True)

        def launched(name, upload):
            """`upload` adds one launch, under `name`, and nothing else"""
            assert ce.lib().hipDeviceSynchronize() == 0
            before = ctx.prof_stats()
            upload()
            assert ce.lib().hipDeviceSynchronize() == 0  # the slot writes run on the batch's upload stream
            after = ctx.prof_stats()
            gained = {k: n - before.get(k, (0, 0.0))[0] for k, (n, _) in after.items() if n != before.get(k, (0, 0.0))[0]}
            assert gained == {name: 1}, (name, gained)
            seen.append(name)

        for dt, channels, cicp_names, hlg_names in PACKED:
            depth = 8 if dt == np.uint8 else 10
            px = rng.integers(0, 1 << depth, (H, W, channels)).astype(dt)
            for m, prim in enumerate((ce.PRIMARIES_BT709, ce.PRIMARIES_BT2020)):
                launched(cicp_names[m], lambda: linear.set_test_cicp(0, 0, px, ce.ColourDescription(prim, ce.TRANSFER_SRGB, depth)))
                launched(hlg_names[m], lambda: linear.set_test_hlg(0, 0, px, ce.HlgDescription(prim, depth)))

        launched("ingest_linear_f32", lambda: linear.set_test_fmt(0, 0, rng.random((H, W, 3), np.float32), ce.PIXEL_RGB_F32))

        for sub, semi, bits, name, name_deep, lin, lin_m, hlg, hlg_m in PLANES:
            img, depth = yuv_image(ce, rng, sub, semi, bits)
            launched(name, lambda: rgb8.set_test_yuv(0, 0, img))
            launched(name_deep, lambda: deep.set_test_yuv(0, 0, img))
            for m, prim in enumerate((ce.PRIMARIES_BT709, ce.PRIMARIES_BT2020)):
                launched((lin, lin_m)[m], lambda: linear.set_test_yuv_cicp(0, 0, img, ce.ColourDescription(prim, ce.TRANSFER_SRGB, depth)))
                launched((hlg, hlg_m)[m], lambda: linear.set_test_yuv_hlg(0, 0, img, ce.HlgDescription(prim, depth)))
        assert len(seen) == 16 + 1 + 14 * 6

        # ICC profiles of both flavours into the three kinds of slot: icc_{lin|u8|u16}_{fmt}[_m], icc_lut_{tri|tet}_{lin|u8|u16}_{fmt}
        packed = {}
        for (dt, channels), fmt in FMT.items():
            depth = 8 if dt == np.uint8 else 10
            packed[fmt] = (rng.integers(0, 1 << depth, (H, W, channels)).astype(dt), depth)
        for prof, stem, suffix in matrix_trc + lut:
            for slot, batch in zip(SLOTS, (linear, rgb8, deep)):
                for fmt, (px, depth) in packed.items():
                    if slot == "u8" and depth != 8:
                        continue  # an RGB8 batch takes 8-bit sources only
                    launched(f"{stem}_{slot}_{fmt}{suffix}", lambda: batch.set_test_icc(0, 0, px, depth, prof))
        assert len(seen) == 101 + 4 * (4 + 2 + 4)

        # gain maps: gainmap_{fmt}_{1|3}[_m]
        for fmt, (px, depth) in packed.items():
            for channels in (1, 3):
                gm = ce.GainMap(rng.integers(0, 256, (5, 7, channels), dtype=np.uint8))
                for suffix, prim in (("", ce.PRIMARIES_BT709), ("_m", ce.PRIMARIES_BT2020)):
                    launched(f"gainmap_{fmt}_{channels}{suffix}",
                             lambda: linear.set_test_gainmap(0, 0, px, ce.ColourDescription(prim, ce.TRANSFER_SRGB, depth), gm))
        assert len(seen) == 141 + 16

        # blended over a background in linear light: {cicp|hlg}_over_{fmt}[_m], icc_over_{fmt}[_m], icc_lut_{tri|tet}_over_{fmt}
        for fmt in ("rgba8", "rgba16"):
            px, depth = packed[fmt]
            for suffix, prim in (("", ce.PRIMARIES_BT709), ("_m", ce.PRIMARIES_BT2020)):
                launched(f"cicp_over_{fmt}{suffix}", lambda: linear.set_test_cicp_over(0, [0], px, ce.ColourDescription(prim, ce.TRANSFER_SRGB, depth), GREY))
                launched(f"hlg_over_{fmt}{suffix}", lambda: linear.set_test_hlg_over(0, [0], px, ce.HlgDescription(prim, depth), GREY))
            for prof, stem, suffix in matrix_trc + lut:
                launched(f"{stem}_over_{fmt}{suffix}", lambda: linear.set_test_icc_over(0, [0], px, depth, prof, GREY))
        rgba_f32 = rng.random((H, W, 4), np.float32)
        launched("linear_over", lambda: linear.set_test_linear_over(0, [0], rgba_f32, GREY))
        launched("linear_over_premul", lambda: linear.set_test_linear_over(0, [0], rgba_f32, GREY, premultiplied=True))
        assert len(seen) == 157 + 2 * (4 + 4) + 2

        # planes through a profile: yuv{sub}_{bits}_icc_{lin|u8|u16}{"" | _m | _tri | _tet}
        pixels = [(prof, suffix) for prof, _, suffix in matrix_trc] + [(lut[0][0], "_tri"), (lut[1][0], "_tet")]
        for sub, semi, bits, name, *_ in PLANES:
            img, depth = yuv_image(ce, rng, sub, semi, bits)
            for slot, batch in zip(SLOTS, (linear, rgb8, deep)):
                for prof, pixel in pixels:
                    launched(f"{name}_icc_{slot}{pixel}", lambda: batch.set_test_yuv_icc(0, 0, img, depth, prof))
        assert len(seen) == 175 + 14 * 3 * 4
    finally:
        ctx.prof_enable(False)
        for prof, _, _ in matrix_trc + lut:
            prof.close()
        for b in (linear, rgb8, deep):
            b.close()
        ctx.close()
