"""The names the ingest launches report to the profiler (Context.prof_stats).  profiles/*.py and the tables of DESIGN.md
sections 13 - 18 are keyed on them, and each one also says which kernel the launcher's ladder picked: sample size,
subsampling, output and primaries matrix.  One 17 x 9 image goes down every route - 17 x 9 is the smallest shape that takes
the cropped group, the odd height's last row and a one-pixel tail at once - and after each image exactly one launch must
have been added, under the name written out below."""
import numpy as np
import pytest

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


def test_every_ingest_route_reports_one_launch_under_its_name(ce):
    ctx = ce.Context(0)  # its own context: the profiler's counters are the context's
    rng = np.random.default_rng(179)
    linear, rgb8, deep = ctx.batch_linear(W, H, 1, 1), ce.Batch(ctx, W, H, 1, 1), ctx.batch_deep(W, H, 1, 1, 16, 16)
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
    finally:
        ctx.prof_enable(False)
        for b in (linear, rgb8, deep):
            b.close()
        ctx.close()
