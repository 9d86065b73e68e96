"""One batch filled through every ingest route in turn.  The per-route files fill a batch through one route at a time; what
the routes share - the ordering rule of slot writes and the two wide staging pairs (ce_ingest.cpp) - shows only when a route
meets a pair that another route sized or left busy.  The expected content of a slot is what the route's own leaf conversion
returns for the same input, uploaded through the plain route into a second batch; the two slabs must agree in every bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_lut_restatement as LR  # noqa: E402
import icc_restatement as R  # noqa: E402
import yuv_restatement as Y  # noqa: E402
from test_gpu_yuv_ingest import image, read_slab  # noqa: E402
from test_gpu_yuv_linear import device_planes  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 23, 9  # w * h is no multiple of 4: the slots of a slab are not 16-byte aligned


def planes(rng, sub, depth):
    """random Y, Cb, Cr of a W x H image at `depth` bits"""
    dt = np.uint8 if depth == 8 else np.uint16
    cw, ch = Y.chroma_size(W, H, sub)
    draw = lambda rows, cols: rng.integers(0, 1 << depth, (rows, cols)).astype(dt)
    return draw(H, W), draw(ch, cw), draw(ch, cw)


def test_rgb8_batch_through_every_route(ce, gpu_ctx):
    """Test slots 0 .. 9: plain RGB8, _fmt RGBA8, _yuv host 4:2:0, _yuv device, _over with two backgrounds (two slots), _lut
    with the identity table, _fmt RGBA8 again, _icc RGBA8 with a Display P3 profile, _yuv_icc host 4:2:2 with a LUT profile.
    The wide staging pairs go 0 (_fmt), 1 (_yuv), 0 (_over), 1 (_lut), 0 (_fmt), 1 (_icc), 0 (_yuv_icc): each is taken while
    still busy, by another route than the one that used it last."""
    rng = np.random.default_rng(2309)
    rgb = lambda: rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgba = lambda: rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    keep = []
    ref, plain, fmt_a, over, lut_in, fmt_b, icc_in = rgb(), rgb(), rgba(), rgba(), rgba(), rgba(), rgba()
    yuv_host = image(ce, *planes(rng, Y.SUB_420, 8), Y.SUB_420, Y.PLANAR, 3, rng)
    yuv_dev = device_planes(ce, image(ce, *planes(rng, Y.SUB_420, 8), Y.SUB_420, Y.SEMIPLANAR, 1, rng), keep)
    bgs = [(255, 255, 255), (12, 200, 77)]
    yuv_prof = image(ce, *planes(rng, Y.SUB_422, 8), Y.SUB_422, Y.PLANAR, 3, rng)
    table = ce.ColorTable(gpu_ctx, ce.ColorTable.identity_cube())
    p3 = ce.IccProfile(gpu_ctx, R.fixtures()["p3"])
    mft2 = ce.IccLutProfile(gpu_ctx, LR.fixtures()["mft2_lab"], 0, LR.TRILINEAR)
    mixed, direct = ce.Batch(gpu_ctx, W, H, 1, 10), ce.Batch(gpu_ctx, W, H, 1, 10)
    try:
        want = [plain, fmt_a[..., :3], gpu_ctx.yuv_to_rgb8(yuv_host, W, H), gpu_ctx.yuv_to_rgb8(yuv_dev, W, H)]
        want += [gpu_ctx.composite_rgba8(over, W, H, bg) for bg in bgs]
        want += [lut_in[..., :3], fmt_b[..., :3], gpu_ctx.icc_to_srgb(icc_in, W, H, 8, p3), gpu_ctx.yuv_icc_to_srgb(yuv_prof, W, H, 8, mft2)]
        mixed.set_reference(0, ref)
        mixed.set_test(0, 0, plain)
        mixed.set_test_fmt(1, 0, fmt_a, ce.PIXEL_RGBA8)
        mixed.set_test_yuv(2, 0, yuv_host)
        mixed.set_test_yuv(3, 0, yuv_dev)
        mixed.set_test_over(4, [0, 0], over, ce.PIXEL_RGBA8, bgs)
        mixed.set_test_lut(6, 0, lut_in, ce.PIXEL_RGBA8, table)
        mixed.set_test_fmt(7, 0, fmt_b, ce.PIXEL_RGBA8)
        mixed.set_test_icc(8, 0, icc_in, 8, p3)
        mixed.set_test_yuv_icc(9, 0, yuv_prof, 8, mft2)
        direct.set_reference(0, ref)
        for i, img in enumerate(want):
            direct.set_test(i, 0, np.ascontiguousarray(img))
        n = W * H * 3
        got, exp = read_slab(ce, mixed.test_slab, 10 * n), read_slab(ce, direct.test_slab, 10 * n)
        for i in range(10):
            assert np.array_equal(got[i * n:(i + 1) * n], exp[i * n:(i + 1) * n]), f"test slot {i}"
        assert np.array_equal(read_slab(ce, mixed.reference_slab, n), read_slab(ce, direct.reference_slab, n))
    finally:
        mixed.close()  # waits for the device: the planes in `keep` are free to go
        direct.close()
        table.close()
        p3.close(), mft2.close()
        keep.clear()


def test_linear_batch_through_every_route_twice(ce, gpu_ctx):
    """Two rounds of twelve test slots.  A round is _fmt RGB_F32, _cicp RGB16 PQ / BT.2020, _hlg RGBA16, _yuv_cicp host 10-bit
    4:2:2, _yuv_cicp device, _yuv_hlg host semiplanar, _gainmap RGB8 with a three-channel map (the side pair), _icc RGBA16 with
    a Display P3 profile, _yuv_icc host 4:2:0 with a LUT profile, _cicp_over RGBA8 over two backgrounds (two slots),
    _linear_over RGBA_F32 (16 bytes per pixel).  Every route but the device planes takes a wide staging pair: ten a round, so
    the second round runs in the reverse order - each pair is then reused by every route, always by another one than used it
    last, while the previous one's conversion may still run."""
    rng = np.random.default_rng(923)
    pq = ce.ColourDescription(ce.PRIMARIES_BT2020, ce.TRANSFER_PQ, 10, 203.0)
    p3_srgb = ce.ColourDescription(ce.PRIMARIES_P3_D65, ce.TRANSFER_SRGB, 8)
    hlg = ce.HlgDescription()  # BT.2020 primaries, 10 bits, 1000 nits
    p3 = ce.IccProfile(gpu_ctx, R.fixtures()["p3"])
    mab = ce.IccLutProfile(gpu_ctx, LR.fixtures()["mab_xyz"], 0, LR.TETRAHEDRAL)
    bgs = [(0.0, 0.0, 0.0), (1.0, 0.25, 4.0)]
    keep, rounds = [], []
    for _ in range(2):
        f32 = rng.random((H, W, 3), np.float32)
        rgb16 = rng.integers(0, 1024, (H, W, 3)).astype(np.uint16)
        rgba16 = rng.integers(0, 1024, (H, W, 4)).astype(np.uint16)
        y422 = image(ce, *planes(rng, Y.SUB_422, 10), Y.SUB_422, Y.PLANAR, 2, rng, depth=10)
        y422_dev = device_planes(ce, image(ce, *planes(rng, Y.SUB_422, 10), Y.SUB_422, Y.PLANAR, 4, rng, depth=10), keep)
        y420_semi = image(ce, *planes(rng, Y.SUB_420, 10), Y.SUB_420, Y.SEMIPLANAR, 2, rng, depth=10)
        base = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        gm = ce.GainMap(rng.integers(0, 256, (4, 11, 3), dtype=np.uint8), gain_max=(2.0, 1.5, 1.0))
        icc16 = rng.integers(0, 1024, (H, W, 4)).astype(np.uint16)
        y420 = image(ce, *planes(rng, Y.SUB_420, 8), Y.SUB_420, Y.PLANAR, 5, rng)
        over8 = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        over_f32 = rng.random((H, W, 4), np.float32)
        # (the route's fill of slots i .., what its leaf says those slots hold)
        rounds.append([
            (lambda b, i, a=f32: b.set_test_fmt(i, 0, a, ce.PIXEL_RGB_F32), [f32]),
            (lambda b, i, a=rgb16: b.set_test_cicp(i, 0, a, pq), [gpu_ctx.cicp_to_linear(rgb16, W, H, pq)]),
            (lambda b, i, a=rgba16: b.set_test_hlg(i, 0, a, hlg), [gpu_ctx.hlg_to_linear(rgba16, W, H, hlg)]),
            (lambda b, i, a=y422: b.set_test_yuv_cicp(i, 0, a, pq), [gpu_ctx.yuv_to_linear(y422, W, H, pq)]),
            (lambda b, i, a=y422_dev: b.set_test_yuv_cicp(i, 0, a, pq), [gpu_ctx.yuv_to_linear(y422_dev, W, H, pq)]),
            (lambda b, i, a=y420_semi: b.set_test_yuv_hlg(i, 0, a, hlg), [gpu_ctx.yuv_hlg_to_linear(y420_semi, W, H, hlg)]),
            (lambda b, i, a=base, g=gm: b.set_test_gainmap(i, 0, a, p3_srgb, g), [gpu_ctx.gainmap_to_linear(base, W, H, p3_srgb, gm)]),
            (lambda b, i, a=icc16: b.set_test_icc(i, 0, a, 10, p3), [gpu_ctx.icc_to_linear(icc16, W, H, 10, p3)]),
            (lambda b, i, a=y420: b.set_test_yuv_icc(i, 0, a, 8, mab), [gpu_ctx.yuv_icc_to_linear(y420, W, H, 8, mab)]),
            (lambda b, i, a=over8: b.set_test_cicp_over(i, [0, 0], a, p3_srgb, bgs), [gpu_ctx.cicp_over_to_linear(over8, W, H, p3_srgb, bg) for bg in bgs]),
            (lambda b, i, a=over_f32: b.set_test_linear_over(i, [0], a, bgs[1:]), [gpu_ctx.linear_over(over_f32, W, H, bgs[1])]),
        ])
    order = rounds[0] + rounds[1][::-1]
    want = [img for _, imgs in order for img in imgs]
    assert len(want) == 24
    ref = rng.random((H, W, 3), np.float32)
    mixed, direct = gpu_ctx.batch_linear(W, H, 1, 24), gpu_ctx.batch_linear(W, H, 1, 24)
    try:
        mixed.set_reference(0, ref)
        i = 0
        for fill, imgs in order:
            fill(mixed, i)
            i += len(imgs)
        direct.set_reference(0, ref)
        for i, img in enumerate(want):
            direct.set_test_fmt(i, 0, np.ascontiguousarray(img, np.float32), ce.PIXEL_RGB_F32)
        n = W * H * 12
        got, exp = read_slab(ce, mixed.test_slab, 24 * n), read_slab(ce, direct.test_slab, 24 * n)
        for i in range(24):
            assert np.array_equal(got[i * n:(i + 1) * n], exp[i * n:(i + 1) * n]), f"test slot {i}"
        assert np.array_equal(read_slab(ce, mixed.reference_slab, n), read_slab(ce, direct.reference_slab, n))
    finally:
        mixed.close()  # waits for the device: the planes in `keep` are free to go
        direct.close()
        p3.close(), mab.close()
        keep.clear()


def test_multi_slot_setters_refuse_the_first_fault(ce, gpu_ctx):
    """ce_batch_set_*_over and ce_batch_set_*_cicp_over with two faults at once: the code and the text are those of the fault
    that the call meets first - the arguments, then the slot range, then the reference indices; the batch kind before a null
    pointer in the linear-light call and behind it in the integer one.  Nothing is launched."""
    import ctypes as C

    w = h = 4
    lib = ce.lib()
    px = np.zeros((h, w, 4), np.uint8)
    rgb = np.zeros((h, w, 3), np.uint8)
    c8 = ce.CeColour(1, 13, 8, 0.0)
    bg16, bg16_bad = np.zeros((2, 3), np.uint16), np.array([[0, 0, 0], [0, 256, 0]], np.uint16)
    bgf, bgf_bad = np.zeros((2, 3), np.float32), np.array([[0, 0, 0], [0, np.inf, 0]], np.float32)
    refs, refs_bad = np.zeros(2, np.uint32), np.array([0, 2], np.uint32)
    plain, linear = ce.Batch(gpu_ctx, w, h, 2, 2), gpu_ctx.batch_linear(w, h, 2, 2)

    def over(b, first=0, r=refs, pixels=px, fmt=ce.PIXEL_RGBA8, bg=bg16):
        """the reference call and the test call with the same arguments, not yet made"""
        p = pixels.ctypes.data if pixels is not None else None
        n = px.nbytes if pixels is None else pixels.nbytes
        return (lambda: lib.ce_batch_set_reference_over(b._h, first, p, n, fmt, 2, bg.ctypes.data),
                lambda: lib.ce_batch_set_test_over(b._h, first, r.ctypes.data, p, n, fmt, 2, bg.ctypes.data))

    def cicp_over(b, first=0, r=refs, pixels=px, fmt=ce.PIXEL_RGBA8, bg=bgf):
        p = pixels.ctypes.data if pixels is not None else None
        n = px.nbytes if pixels is None else pixels.nbytes
        return (lambda: lib.ce_batch_set_reference_cicp_over(b._h, first, p, n, fmt, C.byref(c8), 2, bg.ctypes.data),
                lambda: lib.ce_batch_set_test_cicp_over(b._h, first, r.ctypes.data, p, n, fmt, C.byref(c8), 2, bg.ctypes.data))

    def refused(call, text, **kw):
        for which, make in enumerate(call(**kw)):
            assert lib.ce_batch_set_test_fmt(plain._h, 9, 0, px.ctypes.data, px.nbytes, ce.PIXEL_RGBA8) != ce.CE_OK  # another text in between
            assert gpu_ctx._err() != text
            assert make() == ce.CE_ERR_INVALID_ARG, (text, which)
            assert gpu_ctx._err() == text.replace("{side}", ("reference", "test")[which]), (text, which)

    try:
        # a bad format and a slot range past the batch
        refused(over, "alpha compositing: the format must be CE_PIXEL_RGBA8 or CE_PIXEL_RGBA16", b=plain, first=1, pixels=rgb, fmt=ce.PIXEL_RGB8)
        refused(cicp_over, "linear-light compositing: the format must be CE_PIXEL_RGBA8 or CE_PIXEL_RGBA16", b=linear, first=1, pixels=rgb, fmt=ce.PIXEL_RGB8)
        # a bad background and a slot range past the batch
        refused(over, "alpha compositing: background sample 256 is above 255", b=plain, first=1, bg=bg16_bad)
        refused(cicp_over, "linear-light compositing: a background must be finite and within +-1024", b=linear, first=1, bg=bgf_bad)
        # a slot range past the batch and a reference index out of range
        refused(over, "alpha compositing: {side} slots [1, 3) outside the 2 slots", b=plain, first=1, r=refs_bad)
        refused(cicp_over, "linear-light compositing: {side} slots [1, 3) outside the 2 slots", b=linear, first=1, r=refs_bad)
        # the wrong kind of batch and a null pointer
        refused(over, "alpha compositing: null pointer", b=linear, pixels=None)
        refused(cicp_over, "linear-light compositing writes linear light: it needs a linear batch (ce_batch_create_linear)", b=plain, pixels=None)
        # each fault alone is refused too, so that the pairs above did hold two
        refused(over, "alpha compositing: {side} slots [1, 3) outside the 2 slots", b=plain, first=1)
        refused(cicp_over, "linear-light compositing: {side} slots [1, 3) outside the 2 slots", b=linear, first=1)
        assert lib.ce_batch_set_test_over(plain._h, 0, refs_bad.ctypes.data, px.ctypes.data, px.nbytes, ce.PIXEL_RGBA8, 2, bg16.ctypes.data) == ce.CE_ERR_INVALID_ARG
        assert gpu_ctx._err() == "alpha compositing: ref index 2 out of range"
        assert lib.ce_batch_set_test_cicp_over(linear._h, 0, refs_bad.ctypes.data, px.ctypes.data, px.nbytes, ce.PIXEL_RGBA8, C.byref(c8), 2,
                                               bgf.ctypes.data) == ce.CE_ERR_INVALID_ARG
        assert gpu_ctx._err() == "linear-light compositing: ref index 2 out of range"
        refused(over, "alpha compositing works on encoded integer samples: not for a linear batch", b=linear)
    finally:
        plain.close(), linear.close()
