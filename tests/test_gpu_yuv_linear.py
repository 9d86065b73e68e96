"""Y'CbCr planes with a CICP description into a linear batch, in one kernel (include/ce_metrics.h: ce_batch_set_*_yuv_cicp,
ce_yuv_to_linear).  The definition is the composition of two pinned ones, so the device must equal the
composed numpy restatement (tests/yuv_linear_cases.py) on every float, bit for bit; the scores of what it wrote must equal
those of the same integer RGB taken in by the existing routes."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_linear_cases as L  # noqa: E402
import yuv_restatement as Y  # noqa: E402
from test_gpu_deep_input import run_everything, same  # noqa: E402
from test_gpu_linear_input import golden, only  # noqa: E402
from test_gpu_yuv_ingest import image, read_slab, scores_tuple  # noqa: E402

pytestmark = pytest.mark.gpu

S = importlib.import_module("codec-eval_amd.session")
CASES = L.cases()


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


class HipBuffer:
    """device memory from the HIP runtime the library itself is linked against, freed with the object"""
    def __init__(self, lib, nbytes):
        self.lib, self.ptr = lib, C.c_void_p()
        assert lib.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0

    def __del__(self):
        self.lib.hipFree(self.ptr)


def device_planes(ce, img, keep):
    """The planes of `img` in device memory, passed by address (CE_MEM_DEVICE), junk in the pitch padding.  Allocated with
    hipMalloc through the library's own runtime handle (ce.lib()) rather than with torch: both give the 256-byte alignment a
    decoder's surfaces have (asserted here), and this way the test opens no second HIP runtime in the process.  `keep`
    receives what must outlive the batch's next collect."""
    lib = ce.lib()
    ptrs, pitches = [], []
    for p in img.planes:  # (rows, row bytes) uint8 views; the pitch is the view's row stride
        pitch = p.strides[0] if p.shape[0] > 1 else p.shape[1]
        full = np.full((p.shape[0], pitch), 0xA5, np.uint8)
        full[:, :p.shape[1]] = p
        buf = HipBuffer(lib, full.nbytes)
        assert buf.ptr.value % 256 == 0
        assert lib.hipMemcpy(buf.ptr, C.c_void_p(full.ctypes.data), C.c_size_t(full.nbytes), 1) == 0
        keep.append(buf)
        ptrs.append(buf.ptr.value)
        pitches.append(pitch)
    return ce.YuvImage(ptrs, img.subsampling, img.layout, img.matrix, img.range, img.upsample, img.depth, img.msb_aligned, ce.MEM_DEVICE, pitches)


def case_image(ce, case, planes, rng, keep):
    (d, msb) = case["sample"]
    img = image(ce, *planes, case["sub"], case["layout"], case["pad"] * (1 if d == 8 else 2), rng, matrix=case["matrix"], range=case["range"],
                upsample=case["mode"], depth=d, msb_aligned=msb)
    return device_planes(ce, img, keep) if case["device"] else img


@pytest.mark.parametrize("w,h", L.SHAPES)
def test_ingest_equals_the_restatement_bit_for_bit(ce, gpu_ctx, w, h):
    """Six cases per shape: slots 0, 1 and 2 of the reference slab and of the test slab, the other slots checked untouched;
    ce_yuv_to_linear returns the slot's floats."""
    rng = np.random.default_rng(w * 1000 + h)
    n = w * h * 3
    b = gpu_ctx.batch_linear(w, h, 3, 3)
    keep = []
    try:
        slabs = [[rng.random((h, w, 3), np.float32) for _ in range(3)] for _ in range(2)]
        for i in range(3):
            b.set_reference(i, slabs[0][i])
            b.set_test(i, i, slabs[1][i])
        mine = [c for c in CASES if c["shape"] == (w, h)]
        assert sorted((c["slab"], c["slot"]) for c in mine) == [(s, k) for s in (0, 1) for k in (0, 1, 2)]
        for c in mine:
            planes = L.planes_of(c)
            want = L.want_of(c, planes)
            img = case_image(ce, c, planes, rng, keep)
            colour = ce.ColourDescription(c["prim"], c["tr"], L.c_depth(c), L.WHITE)
            if c["slab"] == 0:
                b.set_reference_yuv_cicp(c["slot"], img, colour)
            else:
                b.set_test_yuv_cicp(c["slot"], (c["slot"] + 1) % 3, img, colour)
                assert b.pair_reference(c["slot"]) == (c["slot"] + 1) % 3
            slabs[c["slab"]][c["slot"]] = want
            got = gpu_ctx.yuv_to_linear(img, w, h, colour)
            assert got.shape == (h, w, 3) and np.array_equal(bits(got), bits(want)), c
            for which, address in ((0, b.reference_slab), (1, b.test_slab)):
                slab = read_slab(ce, address, 3 * n * 4).view(np.uint32)
                assert np.array_equal(slab, np.concatenate([bits(x) for x in slabs[which]])), (c, which)
    finally:
        b.close()  # waits for the device: the planes in `keep` are free to go
        keep.clear()


def forward_planes(rgb, matrix, range_, d, sub, msb=False):
    """Planes of depth d from 8-bit RGB by the matrix's own forward transform in f64 (chroma: the mean of each cell)."""
    a, _, _, e = Y.matrix_constants(matrix)
    kr, kb = 1.0 - a / 2.0, 1.0 - e / 2.0
    v = rgb.astype(np.float64) / 255.0
    y = kr * v[..., 0] + (1.0 - kr - kb) * v[..., 1] + kb * v[..., 2]
    cb, cr = (v[..., 2] - y) / e, (v[..., 0] - y) / a
    u = float(1 << (d - 8))
    if range_ == Y.FULL:
        m = float((1 << d) - 1)
        yq, cbq, crq = y * m, cb * m + (1 << (d - 1)), cr * m + (1 << (d - 1))
    else:
        yq, cbq, crq = 16 * u + 219 * u * y, 128 * u + 224 * u * cb, 128 * u + 224 * u * cr
    h, w = y.shape
    if sub == Y.SUB_420:
        def cells(c):
            c = np.pad(c, ((0, h % 2), (0, w % 2)), mode="edge")
            return c.reshape(c.shape[0] // 2, 2, c.shape[1] // 2, 2).mean(axis=(1, 3))
        cbq, crq = cells(cbq), cells(crq)
    dt = np.uint8 if d == 8 else np.uint16
    q = lambda p: (np.clip(np.rint(p), 0, (1 << d) - 1).astype(dt) << ((16 - d) if msb else 0)).astype(dt)
    return q(yq), q(cbq), q(crq)


@pytest.mark.parametrize("name", ["min8x8_q50", "nat97x131_q75_420", "odd257x129_q30_420"])
def test_exact_score_anchor_srgb_planes_score_as_the_rgb8_batch(ce, gpu_ctx, name):
    """8-bit planes through *_yuv into an RGB8 batch, and through *_yuv_cicp with (1, 13, depth 8) into a linear batch: the
    slots hold ce_srgb_table(8, 0) of the same bytes, so SSIMULACRA2, Butteraugli and their maps are ==.  DSSIM's RGB8
    front end reads the other table rule (f32 powf, rule 1), so, as tests/test_gpu_linear_input.py does for the CICP (1, 13)
    upload, DSSIM is not compared with the RGB8 batch; it is == - score and SSIM maps, like everything else - a linear batch
    loaded through *_cicp with the restated RGB8, which reads the same table as the fused kernel.  (Measured on an MI355X:
    the two rules put DSSIM 8e-4 relative apart on min8x8_q50.)"""
    ref, test = golden(name)
    h, w = ref.shape[:2]
    planes = [forward_planes(x, Y.BT601, Y.FULL, 8, Y.SUB_420) for x in (ref, test)]
    imgs = [image(ce, *p, Y.SUB_420, Y.PLANAR if i == 0 else Y.SEMIPLANAR) for i, p in enumerate(planes)]
    rgb = [Y.yuv_to_rgb(*p, w, h, Y.SUB_420) for p in planes]
    colour = ce.ColourDescription(1, 13, 8)
    plain, lin, chain = ce.Batch(gpu_ctx, w, h, 1, 1), gpu_ctx.batch_linear(w, h, 1, 1), gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        plain.set_reference_yuv(0, imgs[0])
        plain.set_test_yuv(0, 0, imgs[1])
        lin.set_reference_yuv_cicp(0, imgs[0], colour)
        lin.set_test_yuv_cicp(0, 0, imgs[1], colour)
        chain.set_reference_cicp(0, rgb[0], colour)
        chain.set_test_cicp(0, 0, rgb[1], colour)
        a, b, c = (run_everything(ce, x, 1, w, h) for x in (plain, lin, chain))
        assert b["scores"][0][5] == 0 and (b["scores"][0][4] & 7) == 7
        same(only(b, "s2ba"), only(a, "s2ba"))
        same(b, c)
        print(f"anchor {name}: DSSIM RGB8 batch (table rule 1) {a['scores'][0][0]!r} linear batch (rule 0) {b['scores'][0][0]!r}")
    finally:
        for x in (plain, lin, chain):
            x.close()


def test_hdr_chain_p010_scores_equal_the_restated_rgb16_through_cicp(ce, gpu_ctx):
    """P010 4:2:0 BT.2020 limited-range planes of a golden pair, read as (9, 16, depth 16, white 203): every score == that
    of the restatement's RGB16 uploaded through *_cicp."""
    ref, test = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    kw = dict(matrix=Y.BT2020, range=Y.LIMITED, depth=10, msb_aligned=True)
    planes = [forward_planes(x, Y.BT2020, Y.LIMITED, 10, Y.SUB_420, msb=True) for x in (ref, test)]
    colour = ce.ColourDescription(9, 16, 16, 203.0)
    rgb16 = [Y.yuv_to_rgb(*p, w, h, Y.SUB_420, Y.BT2020, Y.LIMITED, Y.TRIANGLE, 10, 16, True) for p in planes]
    fused, chain = gpu_ctx.batch_linear(w, h, 1, 1), gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        fused.set_reference_yuv_cicp(0, image(ce, *planes[0], Y.SUB_420, Y.SEMIPLANAR, **kw), colour)
        fused.set_test_yuv_cicp(0, 0, image(ce, *planes[1], Y.SUB_420, Y.SEMIPLANAR, **kw), colour)
        chain.set_reference_cicp(0, rgb16[0], colour)
        chain.set_test_cicp(0, 0, rgb16[1], colour)
        a, b = run_everything(ce, fused, 1, w, h), run_everything(ce, chain, 1, w, h)
        assert a["scores"][0][5] == 0 and (a["scores"][0][4] & 7) == 7 and a["scores"][0][1] < 100.0
        same(a, b)
    finally:
        fused.close(), chain.close()


def test_session_scores_tagged_planes_through_the_fused_ingest(ce, gpu_ctx, tmp_path):
    ref, test = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    kw = dict(matrix=Y.BT2020, range=Y.LIMITED, depth=10, msb_aligned=True)
    src_p, dec_p = (forward_planes(x, Y.BT2020, Y.LIMITED, 10, Y.SUB_420, msb=True) for x in (ref, test))
    semi = lambda p: [p[0], Y.interleave(p[1], p[2])]
    pq = ce.ColourDescription.BT2020_PQ
    tagged = lambda p: S.ImageData.yuv(semi(p), w, h, ce.YUV_420, ce.YUV_SEMIPLANAR, ce.YUV_BT2020, ce.YUV_LIMITED, depth=10, msb_aligned=True, colour=pq)
    assert tagged(src_p).in_linear_light
    with pytest.raises(ce.MetricCalculation, match="no RGB8 form"):
        tagged(src_p).to_rgb8_vec()
    cfg = S.EvalConfig.builder().report_dir(str(tmp_path)).metrics(ce.MetricConfig.all()).quality_levels([50.0]).build()
    enc = lambda img, req: b"x"
    sess = S.EvalSession(cfg, ctx=gpu_ctx)
    sess.add_codec_with_decode("hdr", "1", enc, lambda data: tagged(dec_p))
    row = sess.evaluate_image("img", tagged(src_p)).results[0]
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        b.set_reference_yuv_cicp(0, image(ce, *src_p, Y.SUB_420, Y.SEMIPLANAR, **kw), pq.with_depth(16))
        b.set_test_yuv_cicp(0, 0, image(ce, *dec_p, Y.SUB_420, Y.SEMIPLANAR, **kw), pq.with_depth(16))
        m = ce.MetricResult.from_c(b.run(1, ce.MetricConfig.all())[0])
    finally:
        b.close()
    assert (row.dssim, row.ssimulacra2, row.butteraugli, row.psnr) == (m.dssim, m.ssimulacra2, m.butteraugli, None)
    assert m.ssimulacra2 is not None and m.ssimulacra2 < 100.0
    # untagged 8-bit planes score as they always did: the RGB8 route, PSNR included
    p8 = forward_planes(test, Y.BT601, Y.FULL, 8, Y.SUB_420)
    plain = S.EvalSession(cfg, ctx=gpu_ctx)
    plain.add_codec_with_decode("sdr", "1", enc, lambda data: S.ImageData.yuv(list(p8), w, h))
    old = plain.evaluate_image("img", S.ImageData.rgb(ref, w, h)).results[0]
    today = gpu_ctx.calculate_metrics(ref, Y.yuv_to_rgb(*p8, w, h, Y.SUB_420), w, h, ce.MetricConfig.all())
    assert (old.dssim, old.ssimulacra2, old.butteraugli, old.psnr) == (today.dssim, today.ssimulacra2, today.butteraugli, today.psnr)
    # untagged planes against a linear-light source enter the linear batch as (1, 13) at depth 16
    mixed = S.EvalSession(cfg, ctx=gpu_ctx)
    mixed.add_codec_with_decode("sdr", "1", enc, lambda data: S.ImageData.yuv(list(p8), w, h))
    got = mixed.evaluate_image("img", tagged(src_p)).results[0]
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        b.set_reference_yuv_cicp(0, image(ce, *src_p, Y.SUB_420, Y.SEMIPLANAR, **kw), pq.with_depth(16))
        b.set_test_yuv_cicp(0, 0, image(ce, *p8, Y.SUB_420), ce.ColourDescription(1, 13, 16))
        m = ce.MetricResult.from_c(b.run(1, ce.MetricConfig.all())[0])
    finally:
        b.close()
    assert (got.dssim, got.ssimulacra2, got.butteraugli, got.psnr) == (m.dssim, m.ssimulacra2, m.butteraugli, None)


@pytest.mark.parametrize("device", [False, True])
def test_set_between_launch_and_collect_is_ordered(ce, gpu_ctx, device):
    """A fused ingest into slots that a launch in flight still reads waits for that launch on the device, from host planes
    (behind the staging copy) and from CE_MEM_DEVICE planes (read in place) alike: the collect returns the first images'
    scores, the launch that follows sees the second images.  (tests/test_gpu_alpha.py's case of the same name.)"""
    ref, test = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    cfg = ce.MetricConfig.all()
    kw = dict(matrix=Y.BT2020, range=Y.LIMITED, depth=10, msb_aligned=True)
    colour = ce.ColourDescription(9, 16, 16, 203.0)
    first = [forward_planes(x, Y.BT2020, Y.LIMITED, 10, Y.SUB_420, msb=True) for x in (ref, test)]
    second = [forward_planes(x, Y.BT2020, Y.LIMITED, 10, Y.SUB_420, msb=True) for x in (np.ascontiguousarray(test[::-1]), np.ascontiguousarray(ref[::-1, ::-1]))]
    keep = []

    def fill(b, planes, dev):
        imgs = [image(ce, *p, Y.SUB_420, Y.SEMIPLANAR, **kw) for p in planes]
        if dev:
            imgs = [device_planes(ce, im, keep) for im in imgs]
        b.set_reference_yuv_cicp(0, imgs[0], colour)
        b.set_test_yuv_cicp(0, 0, imgs[1], colour)

    def alone(planes):
        b = gpu_ctx.batch_linear(w, h, 1, 1)
        try:
            fill(b, planes, False)
            return [scores_tuple(s) for s in b.run(1, cfg)]
        finally:
            b.close()

    want_first, want_second = alone(first), alone(second)
    assert want_first != want_second and want_first[0][0] == 0 and want_second[0][0] == 0
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        fill(b, first, device)
        b.launch(1, cfg)
        fill(b, second, device)  # while the launch is in flight
        assert [scores_tuple(s) for s in b.collect(1)] == want_first
        assert [scores_tuple(s) for s in b.run(1, cfg)] == want_second
        got = read_slab(ce, b.test_slab, w * h * 12).view(np.uint32)
        assert np.array_equal(got, bits(L.composed(*second[1], w, h, Y.SUB_420, Y.BT2020, Y.LIMITED, Y.TRIANGLE, 10, True, 9, 16, 16)))
    finally:
        b.close()
        keep.clear()


def test_refusals_leave_the_batch_usable(ce, gpu_ctx):
    w, h = 16, 10
    rng = np.random.default_rng(23)
    y, cb, cr = Y.random_planes(rng, w, h, Y.SUB_420)
    y10, cb10, cr10 = Y.random_planes(rng, w, h, Y.SUB_420, 10)
    good, good10 = ce.YuvImage([y, cb, cr]), ce.YuvImage([y10, cb10, cr10], depth=10)
    srgb8 = ce.CeColour(1, 13, 8, 0.0)
    want = L.composed(y, cb, cr, w, h, Y.SUB_420, Y.BT601, Y.FULL, Y.TRIANGLE, 8, False, 1, 13, 8)
    table = ce.ColorTable(gpu_ctx, ce.ColorTable.identity_cube())
    odd = np.zeros(h * 2 * w + 1, np.uint8)[1:].reshape(h, 2 * w)  # a u16 plane at an odd address
    lib = ce.lib()

    def c_struct(img, **fields):
        c, keep = img._c()
        for k, v in fields.items():
            setattr(c, k, v)
        return c, keep

    bad_images = {  # everything *_yuv refuses
        "missing plane": c_struct(ce.YuvImage([y, cb, None])),
        "missing CbCr plane": c_struct(ce.YuvImage([y, None, None], layout=ce.YUV_SEMIPLANAR)),
        "unknown subsampling": c_struct(good, subsampling=4),
        "unknown layout": c_struct(good, layout=2),
        "unknown matrix": c_struct(good, matrix=3),
        "unknown range": c_struct(good, range=2),
        "unknown upsampling": c_struct(good, upsample=2),
        "unknown memory": c_struct(good, memory=2),
        "depth 16": c_struct(good, depth=16),
        "depth 9": c_struct(good, depth=9),
        "pitch under the row": c_struct(ce.YuvImage([y, cb, cr], pitches=[w - 1, w // 2, w // 2])),
        "chroma pitch under the row": c_struct(ce.YuvImage([y, cb, cr], pitches=[w, w // 2 - 1, w // 2])),
        "odd u16 pitch": c_struct(ce.YuvImage([y10, cb10, cr10], depth=10, pitches=[2 * w + 1, w, w])),
        "odd u16 pointer": c_struct(ce.YuvImage([odd, cb10, cr10], depth=10)),
        "msb_aligned at depth 8": c_struct(good, msb_aligned=1),
        "colour table": c_struct(good, lut=C.cast(table._h, C.c_void_p).value),
    }
    bad_colours = {  # everything *_cicp refuses about c
        "primaries 2": ce.CeColour(2, 13, 8, 0.0), "transfer 18": ce.CeColour(1, 18, 10, 203.0), "transfer 1": ce.CeColour(1, 1, 10, 0.0),
        "depth 9": ce.CeColour(1, 13, 9, 0.0), "depth 0": ce.CeColour(1, 13, 0, 0.0), "PQ without a white": ce.CeColour(9, 16, 10, 0.0),
        "PQ with a negative white": ce.CeColour(9, 16, 10, -5.0), "PQ with a NaN white": ce.CeColour(9, 16, 10, float("nan")),
    }
    out = np.empty(w * h * 3, np.float32)
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    plain, deep = ce.Batch(gpu_ctx, w, h, 1, 1), gpu_ctx.batch_deep(w, h, 1, 1, 16, 16)
    try:
        b.set_reference_yuv_cicp(0, good, ce.ColourDescription(1, 13, 8))
        b.set_test_yuv_cicp(0, 0, ce.YuvImage([y, cr, cb]), ce.ColourDescription(1, 13, 8))
        first = b.run(1, ce.MetricConfig.all())[0]
        assert first.status == 0 and first.valid == 7

        def refused(what, img_c, col_c):
            calls = (lambda: lib.ce_batch_set_reference_yuv_cicp(b._h, 0, img_c, col_c),
                     lambda: lib.ce_batch_set_test_yuv_cicp(b._h, 0, 0, img_c, col_c),
                     lambda: lib.ce_yuv_to_linear(gpu_ctx._h, img_c, col_c, w, h, out.ctypes.data, out.size))
            for call in calls:
                assert call() == ce.CE_ERR_INVALID_ARG, what
                assert gpu_ctx._err(), what

        for what, (c, _keep) in bad_images.items():
            refused(what, C.byref(c), C.byref(srgb8))
        for what, col in bad_colours.items():
            refused(what, C.byref(good._c()[0]), C.byref(col))
        c10, _keep10 = good10._c()
        refused("c.depth under the samples'", C.byref(c10), C.byref(srgb8))
        refused("null image", None, C.byref(srgb8))
        refused("null colour", C.byref(good._c()[0]), None)
        for other in (plain, deep):  # a batch that is not linear
            assert lib.ce_batch_set_reference_yuv_cicp(other._h, 0, C.byref(good._c()[0]), C.byref(srgb8)) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err()
            assert lib.ce_batch_set_test_yuv_cicp(other._h, 0, 0, C.byref(good._c()[0]), C.byref(srgb8)) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err()
        # slot indices past the batch
        assert lib.ce_batch_set_reference_yuv_cicp(b._h, 1, C.byref(good._c()[0]), C.byref(srgb8)) == ce.CE_ERR_INVALID_ARG
        assert lib.ce_batch_set_test_yuv_cicp(b._h, 1, 0, C.byref(good._c()[0]), C.byref(srgb8)) == ce.CE_ERR_INVALID_ARG
        # *_yuv on a linear batch stays refused, and now names the calls that serve it
        assert lib.ce_batch_set_reference_yuv(b._h, 0, C.byref(good._c()[0])) == ce.CE_ERR_INVALID_ARG and "yuv_cicp" in gpu_ctx._err()
        assert lib.ce_batch_set_test_yuv(b._h, 0, 0, C.byref(good._c()[0])) == ce.CE_ERR_INVALID_ARG and "yuv_cicp" in gpu_ctx._err()
        assert lib.ce_yuv_to_linear(gpu_ctx._h, C.byref(good._c()[0]), C.byref(srgb8), w, h, out.ctypes.data, out.size - 3) == ce.CE_ERR_BAD_LENGTH
        # after all of that: the slots are what they were, the batch scores what it scored, and the calls work
        again = b.run(1, ce.MetricConfig.all())[0]
        assert (again.status, again.valid, again.dssim, again.ssimulacra2, again.butteraugli) == \
               (first.status, first.valid, first.dssim, first.ssimulacra2, first.butteraugli)
        assert np.array_equal(read_slab(ce, b.reference_slab, w * h * 12).view(np.uint32), bits(want))
        assert np.array_equal(bits(gpu_ctx.yuv_to_linear(good, w, h, ce.ColourDescription(1, 13, 8))), bits(want))
    finally:
        for x in (b, plain, deep):
            x.close()
        table.close()
