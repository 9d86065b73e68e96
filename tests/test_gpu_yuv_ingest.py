"""Planar Y'CbCr ingest on the device (ce_yuv_to_rgb*, ce_batch_set_*_yuv) against the numpy restatement
(tests/yuv_restatement.py, itself pinned to libjpeg-turbo in test_yuv_ingest_cpu.py) bit for bit: every subsampling,
filter, layout, depth and alignment; pitches, host and device planes; slots of RGB8 and deep batches; scores of a batch
filled from planes against one filled with the restatement's RGB; the Pillow fixture; every refusal; the session."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_restatement as Y  # noqa: E402

pytestmark = pytest.mark.gpu

S = importlib.import_module("codec-eval_amd.session")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the last three: under 8 pixels wide (the per-sample luma route) and a single row or a single chroma row
SHAPES = ((8, 8), (9, 9), (10, 8), (17, 9), (301, 9), (9, 301), (100, 76), (768, 512), (1, 1), (3, 5), (7, 2))
SUBS = (Y.SUB_444, Y.SUB_422, Y.SUB_420, Y.SUB_400)


def padded(plane, pad, rng):
    """the plane's bytes as rows of a wider buffer whose padding holds junk: a (rows, row bytes) uint8 view, pitch = + pad"""
    raw = np.ascontiguousarray(plane).view(np.uint8).reshape(plane.shape[0], -1)
    if pad == 0:
        return raw
    buf = rng.integers(0, 256, (raw.shape[0], raw.shape[1] + pad), dtype=np.uint8)
    buf[:, :raw.shape[1]] = raw
    return buf[:, :raw.shape[1]]


def image(ce, y, cb, cr, sub, layout=Y.PLANAR, pad=0, rng=None, **kw):
    """planar arrays -> a YuvImage of the asked layout (host planes)"""
    rng = rng or np.random.default_rng(0)
    if sub == Y.SUB_400:
        planes = [padded(y, pad, rng)]
    elif layout == Y.SEMIPLANAR:
        planes = [padded(y, pad, rng), padded(Y.interleave(cb, cr), pad, rng)]
    else:
        planes = [padded(y, pad, rng), padded(cb, pad, rng), padded(cr, pad, rng)]
    return ce.YuvImage(planes, subsampling=sub, layout=layout, **kw)


def on_device(ce, img):
    """the same planes in torch GPU tensors, passed by address; returns (YuvImage, the tensors to keep)"""
    import torch

    keep, ptrs, pitches = [], [], []
    for p in img.planes:  # (rows, row bytes) uint8 views; the pitch is the view's row stride
        pitch = p.strides[0] if p.shape[0] > 1 else p.shape[1]
        full = np.full((p.shape[0], pitch), 0xA5, np.uint8)
        full[:, :p.shape[1]] = p
        t = torch.from_numpy(full).cuda()
        keep.append(t)
        ptrs.append(t.data_ptr())
        pitches.append(pitch)
    torch.cuda.synchronize()
    dev = ce.YuvImage(ptrs, img.subsampling, img.layout, img.matrix, img.range, img.upsample, img.depth, img.msb_aligned,
                      ce.MEM_DEVICE, pitches)
    return dev, keep


def read_slab(ce, address, nbytes):
    """Device bytes -> host after everything queued on the device (the slot writes run on the batch's upload stream)."""
    assert ce.lib().hipDeviceSynchronize() == 0
    out = np.empty(nbytes, np.uint8)
    assert ce.lib().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(address), ctypes.c_size_t(nbytes), 2) == 0
    return out


def scores_tuple(s):
    return (s.status, s.valid, s.dssim, s.ssimulacra2, s.butteraugli, s.psnr)


@pytest.mark.parametrize("w,h", SHAPES)
def test_8bit_equals_the_restatement(gpu_ctx, ce, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    i = 0
    for sub in SUBS:
        y, cb, cr = Y.smooth_planes(rng, w, h, sub) if sub == Y.SUB_420 and (w, h) == (100, 76) else Y.random_planes(rng, w, h, sub)
        for mode in (Y.NEAREST, Y.TRIANGLE):
            for layout in (Y.PLANAR, Y.SEMIPLANAR):
                matrix, range_ = i % 3, (i // 3) % 2
                i += 1
                want = Y.yuv_to_rgb(y, cb, cr, w, h, sub, matrix, range_, mode)
                got = gpu_ctx.yuv_to_rgb8(image(ce, y, cb, cr, sub, layout, matrix=matrix, range=range_, upsample=mode), w, h)
                assert got.shape == (h, w, 3) and np.array_equal(got, want), (sub, mode, layout, matrix, range_)
                # 8-bit planes into 16-bit samples of another depth (what a deep batch of that depth stores)
                if mode == Y.TRIANGLE and layout == Y.PLANAR:
                    got16 = gpu_ctx.yuv_to_rgb16(image(ce, y, cb, cr, sub, layout, matrix=matrix, range=range_, upsample=mode), w, h, 16)
                    assert np.array_equal(got16, Y.yuv_to_rgb(y, cb, cr, w, h, sub, matrix, range_, mode, 8, 16))


@pytest.mark.parametrize("d", [10, 12])
def test_deep_samples_equal_the_restatement(gpu_ctx, ce, d):
    rng = np.random.default_rng(d)
    i = 0
    for msb in (False, True):
        for range_ in (Y.FULL, Y.LIMITED):
            for matrix in (Y.BT601, Y.BT709, Y.BT2020):
                for D in (8, d):
                    sub, mode, layout = SUBS[i % 4], (i // 2) % 2, (i // 4) % 2
                    w, h = ((17, 9), (100, 76), (9, 301))[i % 3]
                    i += 1
                    y, cb, cr = Y.random_planes(rng, w, h, sub, d, msb, over=True)
                    img = image(ce, y, cb, cr, sub, layout, matrix=matrix, range=range_, upsample=mode, depth=d, msb_aligned=msb)
                    want = Y.yuv_to_rgb(y, cb, cr, w, h, sub, matrix, range_, mode, d, D, msb)
                    got = gpu_ctx.yuv_to_rgb8(img, w, h) if D == 8 else gpu_ctx.yuv_to_rgb16(img, w, h, D)
                    assert np.array_equal(got, want), (d, msb, range_, matrix, D, sub, mode, layout, w, h)
    # low-aligned samples above 2^d - 1 are clamped to it
    y = np.full((8, 16), 0xffff, np.uint16)
    c = np.full((4, 8), 1 << (d - 1), np.uint16)
    got = gpu_ctx.yuv_to_rgb16(ce.YuvImage([y, c, c], depth=d), 16, 8, d)
    assert np.array_equal(got, np.full((8, 16, 3), (1 << d) - 1, np.uint16))
    # 768 x 512 P010-style: semiplanar, MSB-aligned, limited range
    y, cb, cr = Y.random_planes(rng, 768, 512, Y.SUB_420, d, True)
    img = image(ce, y, cb, cr, Y.SUB_420, Y.SEMIPLANAR, matrix=Y.BT2020, range=Y.LIMITED, depth=d, msb_aligned=True)
    assert np.array_equal(gpu_ctx.yuv_to_rgb16(img, 768, 512, d), Y.yuv_to_rgb(y, cb, cr, 768, 512, Y.SUB_420, Y.BT2020, Y.LIMITED, Y.TRIANGLE, d, d, True))


@pytest.mark.parametrize("w,h", [(17, 9), (100, 76)])
def test_layout_invariance(gpu_ctx, ce, w, h):
    rng = np.random.default_rng(7)
    for d, pads in ((8, (0, 1, 7, 64)), (10, (0, 2, 64))):
        for sub in SUBS:
            y, cb, cr = Y.random_planes(rng, w, h, sub, d)
            want = Y.yuv_to_rgb(y, cb, cr, w, h, sub, Y.BT709, Y.LIMITED, Y.TRIANGLE, d, d)
            for pad in pads:
                for layout in (Y.PLANAR, Y.SEMIPLANAR):
                    img = image(ce, y, cb, cr, sub, layout, pad, rng, matrix=Y.BT709, range=Y.LIMITED, depth=d)
                    conv = (lambda im: gpu_ctx.yuv_to_rgb8(im, w, h)) if d == 8 else (lambda im: gpu_ctx.yuv_to_rgb16(im, w, h, d))
                    assert np.array_equal(conv(img), want), (d, sub, pad, layout, "host")
                    dev, keep = on_device(ce, img)
                    assert np.array_equal(conv(dev), want), (d, sub, pad, layout, "device")
                    del keep


@pytest.mark.parametrize("w,h", [(9, 9), (100, 76)])
@pytest.mark.parametrize("deep", [False, True])
def test_slots_of_a_batch(gpu_ctx, ce, w, h, deep):
    """3 references, 5 pairs: slots 0, 1 and the last one are written from planes (9 x 9: slot 1 starts at an odd byte of an
    RGB8 slab; 100 x 76: every slot is 16-byte aligned), host and device planes; the other slots keep their bytes."""
    rng = np.random.default_rng(11)
    d = 10 if deep else 8
    n_refs, n_pairs = 3, 5
    batch = ce.Batch(gpu_ctx, w, h, n_refs, n_pairs, depths=(10, 10) if deep else None)
    try:
        dt, bps = (np.uint16, 2) if deep else (np.uint8, 1)
        fill_r = rng.integers(0, 1 << d, (n_refs, h, w, 3)).astype(dt)
        fill_t = rng.integers(0, 1 << d, (n_pairs, h, w, 3)).astype(dt)
        for i in range(n_refs):
            batch.set_reference(i, fill_r[i])
        for i in range(n_pairs):
            batch.set_test(i, i % n_refs, fill_t[i])
        want_r, want_t = fill_r.copy(), fill_t.copy()
        keep = []
        for n, slot in enumerate((0, 1, n_refs - 1)):
            sub = (Y.SUB_420, Y.SUB_422, Y.SUB_444)[n]
            y, cb, cr = Y.random_planes(rng, w, h, sub, d)
            img = image(ce, y, cb, cr, sub, n % 2, 7 * (1 - n % 2) * bps, rng, depth=d)
            if n == 2:
                img, k = on_device(ce, img)
                keep.append(k)
            batch.set_reference_yuv(slot, img)
            want_r[slot] = Y.yuv_to_rgb(y, cb, cr, w, h, sub, d=d, D=d)
            one = gpu_ctx.yuv_to_rgb16(img, w, h, d) if deep else gpu_ctx.yuv_to_rgb8(img, w, h)
            assert np.array_equal(one, want_r[slot])
        for n, slot in enumerate((0, 1, n_pairs - 1)):
            sub = (Y.SUB_400, Y.SUB_420, Y.SUB_420)[n]
            y, cb, cr = Y.random_planes(rng, w, h, sub, d)
            img = image(ce, y, cb, cr, sub, (n + 1) % 2, 0, rng, depth=d, upsample=n % 2)
            if n == 1:
                img, k = on_device(ce, img)
                keep.append(k)
            batch.set_test_yuv(slot, 2, img)
            assert batch.pair_reference(slot) == 2
            want_t[slot] = Y.yuv_to_rgb(y, cb, cr, w, h, sub, mode=n % 2, d=d, D=d)
        got_r = read_slab(ce, batch.reference_slab, want_r.nbytes).view(dt).reshape(want_r.shape)
        got_t = read_slab(ce, batch.test_slab, want_t.nbytes).view(dt).reshape(want_t.shape)
        for i in range(n_refs):
            assert np.array_equal(got_r[i], want_r[i]), ("reference slot", i)
        for i in range(n_pairs):
            assert np.array_equal(got_t[i], want_t[i]), ("test slot", i)
        if not deep:  # every other call on such a batch behaves as on any other: the heuristics read the converted slot
            a = batch.image_heuristics(0, 1)[0]
            b = gpu_ctx.image_heuristics(want_r[0], w, h)
            fields = [f for f in ce.HEURISTICS_FIELDS]
            assert np.array_equal([getattr(a, f) for f in fields], [getattr(b, f) for f in fields], equal_nan=True)
    finally:
        batch.close()


@pytest.mark.parametrize("w,h", [(100, 76), (768, 512)])
@pytest.mark.parametrize("deep", [False, True])
def test_scores_equal_those_of_the_restated_rgb(gpu_ctx, ce, w, h, deep):
    rng = np.random.default_rng(13)
    d = 10 if deep else 8
    m = (1 << d) - 1
    depths = (10, 10) if deep else None
    ref = Y.smooth_planes(rng, w, h, Y.SUB_420, d)
    tests = []
    for amp in (m / 60.0, m / 15.0):
        tests.append(tuple(np.clip(np.rint(p + rng.normal(0, amp, p.shape)), 0, m).astype(p.dtype) for p in ref))
    a, b = ce.Batch(gpu_ctx, w, h, 1, 2, depths=depths), ce.Batch(gpu_ctx, w, h, 1, 2, depths=depths)
    try:
        kw = dict(matrix=Y.BT709, range=Y.LIMITED, depth=d)
        a.set_reference_yuv(0, image(ce, *ref, Y.SUB_420, Y.PLANAR, **kw))
        b.set_reference(0, Y.yuv_to_rgb(*ref, w, h, Y.SUB_420, Y.BT709, Y.LIMITED, d=d, D=d))
        for i, t in enumerate(tests):
            a.set_test_yuv(i, 0, image(ce, *t, Y.SUB_420, Y.SEMIPLANAR, **kw))
            b.set_test(i, 0, Y.yuv_to_rgb(*t, w, h, Y.SUB_420, Y.BT709, Y.LIMITED, d=d, D=d))
        sa, sb = a.run(2, ce.MetricConfig.all()), b.run(2, ce.MetricConfig.all())
        for x, y in zip(sa, sb):
            assert x.status == 0 and x.valid == 15
            assert scores_tuple(x) == scores_tuple(y)
        assert sa[0].ssimulacra2 > sa[1].ssimulacra2  # the two tests differ, and the scores see it
    finally:
        a.close(), b.close()


def test_pillow_fixture_on_the_device(gpu_ctx, ce):
    """libjpeg-turbo's raw 4:2:0 planes through BT601 / FULL / TRIANGLE are Pillow's RGB; its upsampled planes as 4:4:4 too"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "yuv_pillow.npz"))
    for w, h in ((48, 32), (37, 21), (16, 16), (9, 301), (100, 76)):
        half, ycc = g[f"420_{w}x{h}_half"], g[f"420_{w}x{h}_ycc"]
        planes = [np.ascontiguousarray(ycc[..., 0]), np.ascontiguousarray(half[..., 1]), np.ascontiguousarray(half[..., 2])]
        assert np.array_equal(gpu_ctx.yuv_to_rgb8(ce.YuvImage(planes), w, h), g[f"420_{w}x{h}_rgb"])
        for sub in ("444", "422"):
            ycc = g[f"{sub}_{w}x{h}_ycc"]
            planes = [np.ascontiguousarray(ycc[..., c]) for c in range(3)]
            assert np.array_equal(gpu_ctx.yuv_to_rgb8(ce.YuvImage(planes, subsampling=ce.YUV_444), w, h), g[f"{sub}_{w}x{h}_rgb"])


def test_refusals_leave_the_batch_usable(gpu_ctx, ce):
    w, h = 16, 10
    rng = np.random.default_rng(17)
    y, cb, cr = Y.random_planes(rng, w, h, Y.SUB_420)
    y16, cb16, cr16 = Y.random_planes(rng, w, h, Y.SUB_420, 10)
    good = ce.YuvImage([y, cb, cr])
    want = Y.yuv_to_rgb(y, cb, cr, w, h, Y.SUB_420)
    table = ce.ColorTable(gpu_ctx, ce.ColorTable.identity_cube())
    odd = np.zeros(h * 2 * w + 1, np.uint8)[1:].reshape(h, 2 * w)  # a u16 plane at an odd address

    def c_struct(img, **fields):
        c, keep = img._c()
        for k, v in fields.items():
            setattr(c, k, v)
        return c, keep

    bad = {
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
        "odd u16 pitch": c_struct(ce.YuvImage([y16, cb16, cr16], depth=10, pitches=[2 * w + 1, w, w])),
        "odd u16 pointer": c_struct(ce.YuvImage([odd, cb16, cr16], depth=10)),
        "msb_aligned at depth 8": c_struct(good, msb_aligned=1),
        "colour table": c_struct(good, lut=ctypes.cast(table._h, ctypes.c_void_p).value),
    }
    batch = ce.Batch(gpu_ctx, w, h, 1, 1)
    L = ce.lib()
    try:
        for what, (c, _keep) in bad.items():
            for call in (lambda: L.ce_batch_set_reference_yuv(batch._h, 0, ctypes.byref(c)),
                         lambda: L.ce_batch_set_test_yuv(batch._h, 0, 0, ctypes.byref(c)),
                         lambda: L.ce_yuv_to_rgb8(gpu_ctx._h, ctypes.byref(c), w, h, np.empty(w * h * 3, np.uint8).ctypes.data, w * h * 3)):
                assert call() == ce.CE_ERR_INVALID_ARG, what
                assert gpu_ctx._err(), what
            batch.set_reference_yuv(0, good)
            batch.set_test_yuv(0, 0, good)
            s = batch.run(1, ce.MetricConfig.all())[0]
            assert s.status == 0 and s.valid == 15, what
            assert np.array_equal(read_slab(ce, batch.test_slab, w * h * 3).reshape(h, w, 3), want), what
        assert L.ce_batch_set_reference_yuv(batch._h, 0, None) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err()
        assert L.ce_batch_set_reference_yuv(batch._h, 1, ctypes.byref(good._c()[0])) == ce.CE_ERR_INVALID_ARG
        with pytest.raises(ce.CodecEvalError):
            gpu_ctx.yuv_to_rgb16(good, w, h, 9)
        out = np.empty(5, np.uint8)
        assert L.ce_yuv_to_rgb8(gpu_ctx._h, ctypes.byref(good._c()[0]), w, h, out.ctypes.data, out.size) == ce.CE_ERR_BAD_LENGTH
        assert np.array_equal(gpu_ctx.yuv_to_rgb8(good, w, h), want)
    finally:
        batch.close()
        table.close()


def test_session_takes_yuv_decodes(gpu_ctx, ce, tmp_path):
    w, h = 100, 76
    rng = np.random.default_rng(19)
    src_planes = Y.smooth_planes(rng, w, h, Y.SUB_444)
    src = Y.yuv_to_rgb(*src_planes, w, h, Y.SUB_444)
    decodes = {}
    for q in (40, 80):
        y, cb, cr = Y.smooth_planes(np.random.default_rng(19), w, h, Y.SUB_420)
        y = np.clip(y.astype(np.int64) + rng.integers(-(100 - q) // 8, (100 - q) // 8 + 1, y.shape), 0, 255).astype(np.uint8)
        decodes[q] = (y, cb, cr)

    def decode_yuv(blob):
        y, cb, cr = decodes[int(blob)]
        return S.ImageData.yuv([y, Y.interleave(cb, cr)], w, h, ce.YUV_420, ce.YUV_SEMIPLANAR)

    def decode_rgb(blob):
        y, cb, cr = decodes[int(blob)]
        return S.ImageData.rgb(Y.yuv_to_rgb(y, cb, cr, w, h, Y.SUB_420), w, h)

    def run(as_yuv, source=None):
        cfg = S.EvalConfig.builder().report_dir(tmp_path / ("yuv" if as_yuv else "rgb")).metrics(ce.MetricConfig.all()).quality_levels([40, 80]).build()
        ses = S.EvalSession(cfg, ctx=gpu_ctx)
        ses.add_codec_with_decode("planes", "1", lambda im, rq: b"%d" % int(rq.quality), decode_yuv if as_yuv else decode_rgb)
        rep = ses.evaluate_image("x", source or S.ImageData.rgb(src, w, h))
        return [(r.quality, r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in rep.results]

    a, b = run(True), run(False)
    assert len(a) == 2 and a == b and all(v is not None for row in a for v in row)
    y, cb, cr = decodes[40]
    assert np.array_equal(S.ImageData.yuv([y, cb, cr], w, h).to_rgb8_vec().reshape(h, w, 3), Y.yuv_to_rgb(y, cb, cr, w, h, Y.SUB_420))
    # a source image still in its planes (a JPEG source decoded in raw mode): the same scores as its RGB
    c = run(True, S.ImageData.yuv(list(src_planes), w, h, ce.YUV_444))
    assert c == a
    # the multi-device session sweeps without a device of its own and converts on the host: the same rows
    md = importlib.import_module("codec-eval_amd.multidevice")
    cfg = S.EvalConfig.builder().report_dir(tmp_path / "multi").metrics(ce.MetricConfig.all()).quality_levels([40, 80]).build()
    multi = md.MultiDeviceEvalSession(cfg)
    try:
        multi.add_codec_with_decode("planes", "1", lambda im, rq: b"%d" % int(rq.quality), decode_yuv)
        for source in (S.ImageData.rgb(src, w, h), S.ImageData.yuv(list(src_planes), w, h, ce.YUV_444)):
            corpus, _stats = multi.evaluate_corpus("c", [("x", source)])
            assert [(r.quality, r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in corpus.images[0].results] == a
    finally:
        multi.close()
