"""Y'CbCr planes with an ICC profile into any batch, in one kernel (include/ce_metrics.h: ce_batch_set_*_yuv_icc,
ce_yuv_icc_to_*).  The definition is the composition of two pinned ones, so the device must equal the
composed numpy restatement (tests/yuv_icc_cases.py) on every byte; what it wrote must score exactly as the same planes taken
in by the routes it replaces."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_restatement as R  # noqa: E402
import yuv_icc_cases as K  # noqa: E402
import yuv_restatement as Y  # noqa: E402
from test_gpu_deep_input import run_everything, same  # noqa: E402
from test_gpu_linear_input import golden  # noqa: E402
from test_gpu_yuv_ingest import image, read_slab, scores_tuple  # noqa: E402
from test_gpu_yuv_linear import case_image, device_planes, forward_planes  # noqa: E402

pytestmark = pytest.mark.gpu

S = importlib.import_module("codec-eval_amd.session")
CASES = K.cases()
SAMPLE = {"lin": (np.float32, 4), "u8": (np.uint8, 1), "u16": (np.uint16, 2)}


@pytest.fixture(scope="module")
def profiles(ce, gpu_ctx):
    """one handle per profile of the case list, for the module"""
    made = {}
    for name, (flavour, _, interpolation) in K.PROFILES.items():
        p = K.profile_bytes(name)
        made[name] = ce.IccProfile(gpu_ctx, p) if flavour == "matrix" else ce.IccLutProfile(gpu_ctx, p, 0, interpolation)
    yield made
    for h in made.values():
        h.close()


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def batch_for(ce, ctx, w, h, dest, n_refs=3, n_pairs=3):
    kind, depth = dest
    if kind == "lin":
        return ctx.batch_linear(w, h, n_refs, n_pairs)
    return ce.Batch(ctx, w, h, n_refs, n_pairs) if kind == "u8" else ctx.batch_deep(w, h, n_refs, n_pairs, depth, depth)


def leaf(ctx, img, w, h, D, profile, dest):
    return ctx.yuv_icc_to_linear(img, w, h, D, profile) if dest[0] == "lin" else ctx.yuv_icc_to_srgb(img, w, h, D, profile, dest[1])


@pytest.mark.parametrize("w,h", K.SHAPES)
def test_ingest_equals_the_restatement_byte_for_byte(ce, gpu_ctx, profiles, w, h):
    """Six cases per shape: slots 0, 1 and 2 of the reference slab and of the test slab of a batch of the case's kind, host
    and device planes, the other slots checked untouched; the leaf call returns the slot's samples."""
    rng = np.random.default_rng(w * 1000 + h)
    mine = [c for c in CASES if c["shape"] == (w, h)]
    assert sorted((c["slab"], c["slot"]) for c in mine) == [(s, k) for s in (0, 1) for k in (0, 1, 2)]
    batches, keep = {}, []
    try:
        for c in mine:
            dest = c["dest"]
            dt, size = SAMPLE[dest[0]]
            if dest not in batches:  # a batch of this kind, every slot holding known samples
                b = batch_for(ce, gpu_ctx, w, h, dest)
                fill = (lambda: rng.random((h, w, 3), np.float32)) if dest[0] == "lin" else (lambda: rng.integers(0, 1 << dest[1], (h, w, 3)).astype(dt))
                slabs = [[fill() for _ in range(3)] for _ in range(2)]
                for i in range(3):
                    b.set_reference(i, slabs[0][i])
                    b.set_test(i, i, slabs[1][i])
                batches[dest] = (b, slabs)
            b, slabs = batches[dest]
            planes = K.planes_of(c)
            want = K.want_of(c, planes)
            assert want.dtype == dt
            img = case_image(ce, c, planes, rng, keep)
            D, prof = K.rgb_depth(c), profiles[c["profile"]]
            if c["slab"] == 0:
                b.set_reference_yuv_icc(c["slot"], img, D, prof)
            else:
                b.set_test_yuv_icc(c["slot"], (c["slot"] + 1) % 3, img, D, prof)
                assert b.pair_reference(c["slot"]) == (c["slot"] + 1) % 3
            slabs[c["slab"]][c["slot"]] = want
            got = leaf(gpu_ctx, img, w, h, D, prof, dest)
            assert got.shape == (h, w, 3) and got.dtype == dt and np.array_equal(raw(got), raw(want)), c
            for which, address in ((0, b.reference_slab), (1, b.test_slab)):
                slab = read_slab(ce, address, 3 * w * h * 3 * size)
                assert np.array_equal(slab, np.concatenate([raw(x) for x in slabs[which]])), (c, which)
    finally:
        for b, _ in batches.values():
            b.close()  # waits for the device: the planes in `keep` are free to go
        keep.clear()


def test_srgb_anchor_srgb_profile_planes_are_the_yuv_ingest(ce, gpu_ctx, profiles):
    """8-bit planes with an sRGB profile at rgb_depth 8 into an RGB8 batch: the sRGB curve decoded and encoded at 8 bits is the
    identity on codes, so the slabs hold the bytes of ce_batch_set_*_yuv and every score and map is ==."""
    ref, test = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    planes = [forward_planes(x, Y.BT601, Y.FULL, 8, Y.SUB_420) for x in (ref, test)]
    imgs = [image(ce, *p, Y.SUB_420, Y.PLANAR if i == 0 else Y.SEMIPLANAR) for i, p in enumerate(planes)]
    plain, fused = ce.Batch(gpu_ctx, w, h, 1, 1), ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        plain.set_reference_yuv(0, imgs[0])
        plain.set_test_yuv(0, 0, imgs[1])
        fused.set_reference_yuv_icc(0, imgs[0], 8, profiles["srgb_para"])
        fused.set_test_yuv_icc(0, 0, imgs[1], 8, profiles["srgb_para"])
        for a, b in ((plain.reference_slab, fused.reference_slab), (plain.test_slab, fused.test_slab)):
            assert np.array_equal(read_slab(ce, a, w * h * 3), read_slab(ce, b, w * h * 3))
        x, y = run_everything(ce, plain, 1, w, h), run_everything(ce, fused, 1, w, h)
        assert x["scores"][0][5] == 0 and (x["scores"][0][4] & 15) == 15
        same(x, y)
    finally:
        plain.close(), fused.close()


def pair_100x76(d, msb):
    """a smooth pair of 4:2:0 planes at 100 x 76, the test a little off the reference"""
    rng = np.random.default_rng(100 * 76 + d)
    w, h = 100, 76
    y, cb, cr = Y.smooth_planes(rng, w, h, Y.SUB_420, d)
    m = (1 << d) - 1
    off = lambda p, amp: np.clip(p.astype(np.int64) + np.rint(rng.normal(0, amp * m / 255.0, p.shape)).astype(np.int64), 0, m).astype(p.dtype)
    pair = [(y, cb, cr), (off(y, 6), off(cb, 4), off(cr, 4))]
    if msb:
        pair = [tuple((p << (16 - d)).astype(p.dtype) for p in ps) for ps in pair]
    return w, h, pair


@pytest.mark.parametrize("dest,profile,d,msb,D", [(("lin", 0), "mab_xyz_tet", 10, True, 16), (("lin", 0), "p3", 8, False, 8),
                                                  (("u16", 10), "p3", 10, True, 10), (("u16", 12), "mft2_lab_tri", 8, False, 16)])
def test_route_anchor_fused_equals_the_three_crossings(ce, gpu_ctx, profiles, dest, profile, d, msb, D):
    """The route the fused call replaces: ce_yuv_to_rgb16 (planes up, RGB down), then ce_batch_set_*_icc of that RGB as
    CE_PIXEL_RGB16 (RGB up again).  Slabs, every score and every map - Butteraugli's diffmap among them - are ==."""
    w, h, pair = pair_100x76(d, msb)
    kw = dict(matrix=Y.BT709, range=Y.LIMITED, depth=d, msb_aligned=msb)
    imgs = [image(ce, *p, Y.SUB_420, Y.SEMIPLANAR, **kw) for p in pair]
    prof = profiles[profile]
    fused, chain = batch_for(ce, gpu_ctx, w, h, dest, 1, 1), batch_for(ce, gpu_ctx, w, h, dest, 1, 1)
    try:
        fused.set_reference_yuv_icc(0, imgs[0], D, prof)
        fused.set_test_yuv_icc(0, 0, imgs[1], D, prof)
        rgb = [gpu_ctx.yuv_to_rgb16(im, w, h, D) for im in imgs]
        assert np.array_equal(rgb[0], Y.yuv_to_rgb(*pair[0], w, h, Y.SUB_420, Y.BT709, Y.LIMITED, Y.TRIANGLE, d, D, msb))
        chain.set_reference_icc(0, rgb[0], D, prof)
        chain.set_test_icc(0, 0, rgb[1], D, prof)
        n = w * h * 3 * SAMPLE[dest[0]][1]
        assert np.array_equal(read_slab(ce, fused.test_slab, n), read_slab(ce, chain.test_slab, n))
        a, b = run_everything(ce, fused, 1, w, h), run_everything(ce, chain, 1, w, h)
        assert a["scores"][0][5] == 0 and (a["scores"][0][4] & 7) == 7 and a["scores"][0][1] < 100.0 and "diffmap" in a
        same(a, b)
    finally:
        fused.close(), chain.close()


def saturated_pair(w=96, h=64):
    """saturated colour bars with a soft ramp, and the same a little damaged: code values meant as Display P3"""
    yy, xx = np.mgrid[0:h, 0:w]
    bars = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255]], np.float64)[(xx * 6) // w]
    ref = np.clip(bars * (0.55 + 0.45 * yy[..., None] / (h - 1)), 0, 255).astype(np.uint8)
    rng = np.random.default_rng(9)
    test = np.clip(ref.astype(np.int64) + rng.integers(-12, 13, ref.shape), 0, 255).astype(np.uint8)
    return ref, test


def test_p3_pair_scores_differ_with_and_without_the_profile(ce, gpu_ctx, profiles):
    """The fault the feature removes: Display P3 planes through ce_batch_set_*_yuv are read as sRGB.  On a saturated image the
    slabs and the scores with the profile differ from those without."""
    ref, test = saturated_pair()
    h, w = ref.shape[:2]
    imgs = [image(ce, *forward_planes(x, Y.BT601, Y.FULL, 8, Y.SUB_444), Y.SUB_444) for x in (ref, test)]
    plain, tagged = ce.Batch(gpu_ctx, w, h, 1, 1), ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        plain.set_reference_yuv(0, imgs[0])
        plain.set_test_yuv(0, 0, imgs[1])
        tagged.set_reference_yuv_icc(0, imgs[0], 8, profiles["p3"])
        tagged.set_test_yuv_icc(0, 0, imgs[1], 8, profiles["p3"])
        a, b = (scores_tuple(x.run(1, ce.MetricConfig.all())[0]) for x in (plain, tagged))
        assert a[0] == 0 and b[0] == 0 and a[1] == b[1] == 15
        assert not np.array_equal(read_slab(ce, plain.test_slab, w * h * 3), read_slab(ce, tagged.test_slab, w * h * 3))
        assert all(a[k] != b[k] for k in (2, 3, 4, 5)), (a, b)
    finally:
        plain.close(), tagged.close()


def test_session_scores_planes_with_a_profile_through_the_fused_ingest(ce, gpu_ctx, profiles, tmp_path):
    ref, test = saturated_pair()
    h, w = ref.shape[:2]
    p3 = K.profile_bytes("p3")
    dec_p = forward_planes(test, Y.BT601, Y.FULL, 8, Y.SUB_420)
    cfg = S.EvalConfig.builder().report_dir(str(tmp_path)).metrics(ce.MetricConfig.all()).quality_levels([50.0]).build()
    enc = lambda img, req: b"x"
    decoded = lambda **kw: S.ImageData.yuv(list(dec_p), w, h, **kw)
    key = lambda m: (m.dssim, m.ssimulacra2, m.butteraugli, m.psnr)

    def one(source, dec, **session_kw):
        sess = S.EvalSession(cfg, ctx=gpu_ctx, **session_kw)
        sess.add_codec_with_decode("c", "1", enc, lambda data: dec)
        return sess.evaluate_image("img", source).results[0]

    # an RGB8 group, no cms: the fused call at the planes' own depth
    row = one(S.ImageData.rgb(ref, w, h), decoded(icc_profile=p3))
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference(0, ref)
        b.set_test_yuv_icc(0, 0, image(ce, *dec_p, Y.SUB_420), 8, profiles["p3"])
        m = ce.MetricResult.from_c(b.run(1, ce.MetricConfig.all())[0])
    finally:
        b.close()
    assert key(row) == key(m) and m.psnr is not None
    untagged = one(S.ImageData.rgb(ref, w, h), decoded())
    assert key(untagged) != key(row)
    # a session with a cms converts on the host and uploads RGB8: with the restatement as the cms, the same bytes and scores
    cms = lambda profile, rgb: R.to_srgb(rgb, profile, 8, 8)
    assert key(one(S.ImageData.rgb(ref, w, h), decoded(icc_profile=p3), cms=cms)) == key(row)
    # a linear group (a source in linear light): rgb_depth 16
    src_lin = ce.srgb_table(8, 0)[ref]
    row = one(S.ImageData.linear_f32(src_lin, w, h), decoded(icc_profile=p3))
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        b.set_reference(0, src_lin)
        b.set_test_yuv_icc(0, 0, image(ce, *dec_p, Y.SUB_420), 16, profiles["p3"])
        m = ce.MetricResult.from_c(b.run(1, ce.MetricConfig.all())[0])
    finally:
        b.close()
    assert key(row) == (m.dssim, m.ssimulacra2, m.butteraugli, None) and m.ssimulacra2 is not None
    # a profile neither parser takes: the no-`icc`-feature error, word for word; both a colour and a profile: refused as packed images are
    with pytest.raises(ce.MetricCalculation) as e:
        one(S.ImageData.rgb(ref, w, h), decoded(icc_profile=b"not a profile"))
    assert str(e.value).endswith("Metric calculation failed: ICC: ICC profile support requires the 'icc' feature")
    with pytest.raises(ce.MetricCalculation, match="both a colour description and an ICC profile"):
        one(S.ImageData.linear_f32(src_lin, w, h), decoded(icc_profile=p3, colour=ce.ColourDescription.SRGB))


@pytest.mark.parametrize("device", [False, True])
def test_set_between_launch_and_collect_is_ordered(ce, gpu_ctx, profiles, device):
    """A fused ingest into slots that a launch in flight still reads waits for that launch on the device, from host planes
    (behind the staging copy) and from CE_MEM_DEVICE planes (read in place) alike: the collect returns the first images'
    scores, the launch that follows sees the second images.  (tests/test_gpu_yuv_linear.py's case of the same name.)"""
    ref, test = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    cfg = ce.MetricConfig.all()
    kw = dict(matrix=Y.BT709, range=Y.LIMITED, depth=10, msb_aligned=True)
    prof = profiles["p3"]
    first = [forward_planes(x, Y.BT709, Y.LIMITED, 10, Y.SUB_420, msb=True) for x in (ref, test)]
    second = [forward_planes(x, Y.BT709, Y.LIMITED, 10, Y.SUB_420, msb=True) for x in (np.ascontiguousarray(test[::-1]), np.ascontiguousarray(ref[::-1, ::-1]))]
    keep = []

    def fill(b, planes, dev):
        imgs = [image(ce, *p, Y.SUB_420, Y.SEMIPLANAR, **kw) for p in planes]
        if dev:
            imgs = [device_planes(ce, im, keep) for im in imgs]
        b.set_reference_yuv_icc(0, imgs[0], 10, prof)
        b.set_test_yuv_icc(0, 0, imgs[1], 10, prof)

    def alone(planes):
        b = gpu_ctx.batch_deep(w, h, 1, 1, 10, 10)
        try:
            fill(b, planes, False)
            return [scores_tuple(s) for s in b.run(1, cfg)]
        finally:
            b.close()

    want_first, want_second = alone(first), alone(second)
    assert want_first != want_second and want_first[0][0] == 0 and want_second[0][0] == 0
    b = gpu_ctx.batch_deep(w, h, 1, 1, 10, 10)
    try:
        fill(b, first, device)
        b.launch(1, cfg)
        fill(b, second, device)  # while the launch is in flight
        assert [scores_tuple(s) for s in b.collect(1)] == want_first
        assert [scores_tuple(s) for s in b.run(1, cfg)] == want_second
        got = read_slab(ce, b.test_slab, w * h * 6)
        assert np.array_equal(got, raw(K.composed(*second[1], w, h, Y.SUB_420, Y.BT709, Y.LIMITED, Y.TRIANGLE, 10, True, "p3", 10, ("u16", 10))))
    finally:
        b.close()
        keep.clear()


def test_refusals_leave_the_batch_usable(ce, gpu_ctx, profiles):
    w, h = 16, 10
    rng = np.random.default_rng(23)
    y, cb, cr = Y.random_planes(rng, w, h, Y.SUB_420)
    y10, cb10, cr10 = Y.random_planes(rng, w, h, Y.SUB_420, 10)
    good, good10 = ce.YuvImage([y, cb, cr]), ce.YuvImage([y10, cb10, cr10], depth=10)
    prof = profiles["p3"]
    args = (y, cb, cr, w, h, Y.SUB_420, Y.BT601, Y.FULL, Y.TRIANGLE, 8, False, "p3", 8)
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
    out_f, out_8, out_16 = np.empty(w * h * 3, np.float32), np.empty(w * h * 3, np.uint8), np.empty(w * h * 3, np.uint16)
    lin, plain, deep = gpu_ctx.batch_linear(w, h, 1, 1), ce.Batch(gpu_ctx, w, h, 1, 1), gpu_ctx.batch_deep(w, h, 1, 1, 12, 16)
    other_ctx = ce.Context(1) if ce.device_count() > 1 else None
    other_prof = ce.IccProfile(other_ctx, K.profile_bytes("p3")) if other_ctx else None
    try:
        firsts = []
        for b in (lin, plain, deep):
            b.set_reference_yuv_icc(0, good, 8, prof)
            b.set_test_yuv_icc(0, 0, ce.YuvImage([y, cr, cb]), 8, prof)
            firsts.append(scores_tuple(b.run(1, ce.MetricConfig.all())[0]))
            assert firsts[-1][0] == 0 and (firsts[-1][1] & 7) == 7

        def refused(what, img_c, D, handle):
            calls = [lambda b=b: lib.ce_batch_set_reference_yuv_icc(b._h, 0, img_c, D, handle) for b in (lin, plain, deep)]
            calls += [lambda b=b: lib.ce_batch_set_test_yuv_icc(b._h, 0, 0, img_c, D, handle) for b in (lin, plain, deep)]
            calls += [lambda: lib.ce_yuv_icc_to_linear(gpu_ctx._h, img_c, D, handle, w, h, out_f.ctypes.data, out_f.size),
                      lambda: lib.ce_yuv_icc_to_srgb8(gpu_ctx._h, img_c, D, handle, w, h, out_8.ctypes.data, out_8.size),
                      lambda: lib.ce_yuv_icc_to_srgb16(gpu_ctx._h, img_c, D, handle, w, h, 10, out_16.ctypes.data, out_16.size)]
            for call in calls:
                assert call() == ce.CE_ERR_INVALID_ARG, what
                assert gpu_ctx._err(), what

        for what, (c, _keep) in bad_images.items():
            refused(what, C.byref(c), 8, prof._h)
        gc = good._c()[0]
        refused("null image", None, 8, prof._h)
        refused("null handle", C.byref(gc), 8, None)
        for D in (0, 9, 11, 14, 32):
            refused(f"rgb_depth {D}", C.byref(gc), D, prof._h)
        c10, _keep10 = good10._c()
        refused("rgb_depth under the samples'", C.byref(c10), 8, prof._h)
        if other_prof is not None:
            refused("a profile of another device", C.byref(gc), 8, other_prof._h)
        # slot indices past the batch; the output depth of the u16 leaf; wrong lengths
        assert lib.ce_batch_set_reference_yuv_icc(plain._h, 1, C.byref(gc), 8, prof._h) == ce.CE_ERR_INVALID_ARG
        assert lib.ce_batch_set_test_yuv_icc(plain._h, 1, 0, C.byref(gc), 8, prof._h) == ce.CE_ERR_INVALID_ARG
        assert lib.ce_yuv_icc_to_srgb16(gpu_ctx._h, C.byref(gc), 8, prof._h, w, h, 9, out_16.ctypes.data, out_16.size) == ce.CE_ERR_INVALID_ARG
        assert lib.ce_yuv_icc_to_linear(gpu_ctx._h, C.byref(gc), 8, prof._h, w, h, out_f.ctypes.data, out_f.size - 3) == ce.CE_ERR_BAD_LENGTH
        assert lib.ce_yuv_icc_to_srgb8(gpu_ctx._h, C.byref(gc), 8, prof._h, w, h, out_8.ctypes.data, out_8.size + 1) == ce.CE_ERR_BAD_LENGTH
        assert lib.ce_yuv_icc_to_srgb16(gpu_ctx._h, C.byref(gc), 8, prof._h, w, h, 10, out_16.ctypes.data, 0) == ce.CE_ERR_BAD_LENGTH
        # *_yuv on a linear batch stays refused, in its own words
        assert lib.ce_batch_set_reference_yuv(lin._h, 0, C.byref(gc)) == ce.CE_ERR_INVALID_ARG
        assert gpu_ctx._err() == "Y'CbCr ingest writes integer RGB: a linear batch takes planes through ce_batch_set_*_yuv_cicp"
        # after all of that: the slots are what they were, the batches score what they scored, and the calls work
        for b, first in zip((lin, plain, deep), firsts):
            assert scores_tuple(b.run(1, ce.MetricConfig.all())[0]) == first
        assert np.array_equal(read_slab(ce, lin.reference_slab, w * h * 12), raw(K.composed(*args, ("lin", 0))))
        assert np.array_equal(read_slab(ce, plain.reference_slab, w * h * 3), raw(K.composed(*args, ("u8", 8))))
        assert np.array_equal(read_slab(ce, deep.reference_slab, w * h * 6), raw(K.composed(*args, ("u16", 12))))
        assert np.array_equal(gpu_ctx.yuv_icc_to_srgb(good, w, h, 8, prof, 16), K.composed(*args, ("u16", 16)))
    finally:
        for x in (lin, plain, deep):
            x.close()
        table.close()
        if other_prof is not None:
            other_prof.close()
            other_ctx.close()
