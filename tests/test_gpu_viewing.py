"""The viewing simulation on the device: ce_resample_rgb8 / ce_batch_resample against the numpy restatement
(tests/resample_restatement.py, itself pinned to Pillow in test_viewing_cpu.py) byte for byte; scoring a resampled
batch against uploading the restated images; score_under and EvalSession's simulate_viewing against the manual route;
what a resample must leave alone; every refusal."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

S = importlib.import_module("codec-eval_amd.session")
V = importlib.import_module("codec-eval_amd.viewing")

# the displayed / intrinsic size ratios of the eight presets in both directions, plus 3/4
RATIOS = ((1, 3), (1, 2), (2, 3), (3, 4), (1, 1), (4, 3), (3, 2), (2, 1), (3, 1))
SHAPES = ((8, 8), (9, 301), (301, 9), (257, 129), (768, 512))


def read_slab(ce, ctx, address, nbytes):
    """Device bytes -> host (the test's own readback: the ABI has none for the u8 slabs)."""
    ctx.synchronize()
    out = np.empty(nbytes, np.uint8)
    assert ce.lib().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(address), ctypes.c_size_t(nbytes), 2) == 0
    return out


def scores_tuple(s):
    return (s.status, s.valid, s.dssim, s.ssimulacra2, s.butteraugli, s.psnr)


@pytest.mark.parametrize("w,h", SHAPES)
def test_leaf_equals_the_restatement(gpu_ctx, ce, w, h):
    img = R.content(w, h, "noise" if w * h < 100000 else "pattern", seed=3)
    for num, den in RATIOS:
        ow, oh = R.scaled(w, num, den), R.scaled(h, num, den)
        for filt in R.FILTERS:
            got = gpu_ctx.resample_rgb8(img, w, h, ow, oh, filt)
            assert got.shape == (oh, ow, 3)
            assert np.array_equal(got, R.resample(img, ow, oh, filt)), (w, h, ow, oh, filt)
    # one axis only: the other pass is skipped
    for ow, oh in ((w, R.scaled(h, 2, 3)), (R.scaled(w, 3, 2), h)):
        assert np.array_equal(gpu_ctx.resample_rgb8(img, w, h, ow, oh), R.resample(img, ow, oh, R.LANCZOS3))


def test_leaf_noise_768x512_and_uhd_to_1080p(gpu_ctx, ce):
    img = R.content(768, 512, "noise", seed=9)
    for ow, oh, filt in ((256, 171, R.LANCZOS3), (1024, 683, R.BICUBIC), (2304, 1536, R.LANCZOS3), (384, 256, R.BOX)):
        assert np.array_equal(gpu_ctx.resample_rgb8(img, 768, 512, ow, oh, filt), R.resample(img, ow, oh, filt))
    big = R.content(3840, 2160, "noise", seed=4)
    assert np.array_equal(gpu_ctx.resample_rgb8(big, 3840, 2160, 1920, 1080), R.resample(big, 1920, 1080, R.LANCZOS3))
    # a scale beyond what a tile's taps fit in LDS for: the kernel's global-table route
    wide = R.content(2000, 9, "noise", seed=5)
    assert np.array_equal(gpu_ctx.resample_rgb8(wide, 2000, 9, 150, 9), R.resample(wide, 150, 9, R.LANCZOS3))


def test_equal_size_returns_the_input_bytes(gpu_ctx, ce):
    img = R.content(257, 129, "noise", seed=6)
    for filt in R.FILTERS:
        assert np.array_equal(gpu_ctx.resample_rgb8(img, 257, 129, 257, 129, filt), img)
    src, dst = ce.Batch(gpu_ctx, 257, 129, 1, 2), ce.Batch(gpu_ctx, 257, 129, 1, 2)
    try:
        src.set_test(1, 0, img)
        src.resample_into(dst, 1, 1, tests=True)
        assert np.array_equal(read_slab(ce, gpu_ctx, dst.test_slab + img.size, img.size), img.reshape(-1))
    finally:
        src.close(), dst.close()


@pytest.mark.parametrize("w,h,ow,oh", [(257, 129, 193, 97), (100, 76, 300, 228), (9, 301, 5, 151), (768, 512, 384, 256)])
def test_batch_resample_both_slabs_and_nonzero_first(gpu_ctx, ce, w, h, ow, oh):
    n_refs, n_pairs = 3, 5
    refs = [R.content(w, h, "noise", seed=20 + i) for i in range(n_refs)]
    tests = [R.content(w, h, "pattern" if i == 2 else "noise", seed=40 + i) for i in range(n_pairs)]
    src, dst = ce.Batch(gpu_ctx, w, h, n_refs, n_pairs), ce.Batch(gpu_ctx, ow, oh, n_refs + 1, n_pairs + 2)
    try:
        for i, r in enumerate(refs):
            src.set_reference(i, r)
        for i, t in enumerate(tests):
            src.set_test(i, i % n_refs, t)
        sentinel = np.full(ow * oh * 3, 0xA5, np.uint8)
        for i in range(n_refs + 1):
            dst.set_reference(i, sentinel)
        for i in range(n_pairs + 2):
            dst.set_test(i, 0, sentinel)
        out_bytes = ow * oh * 3
        for filt in R.FILTERS:
            src.resample_into(dst, 1, 2, tests=False, filter=filt)  # references [1, 3)
            src.resample_into(dst, 2, 3, tests=True, filter=filt)   # tests [2, 5)
            got_r = read_slab(ce, gpu_ctx, dst.reference_slab, out_bytes * (n_refs + 1)).reshape(n_refs + 1, oh, ow, 3)
            got_t = read_slab(ce, gpu_ctx, dst.test_slab, out_bytes * (n_pairs + 2)).reshape(n_pairs + 2, oh, ow, 3)
            for i in (1, 2):
                assert np.array_equal(got_r[i], R.resample(refs[i], ow, oh, filt)), ("ref", i, filt)
            for i in (2, 3, 4):
                assert np.array_equal(got_t[i], R.resample(tests[i], ow, oh, filt)), ("test", i, filt)
            # nothing outside the ranges was written
            for i in (0, 3):
                assert np.array_equal(got_r[i].reshape(-1), sentinel)
            for i in (0, 1, 5, 6):
                assert np.array_equal(got_t[i].reshape(-1), sentinel)
    finally:
        src.close(), dst.close()


def _grid(workloads, w, h, n_refs=2, per_ref=3):
    refs = [workloads.make_reference(w, h, 50 + i) for i in range(n_refs)]
    tests, binding = [], []
    for q in (35, 70, 92)[:per_ref]:
        for i in range(n_refs):  # interleaved: pair -> reference is not the identity
            tests.append(workloads.distort(refs[i], q))
            binding.append(i)
    return refs, tests, binding


def _fill(batch, refs, tests, binding):
    for i, r in enumerate(refs):
        batch.set_reference(i, r)
    for i, (t, r) in enumerate(zip(tests, binding)):
        batch.set_test(i, r, t)


def _manual_scores(ce, ctx, refs, tests, binding, ow, oh, config, filt=R.LANCZOS3, **run_kw):
    """The host route: restate every image at (ow, oh), upload into a fresh batch of that shape, run."""
    b = ce.Batch(ctx, ow, oh, len(refs), len(tests))
    try:
        _fill(b, [R.resample(r, ow, oh, filt) for r in refs], [R.resample(t, ow, oh, filt) for t in tests], binding)
        scores = [scores_tuple(s) for s in b.run(len(tests), config, **run_kw)]
        maps = b.butteraugli_diffmaps(0, len(tests)) if run_kw.get("butteraugli_diffmap") else None
        return scores, maps
    finally:
        b.close()


@pytest.mark.parametrize("ow,oh,filt", [(48, 40, R.LANCZOS3), (144, 120, R.BICUBIC), (128, 107, R.LANCZOS3)])
def test_resample_pairs_then_run_equals_uploading_the_restated_images(gpu_ctx, ce, workloads, ow, oh, filt):
    w, h = 96, 80
    refs, tests, binding = _grid(workloads, w, h)
    src, dst = ce.Batch(gpu_ctx, w, h, 2, 6), ce.Batch(gpu_ctx, ow, oh, 2, 6)
    try:
        _fill(src, refs, tests, binding)
        src.resample_pairs_into(dst, 2, 6, filter=filt)
        got = [scores_tuple(s) for s in dst.run(6, ce.MetricConfig.all(), butteraugli_diffmap=True)]
        got_maps = dst.butteraugli_diffmaps(0, 6)
        want, want_maps = _manual_scores(ce, gpu_ctx, refs, tests, binding, ow, oh, ce.MetricConfig.all(), filt, butteraugli_diffmap=True)
        assert got == want
        assert all(s[0] == 0 and s[1] == 15 for s in got)
        assert np.array_equal(got_maps, want_maps)
        assert [dst.pair_reference(i) for i in range(6)] == binding
    finally:
        src.close(), dst.close()


def test_score_under_all_presets_equals_the_manual_route(gpu_ctx, ce, workloads, monkeypatch):
    w, h = 64, 48
    refs, tests, binding = _grid(workloads, w, h)
    config = ce.MetricConfig.all()
    src = ce.Batch(gpu_ctx, w, h, 2, 6)
    try:
        _fill(src, refs, tests, binding)
        conds = V.presets.all()
        out = V.score_under(gpu_ctx, src, 2, 6, conds, V.SimulationMode.Accurate, config)
        assert [o.condition for o in out] == conds
        manual = {}
        for o in out:
            p = o.condition.simulation_params(w, h, V.SimulationMode.Accurate)
            shape = p.displayed_size(w, h)
            assert o.params == p and o.displayed_size == shape
            assert (o.dssim_threshold, o.butteraugli_threshold, o.ssimulacra2_threshold) == (
                p.adjust_dssim_threshold(0.0003), p.adjust_butteraugli_threshold(1.0), p.adjust_ssimulacra2_threshold(90.0))
            if shape not in manual:
                manual[shape] = _manual_scores(ce, gpu_ctx, refs, tests, binding, shape[0], shape[1], config)[0]
            got = [(0, 15, r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in o.results]
            assert got == manual[shape], shape
        assert sorted(manual) == sorted({(192, 144), (128, 96), (64, 48), (96, 72), (32, 24), (48, 36)})
        # DownsampleOnly never upscales: the undersized conditions score the images as they are
        down = V.score_under(gpu_ctx, src, 2, 6, conds[:2], V.SimulationMode.DownsampleOnly, config)
        assert all(o.displayed_size == (w, h) and [(0, 15, r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in o.results] == manual[(w, h)]
                   for o in down)
        # a budget that holds two pairs at a time: the chunked route gives the same scores
        fits2 = ce.estimate_batch_bytes(192, 144, 2, 2, config)
        monkeypatch.setenv("CE_VIEWING_BATCH_BYTES", str(fits2))
        chunked = V.score_under(gpu_ctx, src, 2, 6, [conds[0], conds[5]], V.SimulationMode.Accurate, config)
        for o in chunked:
            assert [(0, 15, r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in o.results] == manual[o.displayed_size]
    finally:
        src.close()


def test_a_resample_leaves_the_source_batch_alone_and_is_safe_before_collect(gpu_ctx, ce, workloads):
    w, h = 96, 80
    refs, tests, binding = _grid(workloads, w, h)
    config = ce.MetricConfig.all()
    src, dst = ce.Batch(gpu_ctx, w, h, 2, 6), ce.Batch(gpu_ctx, 48, 40, 2, 6)
    try:
        _fill(src, refs, tests, binding)
        first = [scores_tuple(s) for s in src.run(6, config, butteraugli_diffmap=True, ssimulacra2_maps=True)]
        maps = (src.butteraugli_diffmaps(0, 6), src.dssim_ssim_maps(1, 0, 6)[0], src.ssimulacra2_maps(0, 1, ce.SSIM2_MAP_ARTIFACT, 0, 6)[0])
        src.resample_pairs_into(dst, 2, 6)
        assert [scores_tuple(s) for s in src.collect(6)] == first
        again = (src.butteraugli_diffmaps(0, 6), src.dssim_ssim_maps(1, 0, 6)[0], src.ssimulacra2_maps(0, 1, ce.SSIM2_MAP_ARTIFACT, 0, 6)[0])
        assert all(np.array_equal(a, b) for a, b in zip(maps, again))
        want = _manual_scores(ce, gpu_ctx, refs, tests, binding, 48, 40, config)[0]
        assert [scores_tuple(s) for s in dst.run(6, config)] == want
        # between launch and collect of the source
        src.launch(6, config)
        src.resample_pairs_into(dst, 2, 6, filter=ce.RESAMPLE_BICUBIC)
        assert [scores_tuple(s) for s in src.collect(6)] == first
        assert [scores_tuple(s) for s in dst.run(6, config)] == _manual_scores(ce, gpu_ctx, refs, tests, binding, 48, 40, config, R.BICUBIC)[0]
        # and with the destination's own earlier launch still uncollected
        dst.launch(6, config)
        src.resample_pairs_into(dst, 2, 6)
        assert [scores_tuple(s) for s in dst.run(6, config)] == want
    finally:
        src.close(), dst.close()


def test_session_simulate_viewing(gpu_ctx, ce, workloads, tmp_path):
    def enc(image, request):  # a toy codec: the quantiser step shrinks as quality grows
        step = 1 + int((100.0 - request.quality) / 8.0)
        return np.array([image.width, image.height, step], dtype=np.uint32).tobytes() + image.to_rgb8_vec().tobytes()

    def dec(blob):
        w, h, step = (int(v) for v in np.frombuffer(blob[:12], dtype=np.uint32))
        rgb = np.frombuffer(blob[12:], dtype=np.uint8)
        return S.ImageData.rgb(np.minimum(255, (rgb // step) * step + step // 2).astype(np.uint8), w, h)

    w, h = 96, 80
    src = workloads.make_reference(w, h, 7)
    image = S.ImageData.rgb(src, w, h)

    def sweep(**kw):
        b = S.EvalConfig.builder().report_dir(tmp_path / "rep").metrics(ce.MetricConfig.all()).quality_levels([50, 75, 95])
        cfg = b.build()
        for k, v in kw.items():
            setattr(cfg, k, v)
        ses = S.EvalSession(cfg, ctx=gpu_ctx).add_codec_with_decode("toy", "1.0", enc, dec)
        return [(r.quality, r.dssim, r.ssimulacra2, r.butteraugli, r.psnr, r.perception) for r in ses.evaluate_image("a.png", image).results]

    plain = sweep()
    # None: what the session always returned (the leaf calls at the image's own size), whatever condition it carries
    assert sweep(viewing=V.presets.srcset_2x_on_desktop(), simulate_viewing=None) == plain
    for row in plain:
        decoded = dec(enc(image, S.EncodeRequest(row[0])))
        m = gpu_ctx.calculate_metrics(src, decoded.data, w, h, ce.MetricConfig.all())
        assert row[1:5] == (m.dssim, m.ssimulacra2, m.butteraugli, m.psnr)
    # a native condition displays the image as it is
    assert sweep(viewing=V.presets.native_laptop(), simulate_viewing=V.SimulationMode.Accurate) == plain
    # a 2x image on a 1x desktop is looked at at half its size
    half = sweep(viewing=V.presets.srcset_2x_on_desktop(), simulate_viewing=V.SimulationMode.Accurate)
    small_ref = R.resample(src, 48, 40)
    for row in half:
        decoded = dec(enc(image, S.EncodeRequest(row[0]))).data.reshape(h, w, 3)
        m = gpu_ctx.calculate_metrics(small_ref, R.resample(decoded, 48, 40), 48, 40, ce.MetricConfig.all())
        assert row[1:5] == (m.dssim, m.ssimulacra2, m.butteraugli, m.psnr)
        assert row[5] == m.perception_level()
    assert half != plain
    # DownsampleOnly leaves an undersized image alone
    assert sweep(viewing=V.presets.srcset_1x_on_phone(), simulate_viewing=V.SimulationMode.DownsampleOnly) == plain


def test_every_refusal_leaves_both_batches_usable(gpu_ctx, ce, workloads):
    w, h = 64, 48
    refs, tests, binding = _grid(workloads, w, h)
    config = ce.MetricConfig.all()
    L = ce.lib()
    other = ce.Context(0)
    src, dst = ce.Batch(gpu_ctx, w, h, 2, 6), ce.Batch(gpu_ctx, 32, 24, 2, 4)
    deep = gpu_ctx.batch_deep(w, h, 2, 6, 10, 10)
    foreign = ce.Batch(other, 32, 24, 2, 6)
    try:
        _fill(src, refs, tests, binding)
        src.resample_pairs_into(dst, 2, 4)
        before_src = [scores_tuple(s) for s in src.run(6, config)]
        before_dst = [scores_tuple(s) for s in dst.run(4, config)]
        LZ, T, Rf = ce.RESAMPLE_LANCZOS3, ce.BATCH_TESTS, ce.BATCH_REFERENCES
        bad = [
            ("null", L.ce_batch_resample(None, dst._h, T, 0, 1, LZ)),
            ("null", L.ce_batch_resample(src._h, None, T, 0, 1, LZ)),
            ("contexts", L.ce_batch_resample(src._h, foreign._h, T, 0, 1, LZ)),
            ("same batch", L.ce_batch_resample(src._h, src._h, T, 0, 1, LZ)),
            ("filter", L.ce_batch_resample(src._h, dst._h, T, 0, 1, 4)),
            ("filter", L.ce_batch_resample(src._h, dst._h, T, 0, 1, -1)),
            ("slab", L.ce_batch_resample(src._h, dst._h, 2, 0, 1, LZ)),
            ("outside", L.ce_batch_resample(src._h, dst._h, T, 0, 0, LZ)),
            ("outside", L.ce_batch_resample(src._h, dst._h, T, 3, 2, LZ)),      # past dst's 4 test slots
            ("outside", L.ce_batch_resample(src._h, dst._h, T, 0xFFFFFFFF, 2, LZ)),
            ("outside", L.ce_batch_resample(src._h, dst._h, Rf, 1, 2, LZ)),     # past both batches' 2 references
            ("deep", L.ce_batch_resample(deep._h, dst._h, T, 0, 1, LZ)),
            ("deep", L.ce_batch_resample(src._h, deep._h, T, 0, 1, LZ)),
            ("outside", L.ce_batch_resample_pairs(src._h, dst._h, 2, 6, LZ)),
            ("outside", L.ce_batch_resample_pairs(src._h, dst._h, 0, 4, LZ)),
            ("bound to reference", L.ce_batch_resample_pairs(src._h, dst._h, 1, 4, LZ)),
            ("filter", L.ce_batch_resample_pairs(src._h, dst._h, 2, 4, 9)),
            ("deep", L.ce_batch_resample_pairs(deep._h, dst._h, 2, 4, LZ)),
        ]
        # the reason is read right after each call below; here only the codes
        assert [rc for _, rc in bad] == [ce.CE_ERR_INVALID_ARG] * len(bad)
        for reason, call in (("contexts", lambda: L.ce_batch_resample(src._h, foreign._h, T, 0, 1, LZ)),
                             ("filter", lambda: L.ce_batch_resample(src._h, dst._h, T, 0, 1, 4)),
                             ("outside", lambda: L.ce_batch_resample(src._h, dst._h, T, 3, 2, LZ)),
                             ("deep", lambda: L.ce_batch_resample(deep._h, dst._h, T, 0, 1, LZ)),
                             ("bound to reference", lambda: L.ce_batch_resample_pairs(src._h, dst._h, 1, 4, LZ))):
            assert call() == ce.CE_ERR_INVALID_ARG and reason in gpu_ctx._err()
        with pytest.raises(ce.CodecEvalError) as e:
            src.resample_into(deep, 0, 1)
        assert e.value.status == ce.CE_ERR_INVALID_ARG and "deep" in str(e.value)
        # the leaf: arguments first, then lengths
        img = np.ascontiguousarray(refs[0]).reshape(-1)
        out = np.empty(32 * 24 * 3, np.uint8)
        leaf = lambda *a: L.ce_resample_rgb8(gpu_ctx._h, *a)  # noqa: E731
        assert leaf(None, img.size, w, h, 32, 24, LZ, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
        assert leaf(img.ctypes.data, img.size, w, h, 32, 24, LZ, None, out.size) == ce.CE_ERR_INVALID_ARG
        assert leaf(img.ctypes.data, img.size, w, h, 32, 24, 7, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
        assert leaf(img.ctypes.data, img.size, w, h, 0, 24, LZ, out.ctypes.data, 0) == ce.CE_ERR_INVALID_ARG
        assert leaf(img.ctypes.data, img.size, w, h, 32, 0, LZ, out.ctypes.data, 0) == ce.CE_ERR_INVALID_ARG
        assert "empty side" in gpu_ctx._err()
        assert leaf(img.ctypes.data, img.size - 3, w, h, 32, 24, LZ, out.ctypes.data, out.size) == ce.CE_ERR_BAD_LENGTH
        assert leaf(img.ctypes.data, img.size, w, h, 32, 24, LZ, out.ctypes.data, out.size - 1) == ce.CE_ERR_BAD_LENGTH
        with pytest.raises(ce.MetricCalculation):
            gpu_ctx.resample_rgb8(img[:-3], w, h, 32, 24)
        # both batches still hold what they held and still run
        assert [scores_tuple(s) for s in src.run(6, config)] == before_src
        assert [scores_tuple(s) for s in dst.run(4, config)] == before_dst
        src.resample_pairs_into(dst, 2, 4)
        assert [scores_tuple(s) for s in dst.run(4, config)] == before_dst
    finally:
        for b in (src, dst, deep, foreign):
            b.close()
        other.close()


# ---- the smallest shapes that reach the kernels' edges (the host-compiled run of the same text under sanitizers is
# tests/test_resample_kernel_host_cpu.py; these are exact integers, so everything is array_equal) -------------------------

@pytest.mark.parametrize("ow,oh", [(341, 3), (342, 3)])
def test_slots_at_every_dword_phase(gpu_ctx, ce, ow, oh):
    """A tile is 1024 row bytes counted from the aligned dword that holds the row's first byte.  341 x 3 is 1023 bytes a row
    and 3069 a slot, so four consecutive slots start at all four phases (342 x 3: 1026 and 3078, phases 0 and 2) and the rows
    within a slot move on by 3 (2).  From a two-pass source and a horizontal-only one, with sentinel slots on either side."""
    slot = ow * oh * 3
    assert {(k * slot) % 4 for k in range(1, 5)} == ({0, 1, 2, 3} if ow == 341 else {0, 2})
    sentinel = np.full(slot, 0xA5, np.uint8)
    for w, h in ((682, 6), (171, 3)):
        imgs = [R.content(w, h, "noise", seed=60 + i) for i in range(4)]
        src, dst = ce.Batch(gpu_ctx, w, h, 1, 5), ce.Batch(gpu_ctx, ow, oh, 1, 6)
        try:
            for i, im in enumerate(imgs):
                src.set_test(1 + i, 0, im)
            for filt in R.FILTERS:
                for i in range(6):
                    dst.set_test(i, 0, sentinel)
                src.resample_into(dst, 1, 4, tests=True, filter=filt)
                got = read_slab(ce, gpu_ctx, dst.test_slab, slot * 6).reshape(6, oh, ow, 3)
                for i, im in enumerate(imgs):
                    assert np.array_equal(got[1 + i], R.resample(im, ow, oh, filt)), (w, h, ow, oh, filt, "slot", 1 + i)
                for i in (0, 5):
                    assert np.array_equal(got[i].reshape(-1), sentinel), (w, h, ow, oh, filt, "sentinel", i)
        finally:
            src.close(), dst.close()


@pytest.mark.parametrize("w,h,oh", [(1840, 4, 4), (1841, 4, 4), (1841, 4, 2)])
def test_route_boundary_of_the_horizontal_taps(gpu_ctx, ce, w, h, oh):
    """Lanczos3 to 345 pixels: from 1840 a pixel has 33 taps and a tile's tables are 48 020 bytes, the last that are staged in
    LDS; from 1841 it has 35 and they are read from the global table.  345 pixels are 1035 row bytes: two tiles, three
    images."""
    ow, n = 345, 3
    imgs = [R.content(w, h, "noise", seed=70 + i) for i in range(n)]
    src, dst = ce.Batch(gpu_ctx, w, h, 1, n), ce.Batch(gpu_ctx, ow, oh, 1, n)
    try:
        for i, im in enumerate(imgs):
            src.set_test(i, 0, im)
        src.resample_into(dst, 0, n, tests=True)
        got = read_slab(ce, gpu_ctx, dst.test_slab, ow * oh * 3 * n).reshape(n, oh, ow, 3)
        for i, im in enumerate(imgs):
            assert np.array_equal(got[i], R.resample(im, ow, oh, R.LANCZOS3)), (w, h, ow, oh, i)
    finally:
        src.close(), dst.close()


@pytest.mark.parametrize("h", [1, 5])
def test_leaf_widths_within_a_dword_of_a_tile_boundary(gpu_ctx, ce, h):
    for ow in (340, 341, 342, 343, 682, 683, 684):  # 1020 .. 1029 and 2046 .. 2052 row bytes
        for w in (2 * ow, (ow + 1) // 2):
            img = R.content(w, h, "noise", seed=80)
            assert np.array_equal(gpu_ctx.resample_rgb8(img, w, h, ow, h), R.resample(img, ow, h, R.LANCZOS3)), (w, h, ow)
