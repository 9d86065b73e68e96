"""Linear-light batches resampled on the device: ce_resample_linear / ce_batch_resample on linear
batches against the numpy restatement (tests/resample_linear_restatement.py, itself pinned to Pillow's mode "F" resize in
test_resample_linear_cpu.py) bit for bit; scoring a resampled batch against uploading the restated floats; score_under and
EvalSession's simulate_viewing on linear-light work against the manual route; the checkerboard that separates averaging
light from averaging code values; what a resample must leave alone; every refusal.  No tolerance anywhere."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_linear_restatement as RL  # noqa: E402
import resample_restatement as R8  # noqa: E402

pytestmark = pytest.mark.gpu

CE = importlib.import_module("codec-eval_amd")
S = importlib.import_module("codec-eval_amd.session")
V = importlib.import_module("codec-eval_amd.viewing")

RATIOS = ((1, 3), (1, 2), (2, 3), (1, 1), (3, 2), (3, 1))
SHAPES = ((8, 8), (9, 301), (301, 9), (100, 76), (257, 129))

_restated = {}


def restated(img, key, ow, oh, filt):
    """RL.resample, computed once per (image key, shape, filter) and shared between the tests."""
    k = (key, ow, oh, filt)
    if k not in _restated:
        _restated[k] = RL.resample(img, ow, oh, filt)
        _restated[k].setflags(write=False)
    return _restated[k]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def read_floats(ce, ctx, address, count):
    """Device floats -> host (the test's own readback: the ABI has none for the slabs)."""
    ctx.synchronize()
    out = np.empty(count, np.float32)
    assert ce.lib().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(address), ctypes.c_size_t(out.nbytes), 2) == 0
    return out


def scores_tuple(s):
    """status, valid and the scores as a MetricResult carries them (None where `valid` leaves a metric out)."""
    m = CE.MetricResult.from_c(s)
    return (s.status, s.valid, m.dssim, m.ssimulacra2, m.butteraugli, m.psnr)


@pytest.mark.parametrize("w,h", SHAPES)
def test_leaf_equals_the_restatement(gpu_ctx, ce, w, h):
    img = RL.content(w, h, seed=3, negatives=True)
    for num, den in RATIOS:
        ow, oh = RL.scaled(w, num, den), RL.scaled(h, num, den)
        for filt in RL.FILTERS:
            got = gpu_ctx.resample_linear(img, w, h, ow, oh, filt)
            assert got.shape == (oh, ow, 3) and got.dtype == np.float32
            assert np.array_equal(bits(got), bits(restated(img, ("leaf", w, h), ow, oh, filt))), (w, h, ow, oh, filt)
    # one axis only: the other pass is skipped
    for ow, oh in ((w, RL.scaled(h, 2, 3)), (RL.scaled(w, 3, 2), h)):
        assert np.array_equal(bits(gpu_ctx.resample_linear(img, w, h, ow, oh)), bits(RL.resample(img, ow, oh, RL.LANCZOS3)))


def test_leaf_one_pixel_tile_edges_route_boundary_and_the_largest_case(gpu_ctx, ce):
    one = np.array([[[0.25, -2.0, 125.0]]], np.float32)
    for filt in RL.FILTERS:
        assert np.array_equal(bits(gpu_ctx.resample_linear(one, 1, 1, 5, 3, filt)), bits(np.broadcast_to(one, (3, 5, 3))))
    # 3 * out_w floats on both sides of one and two 256-float tiles: 255, 258, 510, 513
    for ow in (85, 86, 170, 171):
        for w in (2 * ow, 57):
            img = RL.content(w, 3, seed=ow, negatives=True)
            assert np.array_equal(bits(gpu_ctx.resample_linear(img, w, 3, ow, 3)), bits(RL.resample(img, ow, 3))), (w, ow)
        img = RL.content(ow, 7, seed=ow, negatives=True)  # the vertical pass over such rows
        assert np.array_equal(bits(gpu_ctx.resample_linear(img, ow, 7, ow, 3)), bits(RL.resample(img, ow, 3))), ow
    # ksize 69 is the last a tile's taps fit in LDS for, ksize 71 reads the global table
    for w in (336, 345):
        img = RL.content(w, 4, seed=w, negatives=True)
        assert np.array_equal(bits(gpu_ctx.resample_linear(img, w, 4, 30, 2)), bits(RL.resample(img, 30, 2))), w
    big = RL.content(768, 512, seed=9, negatives=True)
    assert np.array_equal(bits(gpu_ctx.resample_linear(big, 768, 512, 384, 256)), bits(restated(big, "big", 384, 256, RL.LANCZOS3)))


def test_clamp_and_equal_size(gpu_ctx, ce):
    img = np.zeros((4, 32, 3), np.float32)
    img[:, 16:] = 1023.0
    got = gpu_ctx.resample_linear(img, 32, 4, 48, 4)
    assert got.max() == np.float32(RL.LINEAR_MAX) and got.min() < 0.0
    assert RL.resample(img, 48, 4, clamp=False).max() > RL.LINEAR_MAX
    assert np.array_equal(bits(got), bits(RL.resample(img, 48, 4)))
    # equal sizes return the input's bits, unclamped (the leaf takes its input as it is)
    raw = np.array([[[5000.0, -0.0, 1e-42], [np.inf, -7.5, 1024.0]]], np.float32)
    for filt in RL.FILTERS:
        assert np.array_equal(bits(gpu_ctx.resample_linear(raw, 2, 1, 2, 1, filt)), bits(raw))


@pytest.mark.parametrize("w,h,ow,oh", [(257, 129, 193, 97), (100, 76, 300, 228), (9, 301, 5, 151), (64, 48, 64, 48)])
def test_batch_resample_both_slabs_and_nonzero_first(gpu_ctx, ce, w, h, ow, oh):
    n_refs, n_pairs = 3, 5
    refs = [RL.content(w, h, seed=20 + i, negatives=True) for i in range(n_refs)]
    tests = [RL.content(w, h, seed=40 + i, negatives=i % 2 == 0) for i in range(n_pairs)]
    src, dst = gpu_ctx.batch_linear(w, h, n_refs, n_pairs), gpu_ctx.batch_linear(ow, oh, n_refs + 1, n_pairs + 2)
    try:
        for i, r in enumerate(refs):
            src.set_reference(i, r)
        for i, t in enumerate(tests):
            src.set_test(i, i % n_refs, t)
        n = ow * oh * 3
        sentinel = np.full(n, 777.0, np.float32)
        for i in range(n_refs + 1):
            dst.set_reference(i, sentinel)
        for i in range(n_pairs + 2):
            dst.set_test(i, 0, sentinel)
        for filt in RL.FILTERS:
            src.resample_into(dst, 1, 2, tests=False, filter=filt)  # references [1, 3)
            src.resample_into(dst, 2, 3, tests=True, filter=filt)   # tests [2, 5)
            got_r = read_floats(ce, gpu_ctx, dst.reference_slab, n * (n_refs + 1)).reshape(n_refs + 1, oh, ow, 3)
            got_t = read_floats(ce, gpu_ctx, dst.test_slab, n * (n_pairs + 2)).reshape(n_pairs + 2, oh, ow, 3)
            for i in (1, 2):
                assert np.array_equal(bits(got_r[i]), bits(restated(refs[i], ("bref", w, h, i), ow, oh, filt))), ("ref", i, filt)
            for i in (2, 3, 4):
                assert np.array_equal(bits(got_t[i]), bits(restated(tests[i], ("btest", w, h, i), ow, oh, filt))), ("test", i, filt)
            for i in (0, 3):  # nothing outside the ranges was written
                assert np.array_equal(got_r[i].reshape(-1), sentinel)
            for i in (0, 1, 5, 6):
                assert np.array_equal(got_t[i].reshape(-1), sentinel)
    finally:
        src.close(), dst.close()


def _grid(ce, workloads, w, h, n_refs=2, per_ref=3):
    """Linear floats with highlights: references and distorted tests, pair -> reference interleaved."""
    t0 = ce.srgb_table(8, 0)
    refs8 = [np.asarray(workloads.make_reference(w, h, 50 + i), np.uint8).reshape(h, w, 3) for i in range(n_refs)]
    refs = [(t0[r] * np.float32(4.0)).astype(np.float32) for r in refs8]
    tests, binding = [], []
    for q in (35, 70, 92)[:per_ref]:
        for i in range(n_refs):
            t8 = np.asarray(workloads.distort(refs8[i], q), np.uint8).reshape(h, w, 3)
            tests.append((t0[t8] * np.float32(4.0) - np.float32(0.01)).astype(np.float32))
            binding.append(i)
    return refs, tests, binding


def _fill(batch, refs, tests, binding):
    for i, r in enumerate(refs):
        batch.set_reference(i, r)
    for i, (t, r) in enumerate(zip(tests, binding)):
        batch.set_test(i, r, t)


def _manual(ce, ctx, refs, tests, binding, ow, oh, config, filt=RL.LANCZOS3, maps=False):
    """The host route: restate every image at (ow, oh), upload into a fresh linear batch of that shape, run."""
    b = ctx.batch_linear(ow, oh, len(refs), len(tests))
    try:
        _fill(b, [RL.resample(r, ow, oh, filt) for r in refs], [RL.resample(t, ow, oh, filt) for t in tests], binding)
        scores = [scores_tuple(s) for s in b.run(len(tests), config, butteraugli_diffmap=maps)]
        return scores, ((b.butteraugli_diffmaps(0, len(tests)), b.dssim_ssim_maps(0, 0, len(tests))[0]) if maps else None)
    finally:
        b.close()


@pytest.mark.parametrize("ow,oh,filt", [(48, 40, RL.LANCZOS3), (144, 120, RL.BICUBIC), (128, 107, RL.BOX)])
def test_resample_pairs_then_run_equals_uploading_the_restated_floats(gpu_ctx, ce, workloads, ow, oh, filt):
    w, h = 96, 80
    refs, tests, binding = _grid(ce, workloads, w, h)
    config = ce.MetricConfig.all()
    src, dst = gpu_ctx.batch_linear(w, h, 2, 6), gpu_ctx.batch_linear(ow, oh, 2, 6)
    try:
        _fill(src, refs, tests, binding)
        src.resample_pairs_into(dst, 2, 6, filter=filt)
        got = [scores_tuple(s) for s in dst.run(6, config, butteraugli_diffmap=True)]
        got_maps = (dst.butteraugli_diffmaps(0, 6), dst.dssim_ssim_maps(0, 0, 6)[0])
        want, want_maps = _manual(ce, gpu_ctx, refs, tests, binding, ow, oh, config, filt, maps=True)
        assert got == want
        assert all(s[0] == 0 and s[1] == 7 for s in got)  # PSNR is not defined on a linear batch
        assert all(np.array_equal(a, b) for a, b in zip(got_maps, want_maps))
        assert [dst.pair_reference(i) for i in range(6)] == binding
    finally:
        src.close(), dst.close()


def _results(rs):
    return [(r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in rs]


def test_score_under_on_a_linear_batch_equals_the_manual_route(gpu_ctx, ce, workloads, monkeypatch):
    w, h = 64, 48
    refs, tests, binding = _grid(ce, workloads, w, h)
    config = ce.MetricConfig.all()
    src = gpu_ctx.batch_linear(w, h, 2, 6)
    try:
        _fill(src, refs, tests, binding)
        conds = [V.presets.srcset_1x_on_laptop(), V.presets.native_desktop(), V.presets.srcset_2x_on_desktop(), V.presets.srcset_2x_on_laptop_1_5x()]
        out = V.score_under(gpu_ctx, src, 2, 6, conds, V.SimulationMode.Accurate, config)
        manual = {}
        for o in out:
            shape = o.condition.simulation_params(w, h, V.SimulationMode.Accurate).displayed_size(w, h)
            assert o.displayed_size == shape
            if shape not in manual:
                manual[shape] = [s[2:] for s in _manual(ce, gpu_ctx, refs, tests, binding, shape[0], shape[1], config)[0]]
            assert _results(o.results) == manual[shape], shape
        assert sorted(manual) == sorted({(128, 96), (64, 48), (32, 24), (48, 36)})
        assert _results(out[1].results) == [scores_tuple(s)[2:] for s in src.run(6, config)]  # displayed as it is: the batch itself
        # a budget that holds two pairs at a time: the chunked route gives the same scores
        monkeypatch.setenv("CE_VIEWING_BATCH_BYTES", str(ce.estimate_batch_bytes_linear(128, 96, 2, 2, config)))
        for o in V.score_under(gpu_ctx, src, 2, 6, [conds[0], conds[2]], V.SimulationMode.Accurate, config):
            assert _results(o.results) == manual[o.displayed_size]
    finally:
        src.close()


def test_session_simulate_viewing_on_a_pq_bt2020_decode(gpu_ctx, ce, workloads, tmp_path):
    w, h = 64, 48
    ref8 = np.asarray(workloads.make_reference(w, h, 4), np.uint8).reshape(h, w, 3)
    test8 = np.asarray(workloads.distort(ref8, 55), np.uint8).reshape(h, w, 3)
    rng = np.random.default_rng(2)
    decode10 = np.clip(test8.astype(np.int32) * 3 + rng.integers(0, 4, test8.shape), 0, 1023).astype(np.uint16)
    lin = (ce.srgb_table(8, 0)[test8] * np.float32(1.5)).astype(np.float32)
    pq = ce.ColourDescription.BT2020_PQ

    def sweep(**kw):
        cfg = S.EvalConfig.builder().report_dir(str(tmp_path)).metrics(ce.MetricConfig.all()).quality_levels([50.0]).build()
        for k, v in kw.items():
            setattr(cfg, k, v)
        sess = S.EvalSession(cfg, ctx=gpu_ctx)
        enc = lambda img, req: b"x"
        sess.add_codec_with_decode("pq", "1", enc, lambda data: S.ImageData.rgb16(decode10, w, h, 10, colour=pq))
        sess.add_codec_with_decode("f32", "1", enc, lambda data: S.ImageData.linear_f32(lin, w, h))
        sess.add_codec_with_decode("flat", "1", enc, lambda data: S.ImageData.rgb(test8, w, h))
        return {r.codec_id: (r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in sess.evaluate_image("img", S.ImageData.rgb(ref8, w, h)).results}

    def manual(ow, oh):
        ref_f = gpu_ctx.cicp_to_linear(ref8, w, h, ce.ColourDescription.SRGB)
        dec_f = gpu_ctx.cicp_to_linear(decode10, w, h, pq)
        b = gpu_ctx.batch_linear(ow, oh, 1, 2)
        try:
            b.set_reference(0, RL.resample(ref_f, ow, oh))
            b.set_test(0, 0, RL.resample(dec_f, ow, oh))
            b.set_test(1, 0, RL.resample(lin, ow, oh))
            return [scores_tuple(s)[2:] for s in b.run(2, ce.MetricConfig.all())]
        finally:
            b.close()

    plain = sweep()
    at_size = manual(w, h)
    assert (plain["pq"], plain["f32"]) == (at_size[0], at_size[1])
    # None: everything as before, whatever condition the config carries; a native condition displays the image as it is
    assert sweep(viewing=V.presets.srcset_2x_on_desktop(), simulate_viewing=None) == plain
    assert sweep(viewing=V.presets.native_laptop(), simulate_viewing=V.SimulationMode.Accurate) == plain
    # a 2x image on a 1x desktop is looked at at half its size; a 1x image on a 2x laptop at twice
    for cond, (ow, oh) in ((V.presets.srcset_2x_on_desktop(), (32, 24)), (V.presets.srcset_1x_on_laptop(), (128, 96))):
        shown = sweep(viewing=cond, simulate_viewing=V.SimulationMode.Accurate)
        want = manual(ow, oh)
        assert (shown["pq"], shown["f32"]) == (want[0], want[1]), (ow, oh)
        assert shown["pq"] != plain["pq"]
        m = gpu_ctx.calculate_metrics(R8.resample(ref8, ow, oh), R8.resample(test8, ow, oh), ow, oh, ce.MetricConfig.all())
        assert shown["flat"] == (m.dssim, m.ssimulacra2, m.butteraugli, m.psnr)  # the 8-bit cell keeps the 8-bit route


def test_checkerboard_pair_linear_route_against_rgb8_route(gpu_ctx, ce):
    """A 0 / 1 one-pixel checkerboard against the flat grey that emits the same light (linear 0.5), looked at at half size
    under the box filter.  In linear light the halved checkerboard IS 0.5 exactly and the pair is (nearly) identical; the
    8-bit route averages code values, makes the checkerboard code 128 = 0.2158 in linear light against the grey's code 188
    = 0.503, and reports a large difference."""
    w, h = 64, 48
    y, x = np.mgrid[0:h, 0:w]
    board8 = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    grey8 = np.full((h, w, 3), 188, np.uint8)
    t0 = ce.srgb_table(8, 0)
    config = ce.MetricConfig.all()
    cond = [V.presets.srcset_2x_on_desktop()]
    lin, small = gpu_ctx.batch_linear(w, h, 1, 1), gpu_ctx.batch_linear(32, 24, 1, 1)
    plain = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        lin.set_reference(0, t0[board8])
        lin.set_test(0, 0, t0[grey8])
        plain.set_reference(0, board8)
        plain.set_test(0, 0, grey8)
        lin.resample_pairs_into(small, 1, 1, filter=ce.RESAMPLE_BOX)
        assert (read_floats(ce, gpu_ctx, small.reference_slab, 32 * 24 * 3) == np.float32(0.5)).all()
        assert (bits(read_floats(ce, gpu_ctx, small.test_slab, 32 * 24 * 3)) == bits(t0[188])).all()
        a = V.score_under(gpu_ctx, lin, 1, 1, cond, V.SimulationMode.Accurate, config, filter=ce.RESAMPLE_BOX)[0].results[0]
        b = V.score_under(gpu_ctx, plain, 1, 1, cond, V.SimulationMode.Accurate, config, filter=ce.RESAMPLE_BOX)[0].results[0]
        print(f"checkerboard pair at half size: linear route dssim {a.dssim!r} ssimulacra2 {a.ssimulacra2!r} butteraugli {a.butteraugli!r}; "
              f"RGB8 route dssim {b.dssim!r} ssimulacra2 {b.ssimulacra2!r} butteraugli {b.butteraugli!r}")
        assert a.dssim < b.dssim and a.butteraugli < b.butteraugli and a.ssimulacra2 > b.ssimulacra2
    finally:
        lin.close(), small.close(), plain.close()


def test_a_resample_leaves_the_source_batch_alone_and_is_safe_before_collect(gpu_ctx, ce, workloads):
    w, h = 96, 80
    refs, tests, binding = _grid(ce, workloads, w, h)
    config = ce.MetricConfig.all()
    src, dst = gpu_ctx.batch_linear(w, h, 2, 6), gpu_ctx.batch_linear(48, 40, 2, 6)
    try:
        _fill(src, refs, tests, binding)
        first = [scores_tuple(s) for s in src.run(6, config, butteraugli_diffmap=True)]
        maps = (src.butteraugli_diffmaps(0, 6), src.dssim_ssim_maps(1, 0, 6)[0])
        src.resample_pairs_into(dst, 2, 6)
        assert [scores_tuple(s) for s in src.collect(6)] == first
        again = (src.butteraugli_diffmaps(0, 6), src.dssim_ssim_maps(1, 0, 6)[0])
        assert all(np.array_equal(a, b) for a, b in zip(maps, again))
        want = _manual(ce, gpu_ctx, refs, tests, binding, 48, 40, config)[0]
        assert [scores_tuple(s) for s in dst.run(6, config)] == want
        # between launch and collect of the source
        src.launch(6, config)
        src.resample_pairs_into(dst, 2, 6, filter=ce.RESAMPLE_BICUBIC)
        assert [scores_tuple(s) for s in src.collect(6)] == first
        assert [scores_tuple(s) for s in dst.run(6, config)] == _manual(ce, gpu_ctx, refs, tests, binding, 48, 40, config, RL.BICUBIC)[0]
        # and with the destination's own earlier launch still uncollected
        dst.launch(6, config)
        src.resample_pairs_into(dst, 2, 6)
        assert [scores_tuple(s) for s in dst.run(6, config)] == want
    finally:
        src.close(), dst.close()


def test_every_refusal_leaves_the_batches_usable(gpu_ctx, ce, workloads):
    w, h = 64, 48
    refs, tests, binding = _grid(ce, workloads, w, h)
    config = ce.MetricConfig.all()
    L = ce.lib()
    src, dst = gpu_ctx.batch_linear(w, h, 2, 6), gpu_ctx.batch_linear(32, 24, 2, 4)
    plain, deep = ce.Batch(gpu_ctx, 32, 24, 2, 4), gpu_ctx.batch_deep(32, 24, 2, 4, 10, 10)
    try:
        _fill(src, refs, tests, binding)
        before = [scores_tuple(s) for s in src.run(6, config)]
        T, Rf, LZ = ce.BATCH_TESTS, ce.BATCH_REFERENCES, ce.RESAMPLE_LANCZOS3
        for reasons, call in (
                (("linear",), lambda: L.ce_batch_resample(src._h, plain._h, T, 0, 1, LZ)),
                (("linear",), lambda: L.ce_batch_resample(plain._h, dst._h, T, 0, 1, LZ)),
                (("linear",), lambda: L.ce_batch_resample_pairs(src._h, plain._h, 2, 4, LZ)),
                (("linear", "deep"), lambda: L.ce_batch_resample(src._h, deep._h, T, 0, 1, LZ)),
                (("linear", "deep"), lambda: L.ce_batch_resample(deep._h, dst._h, T, 0, 1, LZ)),
                (("linear", "deep"), lambda: L.ce_batch_resample_pairs(deep._h, dst._h, 2, 4, LZ)),
                (("deep",), lambda: L.ce_batch_resample(plain._h, deep._h, T, 0, 1, LZ)),
                (("filter",), lambda: L.ce_batch_resample(src._h, dst._h, T, 0, 1, 4)),
                (("filter",), lambda: L.ce_batch_resample(src._h, dst._h, T, 0, 1, -1)),
                (("filter",), lambda: L.ce_batch_resample_pairs(src._h, dst._h, 2, 4, 9)),
                (("slab",), lambda: L.ce_batch_resample(src._h, dst._h, 7, 0, 1, LZ)),
                (("outside",), lambda: L.ce_batch_resample(src._h, dst._h, T, 0, 0, LZ)),
                (("outside",), lambda: L.ce_batch_resample(src._h, dst._h, T, 3, 2, LZ)),  # past dst's 4 test slots
                (("outside",), lambda: L.ce_batch_resample(src._h, dst._h, T, 0xFFFFFFFF, 2, LZ)),
                (("outside",), lambda: L.ce_batch_resample(src._h, dst._h, Rf, 1, 2, LZ)),  # past both batches' 2 references
                (("outside",), lambda: L.ce_batch_resample_pairs(src._h, dst._h, 2, 6, LZ)),
                (("outside",), lambda: L.ce_batch_resample_pairs(src._h, dst._h, 0, 4, LZ)),
                (("bound to reference",), lambda: L.ce_batch_resample_pairs(src._h, dst._h, 1, 4, LZ)),
                (("same batch",), lambda: L.ce_batch_resample(src._h, src._h, T, 0, 1, LZ))):
            assert call() == ce.CE_ERR_INVALID_ARG
            assert all(r in gpu_ctx._err() for r in reasons), (reasons, gpu_ctx._err())
        assert L.ce_batch_resample(None, dst._h, T, 0, 1, LZ) == ce.CE_ERR_INVALID_ARG
        assert L.ce_batch_resample(src._h, None, T, 0, 1, LZ) == ce.CE_ERR_INVALID_ARG
        with pytest.raises(ce.CodecEvalError) as e:
            src.resample_into(plain, 0, 1)
        assert e.value.status == ce.CE_ERR_INVALID_ARG and "linear" in str(e.value)
        # the leaf: null pointers, then the filter, then zero sizes, then the lengths (in bytes), input before output
        img = np.ascontiguousarray(refs[0]).reshape(-1)
        out = np.empty(32 * 24 * 3, np.float32)
        leaf = lambda rgb, n, ww, hh, ow, oh, f, o, on: L.ce_resample_linear(gpu_ctx._h, rgb, n, ww, hh, ow, oh, f, o, on)
        ip, op = img.ctypes.data, out.ctypes.data
        assert leaf(None, img.nbytes, w, h, 32, 24, LZ, op, out.nbytes) == ce.CE_ERR_INVALID_ARG
        assert leaf(ip, img.nbytes, w, h, 32, 24, LZ, None, out.nbytes) == ce.CE_ERR_INVALID_ARG
        assert L.ce_resample_linear(None, ip, img.nbytes, w, h, 32, 24, LZ, op, out.nbytes) == ce.CE_ERR_INVALID_ARG
        assert leaf(ip, img.nbytes - 4, w, h, 32, 24, 4, op, out.nbytes) == ce.CE_ERR_INVALID_ARG and "filter" in gpu_ctx._err()
        for ww, hh, ow, oh in ((0, h, 32, 24), (w, 0, 32, 24), (w, h, 0, 24), (w, h, 32, 0)):
            assert leaf(ip, img.nbytes - 4, ww, hh, ow, oh, LZ, op, out.nbytes) == ce.CE_ERR_INVALID_ARG and "empty side" in gpu_ctx._err()
        assert leaf(ip, img.nbytes - 4, w, h, 32, 24, LZ, op, out.nbytes - 4) == ce.CE_ERR_BAD_LENGTH and str(img.nbytes) in gpu_ctx._err()
        assert leaf(ip, img.size, w, h, 32, 24, LZ, op, out.nbytes) == ce.CE_ERR_BAD_LENGTH  # a count of floats is not a length
        assert leaf(ip, img.nbytes, w, h, 32, 24, LZ, op, out.nbytes + 4) == ce.CE_ERR_BAD_LENGTH and str(out.nbytes) in gpu_ctx._err()
        assert leaf(ip, img.nbytes, w, h, 32, 24, LZ, op, out.nbytes) == 0
        assert np.array_equal(bits(out), bits(RL.resample(refs[0], 32, 24)).reshape(-1))
        # everything still works, and nothing a refused call touched has changed
        assert [scores_tuple(s) for s in src.collect(6)] == before
        assert [scores_tuple(s) for s in src.run(6, config)] == before
        src.resample_pairs_into(dst, 2, 4)
        assert [scores_tuple(s) for s in dst.run(4, config)] == _manual(ce, gpu_ctx, refs, tests[:4], binding[:4], 32, 24, config)[0]
    finally:
        for b in (src, dst, plain, deep):
            b.close()
