"""What the two resamplers share on one context - the tap tables of an axis, keyed by (in, out, filter) for both, and the
image between the passes - when RGB8 and linear-light calls of the same geometry alternate on a context that has no table
yet: every output equals its restatement (tests/resample_restatement.py, tests/resample_linear_restatement.py) bit for
bit, a repeat equals the first result, and batches give what the leaves give.  Then every refusal of the resampling calls,
with its status and its message as the library words them.  No tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_linear_restatement as RL  # noqa: E402
import resample_restatement as R8  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 23, 9
SIZES = ((11, 5), (23, 5), (11, 9), (23, 9))  # both passes, the vertical one alone, the horizontal one alone, the byte copy


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def read_device(ce, ctx, address, nbytes):
    """Device bytes -> host (the test's own readback: the ABI has none for the slabs)."""
    ctx.synchronize()
    out = np.empty(nbytes, np.uint8)
    assert ce.lib().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(address), C.c_size_t(nbytes), 2) == 0
    return out


def scores_bits(scores):
    return [(s.status, s.valid) + tuple(int(np.float64(v).view(np.uint64)) for v in (s.dssim, s.psnr)) for s in scores]


def test_rgb8_and_linear_calls_alternate_on_a_fresh_context(ce):
    assert ce.device_count() > 0
    n_refs, binding = 2, (1, 0, 1)
    imgs8 = [R8.content(W, H, "noise", seed=i) for i in range(5)]
    imgsf = [RL.content(W, H, seed=i, negatives=i % 2 == 0) for i in range(5)]
    ow, oh = SIZES[0]
    with ce.Context(0) as ctx:
        leaves8, leavesf = {}, {}
        for filt in R8.FILTERS:
            # the leaves: the linear call meets the RGB8 call's keys on both axes and needs a larger image between the passes
            first8 = ctx.resample_rgb8(imgs8[0], W, H, ow, oh, filt)
            firstf = ctx.resample_linear(imgsf[0], W, H, ow, oh, filt)
            assert np.array_equal(first8, R8.resample(imgs8[0], ow, oh, filt)), filt
            assert np.array_equal(bits(firstf), bits(RL.resample(imgsf[0], ow, oh, filt))), filt
            assert np.array_equal(ctx.resample_rgb8(imgs8[0], W, H, ow, oh, filt), first8), filt
            assert np.array_equal(bits(ctx.resample_linear(imgsf[0], W, H, ow, oh, filt)), bits(firstf)), filt
            for sw, sh in SIZES[1:]:
                assert np.array_equal(ctx.resample_rgb8(imgs8[0], W, H, sw, sh, filt), R8.resample(imgs8[0], sw, sh, filt)), (sw, sh, filt)
                assert np.array_equal(bits(ctx.resample_linear(imgsf[0], W, H, sw, sh, filt)), bits(RL.resample(imgsf[0], sw, sh, filt))), (sw, sh, filt)
            leaves8[filt] = [first8] + [ctx.resample_rgb8(im, W, H, ow, oh, filt) for im in imgs8[1:]]
            leavesf[filt] = [firstf] + [ctx.resample_linear(im, W, H, ow, oh, filt) for im in imgsf[1:]]
        assert np.array_equal(ctx.resample_rgb8(imgs8[0], W, H, W, H), imgs8[0])
        assert np.array_equal(bits(ctx.resample_linear(imgsf[0], W, H, W, H)), bits(imgsf[0]))

        # the same alternation on batches of that context: 2 references and 3 pairs, with their bindings
        src8, dst8 = ce.Batch(ctx, W, H, 2, 3), ce.Batch(ctx, ow, oh, 2, 3)
        srcf, dstf = ctx.batch_linear(W, H, 2, 3), ctx.batch_linear(ow, oh, 2, 3)
        try:
            for src, imgs in ((src8, imgs8), (srcf, imgsf)):
                for i in range(n_refs):
                    src.set_reference(i, imgs[i])
                for i, r in enumerate(binding):
                    src.set_test(i, r, imgs[n_refs + i])

            def check(src, dst, leaves, bpp, filt, config):
                src.resample_pairs_into(dst, n_refs, 3, filter=filt)
                n = ow * oh * bpp
                want = [np.ascontiguousarray(x).view(np.uint8).reshape(-1) for x in leaves[filt]]
                assert np.array_equal(read_device(ce, ctx, dst.reference_slab, n * n_refs), np.concatenate(want[:n_refs])), (bpp, filt)
                assert np.array_equal(read_device(ce, ctx, dst.test_slab, n * 3), np.concatenate(want[n_refs:])), (bpp, filt)
                # the bindings: the scores of the resampled batch are those of a batch loaded with the leaves' outputs and bound by hand
                manual = ctx.batch_linear(ow, oh, 2, 3) if bpp == 12 else ce.Batch(ctx, ow, oh, 2, 3)
                try:
                    for i in range(n_refs):
                        manual.set_reference(i, leaves[filt][i])
                    for i, r in enumerate(binding):
                        manual.set_test(i, r, leaves[filt][n_refs + i])
                    assert scores_bits(dst.run(3, config)) == scores_bits(manual.run(3, config)), (bpp, filt)
                finally:
                    manual.close()
                assert [dst.pair_reference(i) for i in range(3)] == list(binding)

            config = ce.MetricConfig(dssim=True, psnr=True)  # what an 11 x 5 image can be scored with
            for filt in R8.FILTERS:
                for _ in range(2):
                    check(src8, dst8, leaves8, 3, filt, config)
                    check(srcf, dstf, leavesf, 12, filt, config)
        finally:
            for b in (src8, dst8, srcf, dstf):
                b.close()


def refused(ctx, rc, status, message):
    assert rc == status, (rc, ctx._err())
    assert ctx._err() == message


def test_refusals_of_the_leaves(gpu_ctx, ce):
    ctx, L = gpu_ctx, ce.lib()
    INV, LZ = ce.CE_ERR_INVALID_ARG, ce.RESAMPLE_LANCZOS3
    img8, imgf = R8.content(W, H, "noise", seed=0), RL.content(W, H, seed=0)
    for fn, img, out, bpp in ((L.ce_resample_rgb8, img8, np.empty((5, 11, 3), np.uint8), 3),
                              (L.ce_resample_linear, imgf, np.empty((5, 11, 3), np.float32), 12)):
        n_in, n_out = W * H * bpp, 11 * 5 * bpp

        def call(rgb=img.ctypes.data, n=n_in, w=W, h=H, ow=11, oh=5, filt=LZ, o=out.ctypes.data, on=n_out):
            return fn(ctx._h, rgb, n, w, h, ow, oh, filt, o, on)

        # null pointers, then the filter, then empty sides, then the lengths in bytes, input before output
        refused(ctx, call(rgb=None, filt=9), INV, "resample: null pointer")
        refused(ctx, call(o=None, filt=9), INV, "resample: null pointer")
        assert fn(None, img.ctypes.data, n_in, W, H, 11, 5, LZ, out.ctypes.data, n_out) == INV
        assert ce.lib().ce_last_error(None) == b"resample: null pointer"
        for filt in (4, -1):
            refused(ctx, call(filt=filt, w=0), INV, f"resample: unknown filter {filt}")
        for kw, text in (({"w": 0}, f"0 x {H} to 11 x 5"), ({"h": 0}, f"{W} x 0 to 11 x 5"), ({"ow": 0}, f"{W} x {H} to 0 x 5"),
                         ({"oh": 0}, f"{W} x {H} to 11 x 0")):
            refused(ctx, call(n=1, **kw), INV, f"resample: {text} has an empty side")
        refused(ctx, call(n=n_in - bpp, on=n_out - bpp), ce.CE_ERR_BAD_LENGTH, f"Invalid image size: expected {n_in} bytes, got {n_in - bpp}")
        refused(ctx, call(on=n_out + bpp), ce.CE_ERR_BAD_LENGTH, f"Invalid image size: expected {n_out} bytes, got {n_out + bpp}")
        assert call() == 0


def test_refusals_between_batches(gpu_ctx, ce):
    ctx, L = gpu_ctx, ce.lib()
    INV, LZ, T, R = ce.CE_ERR_INVALID_ARG, ce.RESAMPLE_LANCZOS3, ce.BATCH_TESTS, ce.BATCH_REFERENCES
    deep_only = "resample works on RGB8 and linear batches: a deep batch is out of its scope"
    deep_linear = "resample: a linear batch resamples into a linear batch only, and a deep batch is out of its scope"
    mixed = "resample: a linear batch resamples into a linear batch only, an RGB8 batch into an RGB8 one"
    other = ce.Context(0)
    src, dst = ce.Batch(ctx, W, H, 2, 4), ce.Batch(ctx, 11, 5, 3, 3)
    lsrc, ldst = ctx.batch_linear(W, H, 2, 4), ctx.batch_linear(11, 5, 3, 3)
    deep, far = ctx.batch_deep(11, 5, 2, 3, 10, 10), ce.Batch(other, 11, 5, 2, 3)
    try:
        for kind, (a, b) in (("rgb8", (src, dst)), ("linear", (lsrc, ldst))):
            one = lambda s, d, which=T, first=0, count=1, filt=LZ: L.ce_batch_resample(s, d, which, first, count, filt)
            pairs = lambda s, d, n_refs=2, n_pairs=3, filt=LZ: L.ce_batch_resample_pairs(s, d, n_refs, n_pairs, filt)
            # a null batch (the message goes to the other batch's context), contexts, the same batch, the filter, the kinds ...
            for call in (one, pairs):
                refused(ctx, call(None, b._h, filt=9), INV, "resample: null batch")
                refused(ctx, call(a._h, None, filt=9), INV, "resample: null batch")
                if kind == "rgb8":
                    refused(ctx, call(a._h, far._h, filt=9), INV, "resample: the two batches belong to different contexts")
                refused(ctx, call(a._h, a._h, filt=9), INV, "resample: source and destination are the same batch")
                refused(ctx, call(a._h, b._h, filt=4), INV, "resample: unknown filter 4")
                refused(ctx, call(a._h, deep._h), INV, deep_only if kind == "rgb8" else deep_linear)
                refused(ctx, call(deep._h, b._h), INV, deep_only if kind == "rgb8" else deep_linear)
            # ... then the slab, then the range
            refused(ctx, one(a._h, b._h, which=7, count=0), INV, "resample: unknown slab 7")
            refused(ctx, one(a._h, b._h, first=3, count=2), INV, "resample: tests [3, 5) outside the 3 slots both batches have")
            refused(ctx, one(a._h, b._h, count=0), INV, "resample: tests [0, 0) outside the 3 slots both batches have")
            refused(ctx, one(a._h, b._h, first=0xFFFFFFFF, count=2), INV, "resample: tests [4294967295, 4294967297) outside the 3 slots both batches have")
            refused(ctx, one(a._h, b._h, which=R, first=1, count=2), INV, "resample: references [1, 3) outside the 2 slots both batches have")
            # pairs: references before tests before the bindings
            refused(ctx, pairs(a._h, b._h, n_refs=3, n_pairs=4), INV, "resample: references [0, 3) outside the 2 slots both batches have")
            refused(ctx, pairs(a._h, b._h, n_pairs=4), INV, "resample: tests [0, 4) outside the 3 slots both batches have")
            a.bind_pair(1, 1)
            refused(ctx, pairs(a._h, b._h, n_refs=1), INV, "resample: pair 1 is bound to reference 1, outside the 1 resampled")
            assert pairs(a._h, b._h) == 0 and one(a._h, b._h) == 0
        for s, d in ((src, ldst), (lsrc, dst)):
            refused(ctx, L.ce_batch_resample(s._h, d._h, T, 0, 1, LZ), INV, mixed)
            refused(ctx, L.ce_batch_resample_pairs(s._h, d._h, 2, 3, LZ), INV, mixed)
    finally:
        for b in (src, dst, lsrc, ldst, deep, far):
            b.close()
        other.close()
