"""SSIM / MS-SSIM on the device (ce_batch_msssim, ce_eval_pair_msssim, ce_eval_pair_msssim_deep).  The
definition is made of correctly rounded f64 operations and integer sums, so every integer of every pair must equal the numpy
restatement (tests/msssim_restatement.py) exactly, and the doubles finished from them within 1e-14 relative (only libm's pow
may differ): on RGB8 and deep batches, at every edge of the level kernel's tile, with one level and with five, through the
pair -> reference table, through the leaves, after a tensor ingest, and beside a launch whose results it must leave alone."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as K  # noqa: E402
import msssim_restatement as M  # noqa: E402

pytestmark = pytest.mark.gpu

Q = 1 << 32


def batch_of(ce, ctx, w, h, depth, deep, n_refs, n_pairs):
    return ctx.batch_deep(w, h, n_refs, n_pairs, depth, depth) if deep else ce.Batch(ctx, w, h, n_refs, n_pairs)


def one_pair(ce, ctx, ref, test, depth, deep, levels=5):
    h, w, _ = ref.shape
    b = batch_of(ce, ctx, w, h, depth, deep, 1, 1)
    try:
        b.set_reference(0, ref.astype(np.uint16) if deep else ref)
        b.set_test(0, 0, test.astype(np.uint16) if deep else test)
        return b.ms_ssim(1, levels)[0]
    finally:
        b.close()


@pytest.mark.parametrize("w,h,depth", [(w, h, 8) for w, h in K.SHAPES_8 + K.TILE_EDGES] + K.DEEP, ids=lambda v: str(v))
def test_five_levels_equal_the_restatement_on_every_integer(ce, gpu_ctx, w, h, depth):
    ref, test = K.pair(w, h, depth)
    got = one_pair(ce, gpu_ctx, ref, test, depth, depth != 8)
    K.check_integers(got, K.expected(w, h, depth), (w, h, depth))
    assert got.n == tuple((lw - 10) * (lh - 10) for lw, lh in M.levels_of(w, h, 5)) and 0.35 < got.ms_ssim < 1.0
    print(f"{w} x {h} depth {depth}: ssim {got.ssim!r} ms_ssim {got.ms_ssim!r}")


@pytest.mark.parametrize("w,h", K.ONE_LEVEL, ids=lambda v: str(v))
def test_one_level_on_the_smallest_images(ce, gpu_ctx, w, h):
    ref, test = K.pair(w, h, 8)
    got = one_pair(ce, gpu_ctx, ref, test, 8, False, 1)
    K.check_integers(got, K.expected(w, h, 8, 1), (w, h))
    assert got.n_levels == 1 and np.isnan(got.ms_ssim) and all(np.isnan(v) for v in got.ms_ssim_rgb)
    assert got.n == ((w - 10) * (h - 10), 0, 0, 0, 0) and got.ssim_q[1:] == ((0, 0, 0),) * 4
    r16, t16 = K.pair(w, h, 16)
    K.check_integers(gpu_ctx.ms_ssim(r16, t16, w, h, 1, depth=16), K.expected(w, h, 16, 1), (w, h, 16))


def test_shared_references_pair_table_leaves_and_rgb8_against_deep(ce, gpu_ctx):
    """Five pairs on three references bound out of order, in slots that are no identity; fewer pairs than the batch holds; the
    same pairs through both leaves; and the RGB8 batch against a deep 8 / 8 batch, bit for bit."""
    w, h = 176, 163
    refs = [K.pair(w, h, 8, s)[0] for s in range(3)]
    tests = [K.pair(w, h, 8, s)[1] for s in (1, 0, 2, 2, 0)]
    binding = [1, 0, 2, 1, 0]  # pair 3: test of seed 2 against reference of seed 1
    wants = [K.expected(w, h, 8, 5, 1), K.expected(w, h, 8, 5, 0), K.expected(w, h, 8, 5, 2), K.expected(w, h, 8, 5, 2, 1),
             K.expected(w, h, 8, 5, 0)]
    results = []
    for deep in (False, True):
        b = batch_of(ce, gpu_ctx, w, h, 8, deep, 4, 6)
        try:
            for p in (3, 0, 4, 2, 1):
                b.set_test(p, binding[p], tests[p].astype(np.uint16) if deep else tests[p])
            for i in (2, 0, 1):
                b.set_reference(i, refs[i].astype(np.uint16) if deep else refs[i])
            got = b.ms_ssim(5)
            for p in range(5):
                K.check_integers(got[p], wants[p], (deep, p))
            assert b.ms_ssim(5) == got and b.ms_ssim(2) == got[:2]  # again, and fewer pairs: reference 2 is not named
            ssim_only = b.ms_ssim(5, 1)
            assert [s.ssim_q[0] for s in ssim_only] == [s.ssim_q[0] for s in got] and [s.ssim for s in ssim_only] == [s.ssim for s in got]
            b.bind_pair(0, 0)  # rebinding alone reaches the device
            K.check_integers(b.ms_ssim(1)[0], K.expected(w, h, 8, 5, 1, 0), "rebound")
            results.append(got)
        finally:
            b.close()
    assert results[0] == results[1]
    assert gpu_ctx.ms_ssim(refs[1], tests[3], w, h) == results[0][3]
    assert gpu_ctx.ms_ssim(refs[1].astype(np.uint16), tests[3].astype(np.uint16), w, h, depth=8) == results[0][3]
    r10, t10 = K.pair(192, 256, 10)
    K.check_integers(gpu_ctx.ms_ssim(r10, t10, 192, 256, depth=10), K.expected(192, 256, 10), "deep leaf")


def test_identical_pair_and_inverted_checkerboard(ce, gpu_ctx):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 1 << 16, (163, 161, 3)).astype(np.uint16)
    got = gpu_ctx.ms_ssim(img, img.copy(), 161, 163, depth=16)
    for l in range(5):
        assert got.ssim_q[l] == (got.n[l] * Q,) * 3 and got.cs_q[l] == (got.n[l] * Q,) * 3
    assert got.ssim == 1.0 and got.ms_ssim == 1.0 and got.ssim_rgb == (1.0,) * 3 and got.ms_ssim_rgb == (1.0,) * 3
    a, b = K.checkerboard(192, 176)
    got = gpu_ctx.ms_ssim(a, b, 192, 176)
    K.check_integers(got, M.msssim(a, b, 8, 5), "checkerboard")
    assert all(v < 0 for l in range(3) for v in got.cs_q[l]) and got.ms_ssim == 0.0 and got.ssim < 0


def test_tensor_ingested_float_pair_equals_the_quantised_samples(ce, gpu_ctx):
    """A float32 CHW pair off the 8-bit grid (the samples / 255 plus noise of +-1.3 steps) through the tensor ingest (DESIGN.md
    section 26) scores as its quantised samples, uploaded"""
    w, h = 176, 163
    ref8, test8 = K.pair(w, h, 8)
    rng = np.random.default_rng(26)
    fr = (ref8.astype(np.float32) / np.float32(255.0) + (rng.random(ref8.shape, np.float32) - np.float32(0.5)) / np.float32(100.0)).transpose(2, 0, 1).copy()
    ft = (test8.astype(np.float32) / np.float32(255.0) + (rng.random(ref8.shape, np.float32) - np.float32(0.5)) / np.float32(100.0)).transpose(2, 0, 1).copy()
    qr, qt = ce.quantise_tensor(fr, 8).transpose(1, 2, 0).copy(), ce.quantise_tensor(ft, 8).transpose(1, 2, 0).copy()
    assert qr.dtype == np.uint8 and not np.array_equal(qr, ref8)
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference_tensor(0, ce.TensorImage.from_array(fr, "CHW"))
        b.set_test_tensor(0, [0], ce.TensorImage.from_array(ft, "CHW"))
        got = b.ms_ssim(1)[0]
    finally:
        b.close()
    assert got == gpu_ctx.ms_ssim(qr, qt, w, h)
    K.check_integers(got, M.msssim(qr, qt, 8, 5), "tensor")


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_a_launch_collected_across_the_call_keeps_its_scores_and_diffmap(ce, gpu_ctx):
    w, h = 176, 163
    ref, test = K.pair(w, h, 8)
    cfg = ce.MetricConfig.all()
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference(0, ref)
        b.set_test(0, 0, test)
        scores = b.run(1, cfg, butteraugli_diffmap=True)
        diffmap = b.butteraugli_diffmaps(0, 1).copy()
        b.launch(1, cfg, butteraugli_diffmap=True)
        got = b.ms_ssim(1)[0]
        again = b.collect(1)
        key = lambda s: (bits(s.dssim), bits(s.ssimulacra2), bits(s.butteraugli), bits(s.psnr), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in scores] and again[0].valid == 15
        assert np.array_equal(b.butteraugli_diffmaps(0, 1), diffmap)
        K.check_integers(got, K.expected(w, h, 8), "beside a launch")
    finally:
        b.close()


def test_every_refusal_leaves_the_batch_usable(ce, gpu_ctx):
    w, h = 176, 163
    ref, test = K.pair(w, h, 8)
    L = ce.lib()
    out = (ce.CeMsssimScores * 4)()
    b = ce.Batch(gpu_ctx, w, h, 1, 2)
    try:
        b.set_reference(0, ref)
        b.set_test(0, 0, test)
        b.set_test(1, 0, ref)
        before = b.ms_ssim(2)
        for n_pairs, levels in ((2, 0), (2, 2), (2, 4), (2, 6), (0, 5), (3, 5)):
            assert L.ce_batch_msssim(b._h, n_pairs, levels, out) == ce.CE_ERR_INVALID_ARG, (n_pairs, levels)
            assert gpu_ctx._err() != ""
        assert L.ce_batch_msssim(b._h, 2, 5, None) == ce.CE_ERR_INVALID_ARG
        assert L.ce_batch_msssim(None, 2, 5, out) == ce.CE_ERR_INVALID_ARG
        assert b.ms_ssim(2) == before
    finally:
        b.close()
    # batches the call is not defined on, and images too small for the levels asked for: usable afterwards
    linear = gpu_ctx.batch_linear(w, h, 1, 1)
    uneven = gpu_ctx.batch_deep(w, h, 1, 1, 10, 12)
    small = ce.Batch(gpu_ctx, 160, 200, 1, 1)
    tiny = ce.Batch(gpu_ctx, 10, 40, 1, 1)
    try:
        for other, levels, word in ((linear, 5, "linear"), (uneven, 5, "depth"), (small, 5, "160"), (tiny, 1, "11"), (tiny, 5, "160")):
            with pytest.raises(ce.CodecEvalError) as e:
                other.ms_ssim(1, levels)
            assert e.value.status == ce.CE_ERR_INVALID_ARG and word in str(e.value), str(e.value)
        r, t = K.pair(160, 200, 8, 0)[0], K.pair(160, 200, 8, 0)[1]
        small.set_reference(0, r)
        small.set_test(0, 0, t)
        K.check_integers(small.ms_ssim(1, 1)[0], M.msssim(r, t, 8, 1), "small, one level")
        assert small.run(1, ce.MetricConfig(psnr=True))[0].valid == ce.METRIC_PSNR
    finally:
        for x in (linear, uneven, small, tiny):
            x.close()
    # the leaves: wrong lengths, null pointers, an empty image, a depth that is none, levels, a size too small
    one = ce.CeMsssimScores()
    ctx, rp, tp, n = gpu_ctx._h, ref.ctypes.data, test.ctypes.data, ref.nbytes
    assert L.ce_eval_pair_msssim(ctx, rp, n - 3, tp, n, w, h, 5, one) == ce.CE_ERR_BAD_LENGTH
    assert L.ce_eval_pair_msssim(ctx, rp, n, tp, n + 3, w, h, 5, one) == ce.CE_ERR_BAD_LENGTH
    assert L.ce_eval_pair_msssim(ctx, None, n, tp, n, w, h, 5, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim(ctx, rp, n, None, n, w, h, 5, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim(ctx, rp, n, tp, n, w, h, 5, None) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim(None, rp, n, tp, n, w, h, 5, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim(ctx, rp, 0, tp, 0, 0, h, 5, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim(ctx, rp, n, tp, n, w, h, 3, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim(ctx, rp, 160 * 170 * 3, tp, 160 * 170 * 3, 160, 170, 5, one) == ce.CE_ERR_INVALID_ARG
    assert "160" in gpu_ctx._err()
    r16, t16 = ref.astype(np.uint16), test.astype(np.uint16)
    assert L.ce_eval_pair_msssim_deep(ctx, r16.ctypes.data, 2 * n, t16.ctypes.data, 2 * n, 9, w, h, 5, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim_deep(ctx, r16.ctypes.data, 2 * n, t16.ctypes.data, n, 8, w, h, 5, one) == ce.CE_ERR_BAD_LENGTH
    assert C.sizeof(one) == 352
    K.check_integers(gpu_ctx.ms_ssim(ref, test, w, h), K.expected(w, h, 8), "leaf after the refusals")
