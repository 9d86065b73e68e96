"""CIEDE2000 on the device (ce_batch_ciede2000, ce_eval_pair_ciede2000, ce_eval_pair_ciede2000_deep).  The
definition is made of separately rounded IEEE f64 operations and integers, so the device must equal the numpy restatement
(tests/ciede2000_restatement.py) exactly - the sum, the maximum and every count of every pair - and the three doubles finished
from them to 1e-14 relative: on both load paths, with one and with several blocks a pair and with a grid-stride loop that goes
round, on RGB8 batches and deep ones of equal and unequal depths, through a pair -> reference table that is no identity, with
and without thresholds, right behind the uploads and beside a launch that is still to be collected."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_cases as K  # noqa: E402
import ciede2000_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def tables(ce):
    K.use(ce)
    return K.TABLES


def batch_of(ce, ctx, w, h, kind, max_refs, max_pairs):
    return ce.Batch(ctx, w, h, max_refs, max_pairs) if kind == (0, 0) else ctx.batch_deep(w, h, max_refs, max_pairs, kind[0], kind[1])


def load(ce, ctx, w, h, kind, n_pairs=5, spare=2):
    """The case's two references and n_pairs tests (the five in turn) in a batch with room for `spare` more pairs and a spare
    reference, the tests bound before the references and out of order."""
    refs, tests = K.images(w, h, kind)
    b = batch_of(ce, ctx, w, h, kind, 3, n_pairs + spare)
    for p in reversed(range(n_pairs)):
        b.set_test(p, K.BINDING[p % 5], tests[p % 5])
    for i in (1, 0):
        b.set_reference(i, refs[i])
    return b


@pytest.mark.parametrize("kind", K.KINDS, ids=lambda k: "rgb8" if k == (0, 0) else "deep%d_%d" % k)
@pytest.mark.parametrize("w,h", K.SHAPES, ids=lambda v: str(v))
def test_batch_equals_restatement_exactly(ce, gpu_ctx, w, h, kind):
    b = load(ce, gpu_ctx, w, h, kind)
    try:
        got = b.ciede2000(5, K.THRESHOLDS)  # right behind the uploads: nothing was synchronised
        for p, want in enumerate(K.expected(w, h, kind)):
            K.check(got[p], want, (w, h, kind, p))
        none = b.ciede2000(5)
        for p, want in enumerate(K.expected(w, h, kind, False)):
            K.check(none[p], want, (w, h, kind, p, "no thresholds"))
            assert none[p].n_above == ()
        assert b.ciede2000(5, K.THRESHOLDS) == got and b.ciede2000(2, K.THRESHOLDS) == got[:2]  # again, and fewer pairs
        assert b.ciede2000(5, K.THRESHOLDS[2:5]) == [type(g)(g.mean, g.max, g.ciede2000_db, g.sum_q20, g.max_q20, g.n, g.n_above[2:5]) for g in got]
    finally:
        b.close()


@pytest.mark.parametrize("kind", [(0, 0), (16, 16), (12, 16)], ids=lambda k: "rgb8" if k == (0, 0) else "deep%d_%d" % k)
def test_more_pixels_than_the_launch_has_lanes(ce, gpu_ctx, kind):
    """512 x 520 with sixteen pairs: 64 blocks a pair on the wide path, fewer lanes than units of 16 (RGB8) or 8 (deep) pixels."""
    w, h = K.BIG
    deep = kind != (0, 0)
    assert K.wide(w * h, deep) and K.blocks(w * h, K.BIG_PAIRS, deep) == 64 and K.goes_round(w * h, K.BIG_PAIRS, deep)
    b = load(ce, gpu_ctx, w, h, kind, K.BIG_PAIRS, 0)
    try:
        got = b.ciede2000(K.BIG_PAIRS, K.THRESHOLDS)
        want = K.expected(w, h, kind)
        for p in range(K.BIG_PAIRS):
            K.check(got[p], want[p % 5], (kind, p))
    finally:
        b.close()


def test_leaves_equal_the_batch_and_rgb8_equals_deep_8(ce, gpu_ctx):
    w, h = 16, 8
    for kind in K.KINDS:
        refs, tests = K.images(w, h, kind)
        want = K.expected(w, h, kind)
        for p in range(5):
            r, t = refs[K.BINDING[p]], tests[p]
            got = (gpu_ctx.ciede2000(r, t, w, h, K.THRESHOLDS) if kind == (0, 0)
                   else gpu_ctx.ciede2000(r, t, w, h, K.THRESHOLDS, depth=kind[0], test_depth=kind[1]))
            K.check(got, want[p], ("leaf", kind, p))
    refs, tests = K.images(333, 251, (0, 0))
    want = K.expected(333, 251, (0, 0))[3]
    K.check(gpu_ctx.ciede2000(refs[1], tests[3], 333, 251, K.THRESHOLDS), want, "rgb8 leaf")
    K.check(gpu_ctx.ciede2000(refs[1].astype(np.uint16), tests[3].astype(np.uint16), 333, 251, K.THRESHOLDS, depth=8), want, "deep 8 / 8 leaf")


def test_identical_images_black_and_white_and_the_host_function(ce, gpu_ctx, tables):
    rng = np.random.default_rng(30)
    for depth in (0, 10, 16):
        img = rng.integers(0, 256 if depth == 0 else 1 << depth, (8, 16, 3)).astype(np.uint8 if depth == 0 else np.uint16)
        got = gpu_ctx.ciede2000(img, img.copy(), 16, 8, [0], depth=depth)
        assert (got.sum_q20, got.max_q20, got.n, got.n_above) == (0, 0, 128, (0,)) and got.mean == 0.0 and got.ciede2000_db == float("inf")
    v8 = rng.integers(0, 256, (5, 7, 3))
    got = gpu_ctx.ciede2000(v8.astype(np.uint16), (257 * v8).astype(np.uint16), 7, 5, depth=8, test_depth=16)
    assert got.sum_q20 == 0 and got.max_q20 == 0  # equal table values, unequal codes and depths: no pixel is skipped, every q is 0
    black, white = np.zeros((3, 5, 3), np.uint8), np.full((3, 5, 3), 255, np.uint8)
    got = gpu_ctx.ciede2000(black, white, 5, 3, [(100 << 20) - 1, 100 << 20])
    assert (got.sum_q20, got.max_q20, got.n_above) == (15 * (100 << 20), 100 << 20, (15, 0)) and got.mean == 100.0 and got.max == 100.0
    assert abs(got.ciede2000_db - 5.0) <= 1e-13  # 45 - 20 log10(100)
    # the host function and the device, pixel by pixel: one-pixel images
    a = np.array(K.ANCHORS, np.uint8)
    host = ce.ciede2000_pixels(a[:, 0], a[:, 1])
    for i in range(len(a)):
        assert gpu_ctx.ciede2000(a[i, 0].reshape(1, 1, 3), a[i, 1].reshape(1, 1, 3), 1, 1).sum_q20 == int(host[i]), K.ANCHORS[i]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_a_launch_collected_across_the_call_keeps_its_scores(ce, gpu_ctx):
    w, h = 96, 64
    refs, tests = K.images(w, h, (0, 0))
    cfg = ce.MetricConfig.all()
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference(0, refs[1])
        b.set_test(0, 0, tests[0])
        scores = b.run(1, cfg, butteraugli_diffmap=True)
        diffmap = b.butteraugli_diffmaps(0, 1).copy()
        b.launch(1, cfg, butteraugli_diffmap=True)
        got = b.ciede2000(1, K.THRESHOLDS)[0]
        again = b.collect(1)
        key = lambda s: (bits(s.dssim), bits(s.ssimulacra2), bits(s.butteraugli), bits(s.psnr), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in scores] and again[0].valid == 15
        assert np.array_equal(b.butteraugli_diffmaps(0, 1), diffmap)
        K.check(got, R.scores(K.q_of(refs[1], tests[0], (0, 0)), K.THRESHOLDS), "beside a launch")
    finally:
        b.close()


def test_every_refusal_leaves_the_batch_usable(ce, gpu_ctx):
    w, h = 16, 8
    refs, tests = K.images(w, h, (0, 0))
    L = ce.lib()
    out = (ce.CeCiede2000Scores * 4)()
    thr = (C.c_uint32 * 9)(*range(9))
    b = ce.Batch(gpu_ctx, w, h, 1, 2)
    try:
        b.set_reference(0, refs[0])
        b.set_test(0, 0, tests[1])
        b.set_test(1, 0, tests[4])
        before = b.ciede2000(2, K.THRESHOLDS)
        for n_pairs, n_thr in ((0, 8), (3, 8), (2, 9)):
            assert L.ce_batch_ciede2000(b._h, n_pairs, thr, n_thr, out) == ce.CE_ERR_INVALID_ARG, (n_pairs, n_thr)
            assert gpu_ctx._err() != ""
        assert "at most 8" in gpu_ctx._err()
        assert L.ce_batch_ciede2000(b._h, 2, None, 3, out) == ce.CE_ERR_INVALID_ARG
        assert L.ce_batch_ciede2000(b._h, 2, thr, 8, None) == ce.CE_ERR_INVALID_ARG
        assert L.ce_batch_ciede2000(None, 2, thr, 8, out) == ce.CE_ERR_INVALID_ARG
        assert b.ciede2000(2, K.THRESHOLDS) == before
        assert b.run(2, ce.MetricConfig(psnr=True))[0].valid == ce.METRIC_PSNR
    finally:
        b.close()
    linear = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        with pytest.raises(ce.CodecEvalError) as e:
            linear.ciede2000(1)
        assert e.value.status == ce.CE_ERR_INVALID_ARG and "Delta E ITP" in str(e.value)
        lin = np.full((h, w, 3), 0.5, np.float32)
        linear.set_reference(0, lin)
        linear.set_test(0, 0, lin)
        assert linear.hdr_fidelity(1)[0].itp_sum_q20 == 0
    finally:
        linear.close()
    # the leaves: wrong lengths, null pointers, an empty image, depths that are none, too many thresholds
    one = ce.CeCiede2000Scores()
    ref, test = refs[0], tests[1]
    ctx, rp, tp, n = gpu_ctx._h, ref.ctypes.data, test.ctypes.data, ref.nbytes
    assert L.ce_eval_pair_ciede2000(ctx, rp, n - 3, tp, n, w, h, None, 0, one) == ce.CE_ERR_BAD_LENGTH
    assert L.ce_eval_pair_ciede2000(ctx, rp, n, tp, n + 3, w, h, None, 0, one) == ce.CE_ERR_BAD_LENGTH
    assert L.ce_eval_pair_ciede2000(ctx, None, n, tp, n, w, h, None, 0, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_ciede2000(ctx, rp, n, None, n, w, h, None, 0, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_ciede2000(ctx, rp, n, tp, n, w, h, None, 0, None) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_ciede2000(None, rp, n, tp, n, w, h, None, 0, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_ciede2000(ctx, rp, 0, tp, 0, 0, h, None, 0, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_ciede2000(ctx, rp, n, tp, n, w, h, thr, 9, one) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_ciede2000(ctx, rp, n, tp, n, w, h, None, 2, one) == ce.CE_ERR_INVALID_ARG
    r16, t16 = ref.astype(np.uint16), test.astype(np.uint16)
    for dr, dt in ((9, 8), (8, 14), (0, 8)):
        assert L.ce_eval_pair_ciede2000_deep(ctx, r16.ctypes.data, 2 * n, t16.ctypes.data, 2 * n, dr, dt, w, h, None, 0, one) == ce.CE_ERR_INVALID_ARG
        assert "depths" in gpu_ctx._err()
    assert L.ce_eval_pair_ciede2000_deep(ctx, r16.ctypes.data, 2 * n, t16.ctypes.data, n, 8, 8, w, h, None, 0, one) == ce.CE_ERR_BAD_LENGTH
    assert C.sizeof(one) == 120
    K.check(gpu_ctx.ciede2000(ref, test, w, h, K.THRESHOLDS), K.expected(w, h, (0, 0))[1], "leaf after the refusals")
