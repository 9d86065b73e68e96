"""The SSIM / MS-SSIM maps on the device (ce_batch_msssim_map, ce_eval_pair_msssim_map, ce_eval_pair_msssim_map_deep; DESIGN.md
section 29).  A map value is 2^32 minus an integer the definition pins, a cell is an integer maximum and a count an integer sum,
so every element of every output must equal the numpy restatement (tests/msssim_map_restatement.py) with ==: at every shape
that is one way for the kernel to go wrong (tests/msssim_map_cases.py), every level, both terms, every block, with and without
counts, through the pair -> reference table, on deep batches, through the leaves, and beside a launch and a score call whose
results it must leave alone."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as K  # noqa: E402
import msssim_map_cases as MK  # noqa: E402
import msssim_map_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu


def batch_of(ce, ctx, w, h, depth, deep, n_refs, n_pairs):
    return ctx.batch_deep(w, h, n_refs, n_pairs, depth, depth) if deep else ce.Batch(ctx, w, h, n_refs, n_pairs)


def loaded(ce, ctx, ref, test, depth, deep):
    h, w, _ = ref.shape
    b = batch_of(ce, ctx, w, h, depth, deep, 1, 1)
    b.set_reference(0, ref.astype(np.uint16) if deep else ref)
    b.set_test(0, 0, test.astype(np.uint16) if deep else test)
    return b


@pytest.mark.parametrize("w,h,depth,levels,lvls", MK.SHAPES, ids=lambda v: str(v))
def test_maps_and_counts_equal_the_restatement_on_every_element(ce, gpu_ctx, w, h, depth, levels, lvls):
    ref, test = K.pair(w, h, depth)
    b = loaded(ce, gpu_ctx, ref, test, depth, depth != 8)
    try:
        for level in lvls:
            for what in (("ssim", "cs") if (w, h) == (176, 163) else ("ssim",)):
                want = MK.expected(w, h, depth, levels, level, what)
                m, over = b.ms_ssim_maps(0, 1, levels, level, what, 1, MK.THR8)
                assert m.dtype == np.uint32 and m.shape == (1,) + want.shape and over.dtype == np.uint64 and over.shape == (1, 3, 8)
                assert np.array_equal(m[0], want), (level, what, np.argwhere(m[0] != want)[:4])
                assert np.array_equal(over[0], MK.expected_over(w, h, depth, levels, level, what, MK.THR8)), (level, what)
                cells, none = b.ms_ssim_maps(0, 1, levels, level, what, 16)
                assert none is None and np.array_equal(cells[0], MK.expected(w, h, depth, levels, level, what, 16)), (level, what)
    finally:
        b.close()


@pytest.mark.parametrize("w,h", [(171, 171), (43, 27)], ids=lambda v: str(v))
def test_every_block_counts_only_maps_only_and_repeats(ce, gpu_ctx, w, h):
    levels = 5 if w > 160 else 1
    ref, test = K.pair(w, h, 8)
    b = loaded(ce, gpu_ctx, ref, test, 8, False)
    try:
        for block in MK.BLOCKS:
            want = MK.expected(w, h, 8, levels, 0, "ssim", block)
            m, over = b.ms_ssim_maps(0, 1, levels, 0, "ssim", block, MK.THR8[:3])
            assert np.array_equal(m[0], want), (block, np.argwhere(m[0] != want)[:4])
            # counts are over positions, never over cells, whatever the block
            assert np.array_equal(over[0], MK.expected_over(w, h, 8, levels, 0, "ssim", MK.THR8[:3])), block
            again = b.ms_ssim_maps(0, 1, levels, 0, "ssim", block, MK.THR8[:3])
            assert np.array_equal(again[0], m) and np.array_equal(again[1], over)
        for thr in (MK.THR8[:1], MK.THR8[2:5], MK.THR8):
            m, over = b.ms_ssim_maps(0, 1, levels, 0, "cs", 1, thr, maps=False)
            assert m is None and over.shape == (1, 3, len(thr))
            assert np.array_equal(over[0], MK.expected_over(w, h, 8, levels, 0, "cs", thr)), thr
        m, over = b.ms_ssim_maps(0, 1, levels, 0, "cs")
        assert over is None and np.array_equal(m[0], MK.expected(w, h, 8, levels, 0, "cs"))
    finally:
        b.close()


def test_identical_pair_is_zero_and_inverted_checkerboard_saturates(ce, gpu_ctx):
    rng = np.random.default_rng(3)
    img = rng.integers(0, 1 << 16, (163, 161, 3)).astype(np.uint16)
    for level in (0, 3):
        m, over = gpu_ctx.ms_ssim_map(img, img.copy(), 161, 163, 5, level, "ssim", 1, [0, 1, MK.U32_MAX], depth=16)
        assert not m.any() and not over.any()
    w, h = 43, 27
    a, b = K.checkerboard(w, h)
    n = (w - 10) * (h - 10)
    m, over = gpu_ctx.ms_ssim_map(a, b, w, h, 1, 0, "ssim", 1, [0, R.Q32 // 2, MK.U32_MAX - 1, MK.U32_MAX])
    assert m.shape == (1, 3, h - 10, w - 10) and (m == MK.U32_MAX).all()
    assert over[0].tolist() == [[n, n, n, 0]] * 3
    cells, _ = gpu_ctx.ms_ssim_map(a, b, w, h, 1, 0, "ssim", 64)
    assert cells.shape == (1, 3, 1, 1) and (cells == MK.U32_MAX).all()
    for what in ("ssim", "cs"):
        got = gpu_ctx.ms_ssim_map(a, b, w, h, 1, 0, what, 4)[0]
        assert np.array_equal(got[0], R.cells(R.full_map(a, b, 8, 1, 0, what), 4)), what


def test_pair_table_first_leaves_rgb8_against_deep_and_the_sum_identity(ce, gpu_ctx):
    """Five pairs on three references bound out of order, in slots that are no identity, in a batch that holds more; ranges that
    do not start at pair 0; the RGB8 batch against a deep 8 / 8 batch, bit for bit; both leaves against the batch; and n * 2^32 -
    map.sum() against Batch.ms_ssim's integers on the device."""
    w, h = 176, 163
    refs = [K.pair(w, h, 8, s)[0] for s in range(3)]
    seeds = (1, 0, 2, 2, 0)
    tests = [K.pair(w, h, 8, s)[1] for s in seeds]
    binding = [1, 0, 2, 1, 0]  # pair 3: test of seed 2 against reference of seed 1
    want = lambda p, level, what, block=1: MK.expected(w, h, 8, 5, level, what, block, seeds[p], binding[p])  # noqa: E731
    results = []
    for deep in (False, True):
        b = batch_of(ce, gpu_ctx, w, h, 8, deep, 4, 6)
        try:
            for p in (3, 0, 4, 2, 1):
                b.set_test(p, binding[p], tests[p].astype(np.uint16) if deep else tests[p])
            for i in (2, 0, 1):
                b.set_reference(i, refs[i].astype(np.uint16) if deep else refs[i])
            got = []
            for level, what, block in ((0, "ssim", 1), (2, "cs", 1), (1, "ssim", 32)):
                m, over = b.ms_ssim_maps(0, 5, 5, level, what, block, MK.THR8)
                for p in range(5):
                    assert np.array_equal(m[p], want(p, level, what, block)), (deep, p, level, what, block)
                    assert np.array_equal(over[p], R.over(want(p, level, what), MK.THR8)), (deep, p, level, what)
                part, part_over = b.ms_ssim_maps(2, 3, 5, level, what, block, MK.THR8[:3])  # first > 0: reference 0 is named by pair 4 only
                assert np.array_equal(part, m[2:]) and np.array_equal(part_over, over[2:, :, :3])
                one = b.ms_ssim_maps(3, 1, 5, level, what, block)[0]
                assert np.array_equal(one[0], m[3])
                got.append((m, over))
            if not deep:
                scores = b.ms_ssim(5)
                for level, what, key in ((0, "ssim", "ssim_q"), (2, "cs", "cs_q")):
                    m = b.ms_ssim_maps(0, 5, 5, level, what)[0]
                    held = []
                    for p in range(5):
                        q = MK.level_q(w, h, 8, 5, level, seeds[p], binding[p])[R.WHAT[what]]
                        for c in range(3):
                            if int(q[c].min()) < 1 or int(q[c].max()) > R.Q32:
                                continue  # the identity is stated for maps none of whose values saturates
                            total = sum(int(v) for v in m[p, c].sum(axis=1, dtype=np.uint64))
                            assert scores[p].n[level] * R.Q32 - total == getattr(scores[p], key)[level][c], (p, level, what, c)
                            held.append(p)
                    # pair 3 sets one pattern against another and has positions of negative SSIM; the others are a pattern and its noisy self
                    assert {0, 1, 2, 4} <= set(held)
            results.append(got)
        finally:
            b.close()
    for (m8, o8), (m16, o16) in zip(*results):
        assert np.array_equal(m8, m16) and np.array_equal(o8, o16)
    for level, what, block in ((0, "ssim", 1), (2, "cs", 8)):
        m, over = gpu_ctx.ms_ssim_map(refs[1], tests[3], w, h, 5, level, what, block, MK.THR8)
        assert np.array_equal(m[0], want(3, level, what, block)) and np.array_equal(over[0], R.over(want(3, level, what), MK.THR8))
        m16, over16 = gpu_ctx.ms_ssim_map(refs[1].astype(np.uint16), tests[3].astype(np.uint16), w, h, 5, level, what, block, MK.THR8, depth=8)
        assert np.array_equal(m16, m) and np.array_equal(over16, over)
    r10, t10 = K.pair(192, 256, 10)
    m, _ = gpu_ctx.ms_ssim_map(r10, t10, 192, 256, 5, 2, "ssim", depth=10)
    assert np.array_equal(m[0], MK.expected(192, 256, 10, 5, 2, "ssim"))


def test_a_patch_is_where_the_cell_maxima_say(ce, gpu_ctx):
    w, h, x0, y0 = 171, 171, 100, 60
    ref, test = MK.patched(w, h, x0, y0)
    cells, over = gpu_ctx.ms_ssim_map(ref, test, w, h, 5, 0, "ssim", 16, [0])
    full = R.full_map(ref, test, 8, 5, 0)
    assert np.array_equal(cells[0], R.cells(full, 16)) and np.array_equal(over[0], R.over(full, [0]))
    for c in range(3):
        cy, cx = np.unravel_index(np.argmax(cells[0, c]), cells[0, c].shape)
        assert y0 - 10 < (cy + 1) * 16 and cy * 16 < y0 + 6 and x0 - 10 < (cx + 1) * 16 and cx * 16 < x0 + 6, (c, cy, cx)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_a_launch_and_a_score_call_keep_their_results_across_the_map_call(ce, gpu_ctx):
    w, h = 176, 163
    ref, test = K.pair(w, h, 8)
    cfg = ce.MetricConfig.all()
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference(0, ref)
        b.set_test(0, 0, test)
        scores = b.run(1, cfg, butteraugli_diffmap=True)
        diffmap = b.butteraugli_diffmaps(0, 1).copy()
        ms = b.ms_ssim(1)
        b.launch(1, cfg, butteraugli_diffmap=True)
        m, over = b.ms_ssim_maps(0, 1, 5, 1, "ssim", 1, MK.THR8)
        cells = b.ms_ssim_maps(0, 1, 5, 0, "cs", 64)[0]
        again = b.collect(1)
        key = lambda s: (bits(s.dssim), bits(s.ssimulacra2), bits(s.butteraugli), bits(s.psnr), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in scores] and again[0].valid == 15
        assert np.array_equal(b.butteraugli_diffmaps(0, 1), diffmap)
        assert b.ms_ssim(1) == ms
        K.check_integers(ms[0], K.expected(w, h, 8), "beside the map calls")
        assert np.array_equal(m[0], MK.expected(w, h, 8, 5, 1, "ssim")) and np.array_equal(over[0], MK.expected_over(w, h, 8, 5, 1, "ssim", MK.THR8))
        assert np.array_equal(cells[0], MK.expected(w, h, 8, 5, 0, "cs", 64))
    finally:
        b.close()


def test_every_refusal_leaves_the_batch_usable(ce, gpu_ctx):
    w, h = 176, 163
    ref, test = K.pair(w, h, 8)
    L = ce.lib()
    vw, vh = w - 10, h - 10
    n = 2 * 3 * vw * vh
    buf, thr, over = np.zeros(n + 8, np.uint32), np.array(MK.THR8 + [5], np.uint32), np.zeros(2 * 3 * 9, np.uint64)
    bp, tp, op = buf.ctypes.data, thr.ctypes.data, over.ctypes.data
    b = ce.Batch(gpu_ctx, w, h, 1, 2)
    try:
        b.set_reference(0, ref)
        b.set_test(0, 0, test)
        b.set_test(1, 0, ref)
        before = b.ms_ssim_maps(0, 2, 5, 0, "ssim", 1, MK.THR8)
        assert not before[0][1].any() and not before[1][1].any()
        call = lambda first=0, count=2, levels=5, level=0, what=0, block=1, m=bp, m_len=n, t=tp, k=8, o=op: L.ce_batch_msssim_map(  # noqa: E731
            b._h, first, count, levels, level, what, block, m, m_len, t, k, o)
        assert call() == ce.CE_OK
        refused = {
            "levels 0": call(levels=0), "levels 2": call(levels=2), "levels 6": call(levels=6), "level 5 of 5": call(level=5),
            "level 1 of 1": call(levels=1, level=1), "what 2": call(what=2), "block 0": call(block=0), "block 3": call(block=3),
            "block 128": call(block=128), "map_len short": call(m_len=n - 1), "map_len long": call(m_len=n + 1),
            "map_len of block 1 at block 2": call(block=2), "map without length": call(m_len=0), "length without map": call(m=None),
            "count 0": call(count=0, m_len=0), "count past": call(count=3, m_len=n // 2 * 3), "first past": call(first=2, count=1, m_len=n // 2),
            "first + count past": call(first=1, count=2), "nine thresholds": call(k=9), "over without thresholds": call(t=None, k=0),
            "over with a count of 0": call(k=0), "thresholds without over": call(o=None), "a count without over": call(t=None, o=None),
            "both outputs null": call(m=None, m_len=0, t=None, k=0, o=None),
        }
        assert {k: v for k, v in refused.items() if v != ce.CE_ERR_INVALID_ARG} == {}
        assert gpu_ctx._err() != ""
        assert L.ce_batch_msssim_map(None, 0, 2, 5, 0, 0, 1, bp, n, tp, 8, op) == ce.CE_ERR_INVALID_ARG
        for kw in ({"what": "luminance"}, {"block": 0}, {"block": 3}, {"level": 5}, {"levels": 3}):
            with pytest.raises(ce.CodecEvalError) as e:
                b.ms_ssim_maps(0, 2, **kw)
            assert e.value.status == ce.CE_ERR_INVALID_ARG, kw
        after = b.ms_ssim_maps(0, 2, 5, 0, "ssim", 1, MK.THR8)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
        assert np.array_equal(after[0][0], MK.expected(w, h, 8, 5, 0, "ssim"))
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
                other.ms_ssim_maps(0, 1, levels)
            assert e.value.status == ce.CE_ERR_INVALID_ARG and word in str(e.value), str(e.value)
        r, t = K.pair(160, 200, 8, 0)
        small.set_reference(0, r)
        small.set_test(0, 0, t)
        assert np.array_equal(small.ms_ssim_maps(0, 1, 1)[0][0], R.full_map(r, t, 8, 1, 0))
        assert small.run(1, ce.MetricConfig(psnr=True))[0].valid == ce.METRIC_PSNR
    finally:
        for x in (linear, uneven, small, tiny):
            x.close()
    # the leaves: wrong lengths, null pointers, an empty image, a depth that is none, levels, a size too small
    ctx, rp, tp8, nb = gpu_ctx._h, ref.ctypes.data, test.ctypes.data, ref.nbytes
    one = n // 2
    leaf = lambda r=rp, r_len=nb, t=tp8, t_len=nb, ww=w, hh=h, levels=5, level=0: L.ce_eval_pair_msssim_map(  # noqa: E731
        ctx, r, r_len, t, t_len, ww, hh, levels, level, 0, 1, bp, one, tp, 8, op)
    assert leaf() == ce.CE_OK
    assert leaf(r_len=nb - 3) == ce.CE_ERR_BAD_LENGTH and leaf(t_len=nb + 3) == ce.CE_ERR_BAD_LENGTH
    assert leaf(r=None) == ce.CE_ERR_INVALID_ARG and leaf(t=None) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_msssim_map(None, rp, nb, tp8, nb, w, h, 5, 0, 0, 1, bp, one, tp, 8, op) == ce.CE_ERR_INVALID_ARG
    assert leaf(r_len=0, t_len=0, ww=0) == ce.CE_ERR_INVALID_ARG
    assert leaf(levels=3) == ce.CE_ERR_INVALID_ARG and leaf(level=5) == ce.CE_ERR_INVALID_ARG
    assert leaf(r_len=160 * 170 * 3, t_len=160 * 170 * 3, ww=160, hh=170) == ce.CE_ERR_INVALID_ARG
    assert "160" in gpu_ctx._err()
    r16, t16 = ref.astype(np.uint16), test.astype(np.uint16)
    deep = lambda depth=8, t_len=2 * nb: L.ce_eval_pair_msssim_map_deep(  # noqa: E731
        ctx, r16.ctypes.data, 2 * nb, t16.ctypes.data, t_len, depth, w, h, 5, 0, 0, 1, bp, one, tp, 8, op)
    assert deep(depth=9) == ce.CE_ERR_INVALID_ARG and deep(t_len=nb) == ce.CE_ERR_BAD_LENGTH and deep() == ce.CE_OK
    assert np.array_equal(buf[:one].reshape(3, vh, vw), MK.expected(w, h, 8, 5, 0, "ssim"))
    assert np.array_equal(gpu_ctx.ms_ssim_map(ref, test, w, h)[0][0], MK.expected(w, h, 8, 5, 0, "ssim"))
