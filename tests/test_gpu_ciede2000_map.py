"""The CIEDE2000 maps on the device (ce_batch_ciede2000_map, ce_eval_pair_ciede2000_map, ce_eval_pair_ciede2000_map_deep; DESIGN.md
section 34).  Every value is made of separately rounded IEEE f64 operations and one rint, and everything after it is an integer
maximum or an integer sum, so the device must equal the numpy restatement (tests/ciede2000_map_restatement.py) exactly: every
element of every map of every `what`, every cell at every B, every count - on both load paths, with units of work that span
several rows, straddle row ends and change cell inside a unit, with one and with several blocks a pair and with a grid-stride loop
that goes round, on RGB8 batches and deep ones of equal and unequal depths, through a pair -> reference table that is no identity,
past 65535 pairs, right behind the uploads and beside a launch that is still to be collected.  For what = "de" the map is tied to
the shipped scores: its sum, its maximum and its counts are Batch.ciede2000's integers."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_cases as K  # noqa: E402
import ciede2000_map_restatement as M  # noqa: E402
import extreme_shape_cases as X  # noqa: E402

pytestmark = pytest.mark.gpu

THR = K.THRESHOLDS
# what each shape is for: the scalar path with one lane and cells larger than the image; the wide path with exactly one row a unit
# (RGB8) or half a row (deep); the wide path with w below the unit (a unit spans four rows of 5 x 16 and changes cell inside
# itself at B = 2); the wide path with units that straddle row ends and clipped cells on both edges at every B (72 x 34 = 16 * 153
# pixels); the scalar path with the same clipping; several blocks a pair, ragged
SHAPES = [(1, 1), (3, 1), (4, 1), (5, 3), (16, 8), (5, 16), (72, 34), (70, 37), (333, 251)]
KIND_IDS = lambda k: "rgb8" if k == (0, 0) else "deep%d_%d" % k  # noqa: E731


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


def want_over(want):
    """uint32 [n, h, w] -> uint64 [n, 8]"""
    return np.stack([M.over(m, THR) for m in want])


@pytest.mark.parametrize("kind", K.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("w,h", SHAPES, ids=lambda v: str(v))
def test_maps_cells_and_counts_equal_the_restatement(ce, gpu_ctx, w, h, kind):
    deep = kind != (0, 0)
    assert K.wide(w * h, deep) == ((w, h) in ((16, 8), (5, 16), (72, 34)))
    b = load(ce, gpu_ctx, w, h, kind)
    try:
        for what, name in zip(M.WHATS, M.NAMES):
            want = M.expected(w, h, kind)[..., what]  # [5, h, w]
            counts = want_over(want)
            full, over = b.ciede2000_maps(0, 5, name, 1, THR)  # the first of them right behind the uploads: nothing was synchronised
            assert full.dtype == np.uint32 and full.shape == (5, h, w) and over.dtype == np.uint64 and over.shape == (5, 8)
            bad = np.argwhere(full != want)
            assert bad.size == 0, (name, len(bad), bad[:4].tolist())
            assert np.array_equal(over, counts), name
            assert not full[2].any()  # an image against itself: every pixel skipped (or, at 8 / 16, computed), every element 0
            # the map alone, the counts alone, the integer constant for the name
            only_map = b.ciede2000_maps(0, 5, what)
            assert only_map[1] is None and np.array_equal(only_map[0], want)
            only_counts = b.ciede2000_maps(0, 5, name, 1, THR, maps=False)
            assert only_counts[0] is None and np.array_equal(only_counts[1], counts)
            # cells at every B against the device's own full map and the restatement; the counts stay those of the pixels
            for block in M.BLOCKS:
                cells, over_b = b.ciede2000_maps(0, 5, name, block, THR)
                assert cells.shape == (5, -(-h // block), -(-w // block))
                for p in range(5):
                    assert np.array_equal(cells[p], M.block_max(full[p], block)), (name, block, p)
                    assert np.array_equal(cells[p], M.block_max(want[p], block)), (name, block, p)
                assert np.array_equal(over_b, counts), (name, block)
            # first > 0 with count < n, and fewer thresholds
            part, over_part = b.ciede2000_maps(2, 2, name, 1, THR[2:5])
            assert np.array_equal(part, want[2:4]) and np.array_equal(over_part, counts[2:4, 2:5])
            part, over_part = b.ciede2000_maps(4, 1, name, 4, THR[:1])
            assert np.array_equal(part[0], M.block_max(want[4], 4)) and np.array_equal(over_part, counts[4:5, :1])
            if what == M.DE:  # the tie to the shipped scores
                scores = b.ciede2000(5, THR)
                for p in range(5):
                    assert int(full[p].astype(np.uint64).sum()) == scores[p].sum_q20 and int(full[p].max()) == scores[p].max_q20, p
                    assert tuple(int(v) for v in over[p]) == scores[p].n_above, p
                    assert np.array_equal(full[p].reshape(-1), K.pair_q(w, h, kind, p))
    finally:
        b.close()


@pytest.mark.parametrize("kind", [(0, 0), (16, 16), (12, 16)], ids=KIND_IDS)
def test_more_pixels_than_the_launch_has_lanes(ce, gpu_ctx, kind):
    """512 x 520 with sixteen pairs: 64 blocks a pair on the wide path, fewer lanes than units of 16 (RGB8) or 8 (deep) pixels."""
    w, h = K.BIG
    deep = kind != (0, 0)
    assert K.wide(w * h, deep) and K.blocks(w * h, K.BIG_PAIRS, deep) == 64 and K.goes_round(w * h, K.BIG_PAIRS, deep)
    b = load(ce, gpu_ctx, w, h, kind, K.BIG_PAIRS, 0)
    try:
        scores = b.ciede2000(K.BIG_PAIRS, THR)
        for what, name in zip(M.WHATS, M.NAMES):
            want = M.expected(w, h, kind)[..., what]
            full, over = b.ciede2000_maps(0, K.BIG_PAIRS, name, 1, THR)
            cells, over_b = b.ciede2000_maps(0, K.BIG_PAIRS, name, 8, THR)
            for p in range(K.BIG_PAIRS):
                assert np.array_equal(full[p], want[p % 5]), (name, p)
                assert np.array_equal(cells[p], M.block_max(want[p % 5], 8)), (name, p)
                assert np.array_equal(over[p], M.over(want[p % 5], THR)) and np.array_equal(over_b[p], over[p]), (name, p)
                if what == M.DE:
                    assert (int(full[p].astype(np.uint64).sum()), int(full[p].max()), tuple(int(v) for v in over[p])) == \
                        (scores[p].sum_q20, scores[p].max_q20, scores[p].n_above), p
    finally:
        b.close()


def test_leaves_equal_the_batch_call(ce, gpu_ctx):
    for (w, h), block in (((16, 8), 1), ((5, 16), 2), ((70, 37), 8)):
        for kind in K.KINDS:
            refs, tests = K.images(w, h, kind)
            depths = {} if kind == (0, 0) else {"depth": kind[0], "test_depth": kind[1]}
            b = load(ce, gpu_ctx, w, h, kind)
            try:
                for what, name in zip(M.WHATS, M.NAMES):
                    want_map, want_over_ = b.ciede2000_maps(0, 5, name, block, THR)
                    for p in (0, 1, 3):
                        got, over = gpu_ctx.ciede2000_map(refs[K.BINDING[p]], tests[p], w, h, name, block, THR, **depths)
                        assert got.shape == (1,) + want_map.shape[1:] and np.array_equal(got[0], want_map[p]), (w, h, kind, name, p)
                        assert np.array_equal(over[0], want_over_[p]), (w, h, kind, name, p)
                    got = gpu_ctx.ciede2000_map(refs[1], tests[3], w, h, name, block, THR, maps=False, **depths)
                    assert got[0] is None and np.array_equal(got[1][0], want_over_[3])
            finally:
                b.close()
    # an RGB8 pair and the same codes as a deep 8 / 8 pair
    refs, tests = K.images(333, 251, (0, 0))
    want = M.expected(333, 251, (0, 0))[3]
    for what, name in zip(M.WHATS, M.NAMES):
        assert np.array_equal(gpu_ctx.ciede2000_map(refs[1], tests[3], 333, 251, name)[0][0], want[..., what])
        assert np.array_equal(gpu_ctx.ciede2000_map(refs[1].astype(np.uint16), tests[3].astype(np.uint16), 333, 251, name, depth=8)[0][0],
                              want[..., what])


def test_worked_cases_and_the_host_function(ce, gpu_ctx):
    black, white = np.zeros((3, 5, 3), np.uint8), np.full((3, 5, 3), 255, np.uint8)
    for what, value in zip(M.NAMES, (100 << 20, 100 << 20, 0, 0)):
        m, over = gpu_ctx.ciede2000_map(black, white, 5, 3, what, 1, [(100 << 20) - 1, 100 << 20])
        assert (m == value).all() and over.tolist() == [[15 if value else 0, 0]]
    rng = np.random.default_rng(34)
    for depth in (0, 10, 16):
        img = rng.integers(0, 256 if depth == 0 else 1 << depth, (8, 16, 3)).astype(np.uint8 if depth == 0 else np.uint16)
        for what in M.NAMES:
            m, over = gpu_ctx.ciede2000_map(img, img.copy(), 16, 8, what, 1, [0], depth=depth)
            assert not m.any() and not over.any()
    # the host function and the device, pixel by pixel
    a = np.array(K.ANCHORS, np.uint8)  # [25, 2, 3]
    host = ce.ciede2000_pixel_terms(a[:, 0], a[:, 1])
    for what in M.WHATS:
        got = gpu_ctx.ciede2000_map(a[:, 0].reshape(5, 5, 3), a[:, 1].reshape(5, 5, 3), 5, 5, what)[0]
        assert np.array_equal(got.reshape(-1), host[:, what]), what


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
        before = b.ciede2000(1, THR)
        b.launch(1, cfg, butteraugli_diffmap=True)
        got = {name: b.ciede2000_maps(0, 1, name, 1, THR) for name in M.NAMES}
        cells = b.ciede2000_maps(0, 1, "dh", 16, THR)
        again = b.collect(1)
        key = lambda s: (bits(s.dssim), bits(s.ssimulacra2), bits(s.butteraugli), bits(s.psnr), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in scores] and again[0].valid == 15
        assert np.array_equal(b.butteraugli_diffmaps(0, 1), diffmap)
        assert b.ciede2000(1, THR) == before
        want = M.terms_of_images(refs[1], tests[0], (0, 0))
        for what, name in zip(M.WHATS, M.NAMES):
            assert np.array_equal(got[name][0][0], want[..., what]) and np.array_equal(got[name][1][0], M.over(want[..., what], THR)), name
        assert np.array_equal(cells[0][0], M.block_max(want[..., M.DH], 16))
        assert int(got["de"][0].astype(np.uint64).sum()) == before[0].sum_q20
    finally:
        b.close()


def many_images():
    """Three references and seven tests of 4 x 1, uint8: noise, and the reference p % 3 moved by up to +-3 codes."""
    rng = np.random.default_rng(3465)
    refs = [rng.integers(0, 256, (1, 4, 3)).astype(np.uint8) for _ in range(X.MAX_REFS)]
    tests = [np.clip(refs[j % X.MAX_REFS].astype(np.int64) + rng.integers(-3, 4, (1, 4, 3)), 0, 255).astype(np.uint8) for j in range(X.K_TESTS)]
    return refs, tests


def test_past_65535_pairs(ce, gpu_ctx):
    """65537 pairs of 4 x 1 against three references: two launches, the second of two pairs with first = 65535."""
    n = 65537
    assert n > X.GRID_YZ_MAX
    refs, tests = many_images()
    b = ce.Batch(gpu_ctx, 4, 1, X.MAX_REFS, n)
    try:
        X.fill_many(ce, b, refs, tests, n)
        want = np.stack([M.terms_of_images(refs[p % X.MAX_REFS], tests[p % X.K_TESTS], (0, 0)) for p in range(X.TWINS)])  # [21, 1, 4, 4]
        scores = b.ciede2000(n, THR)
        for what, name in zip(M.WHATS, M.NAMES):
            _, over = b.ciede2000_maps(0, n, name, 1, THR, maps=False)
            X.assert_twins(over, ("counts", name))
            assert np.array_equal(over[:X.TWINS], np.stack([M.over(want[p, ..., what], THR) for p in range(X.TWINS)])), name
            full, over_m = b.ciede2000_maps(0, n, name, 1, THR)  # 65537 * 4 * 4 bytes: about 1 MB
            X.assert_twins(full, ("map", name))
            assert np.array_equal(full[:X.TWINS], want[..., what]) and np.array_equal(over_m, over), name
            cells, _ = b.ciede2000_maps(0, n, name, 2, THR)
            X.assert_twins(cells, ("cells", name))
            assert np.array_equal(cells[:X.TWINS, 0], np.stack([M.block_max(want[p, ..., what], 2)[0] for p in range(X.TWINS)]))
            tail, over_t = b.ciede2000_maps(65530, 7, name, 1, THR)  # a range that ends at the batch's last pair
            assert np.array_equal(tail, full[65530:]) and np.array_equal(over_t, over[65530:])
            if what == M.DE:
                assert [int(v) for v in full.reshape(n, -1).astype(np.uint64).sum(axis=1)] == [s.sum_q20 for s in scores]
                assert [tuple(int(v) for v in row) for row in over] == [s.n_above for s in scores]
    finally:
        b.close()


def test_every_refusal_leaves_the_batch_usable(ce, gpu_ctx):
    w, h = 16, 8
    refs, tests = K.images(w, h, (0, 0))
    L = ce.lib()
    m, cnt = np.zeros(2 * w * h, np.uint32), np.zeros(2 * 8, np.uint64)
    thr = (C.c_uint32 * 9)(*range(9))
    mp, cp = m.ctypes.data, cnt.ctypes.data
    b = ce.Batch(gpu_ctx, w, h, 1, 2)
    try:
        b.set_reference(0, refs[0])
        b.set_test(0, 0, tests[1])
        b.set_test(1, 0, tests[4])
        good_map, good_over = b.ciede2000_maps(0, 2, "dh", 1, THR)
        cells8 = 2 * 1 * 2
        refusals = [
            ((b._h, 0, 2, 4, 1, mp, m.size, thr, 8, cp), "what above 3"),
            ((b._h, 0, 2, 0, 0, mp, m.size, thr, 8, cp), "block 0"),
            ((b._h, 0, 2, 0, 3, mp, m.size, thr, 8, cp), "block 3"),
            ((b._h, 0, 2, 0, 128, mp, m.size, thr, 8, cp), "block 128"),
            ((b._h, 0, 2, 0, 1, mp, m.size - 1, thr, 8, cp), "a short map_len"),
            ((b._h, 0, 2, 0, 8, mp, m.size, thr, 8, cp), "the full map's length for cells"),
            ((b._h, 0, 2, 0, 1, None, m.size, thr, 8, cp), "no map with a map_len"),
            ((b._h, 0, 2, 0, 1, None, 0, None, 0, None), "both outputs NULL"),
            ((b._h, 0, 0, 0, 1, mp, 0, thr, 8, cp), "count 0"),
            ((b._h, 1, 2, 0, 1, mp, m.size, thr, 8, cp), "a range past max_pairs"),
            ((b._h, 3, 1, 0, 1, mp, w * h, thr, 8, cp), "first past max_pairs"),
            ((b._h, 0, 2, 0, 1, mp, m.size, thr, 9, cp), "nine thresholds"),
            ((b._h, 0, 2, 0, 1, mp, m.size, None, 0, cp), "over without thresholds"),
            ((b._h, 0, 2, 0, 1, mp, m.size, thr, 0, cp), "over with a threshold pointer and n = 0"),
            ((b._h, 0, 2, 0, 1, mp, m.size, thr, 8, None), "thresholds without over"),
        ]
        for args, why in refusals:
            assert L.ce_batch_ciede2000_map(*args) == ce.CE_ERR_INVALID_ARG, why
            assert gpu_ctx._err() != "", why
            got = b.ciede2000_maps(0, 2, "dh", 1, THR)
            assert np.array_equal(got[0], good_map) and np.array_equal(got[1], good_over), why
        assert L.ce_batch_ciede2000_map(None, 0, 2, 0, 1, mp, m.size, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
        assert L.ce_batch_ciede2000_map(b._h, 0, 2, 3, 8, mp, cells8, thr, 8, cp) == ce.CE_OK  # eight thresholds and what = 3 are allowed
        with pytest.raises(ce.CodecEvalError):
            b.ciede2000_maps(0, 2, "dz")
        assert b.run(2, ce.MetricConfig(psnr=True))[0].valid == ce.METRIC_PSNR
    finally:
        b.close()
    linear = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        with pytest.raises(ce.CodecEvalError) as e:
            linear.ciede2000_maps(0, 1)
        assert e.value.status == ce.CE_ERR_INVALID_ARG and "ce_batch_delta_e_itp_map" in str(e.value)
        lin = np.full((h, w, 3), 0.5, np.float32)
        linear.set_reference(0, lin)
        linear.set_test(0, 0, lin)
        assert not linear.delta_e_itp_maps(0, 1)[0].any()
    finally:
        linear.close()
    # the leaves: wrong lengths, null pointers, an empty image, depths that are none, and what the batch call refuses
    ref, test = refs[0], tests[1]
    ctx, rp, tp, n = gpu_ctx._h, ref.ctypes.data, test.ctypes.data, ref.nbytes
    leaf = L.ce_eval_pair_ciede2000_map
    one = w * h
    assert leaf(ctx, rp, n - 3, tp, n, w, h, 0, 1, mp, one, thr, 8, cp) == ce.CE_ERR_BAD_LENGTH
    assert leaf(ctx, rp, n, tp, n + 3, w, h, 0, 1, mp, one, thr, 8, cp) == ce.CE_ERR_BAD_LENGTH
    assert leaf(ctx, None, n, tp, n, w, h, 0, 1, mp, one, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
    assert leaf(ctx, rp, n, None, n, w, h, 0, 1, mp, one, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
    assert leaf(None, rp, n, tp, n, w, h, 0, 1, mp, one, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
    assert leaf(ctx, rp, 0, tp, 0, 0, h, 0, 1, mp, 0, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
    assert leaf(ctx, rp, n, tp, n, w, h, 4, 1, mp, one, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
    assert leaf(ctx, rp, n, tp, n, w, h, 0, 5, mp, one, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
    assert leaf(ctx, rp, n, tp, n, w, h, 0, 1, mp, one + 1, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
    assert leaf(ctx, rp, n, tp, n, w, h, 0, 1, None, 0, None, 0, None) == ce.CE_ERR_INVALID_ARG
    assert leaf(ctx, rp, n, tp, n, w, h, 0, 1, mp, one, thr, 9, cp) == ce.CE_ERR_INVALID_ARG
    r16, t16 = ref.astype(np.uint16), test.astype(np.uint16)
    deep_leaf = L.ce_eval_pair_ciede2000_map_deep
    for dr, dt in ((9, 8), (8, 14), (0, 8)):
        assert deep_leaf(ctx, r16.ctypes.data, 2 * n, t16.ctypes.data, 2 * n, dr, dt, w, h, 0, 1, mp, one, thr, 8, cp) == ce.CE_ERR_INVALID_ARG
        assert "depths" in gpu_ctx._err()
    assert deep_leaf(ctx, r16.ctypes.data, 2 * n, t16.ctypes.data, n, 8, 8, w, h, 0, 1, mp, one, thr, 8, cp) == ce.CE_ERR_BAD_LENGTH
    got = gpu_ctx.ciede2000_map(ref, test, w, h, "dc", 1, THR)
    want = M.expected(w, h, (0, 0))[1][..., M.DC]
    assert np.array_equal(got[0][0], want) and np.array_equal(got[1][0], M.over(want, THR))
