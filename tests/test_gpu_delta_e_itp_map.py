"""The Delta E ITP maps on the device (ce_batch_delta_e_itp_map, ce_eval_pair_delta_e_itp_map).  The
definition is integers and correctly rounded IEEE operations, so the device must equal the numpy restatement
(tests/delta_e_itp_map_restatement.py) exactly: every pixel of every pair on both load paths, with one and with several blocks a
pair, through the pair -> reference table; the cell maxima against the device's own full map; the exceedance counts with the
map, with the cells and alone; the sum and the maximum of a map against the shipped scores of the same batch; saturation where
k needs 33 bits; the leaf against the batch; and every refusal, with the batch usable afterwards."""
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_e_itp_map_restatement as M  # noqa: E402
import hdr_fidelity_cases as K  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["%dx%d" % c[:2] for c in K.shape_cases()]
THR = list(M.THRESHOLDS)


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def load(ctx, w, h, pairs):
    """The pairs as one linear batch, a reference slot per distinct reference array."""
    refs = []
    for _, ref, _ in pairs:
        if not any(r is ref for r in refs):
            refs.append(ref)
    b = ctx.batch_linear(w, h, len(refs), len(pairs))
    for i, r in enumerate(refs):
        b.set_reference(i, r)
    for p, (_, ref, test) in enumerate(pairs):
        b.set_test(p, next(i for i, r in enumerate(refs) if r is ref), test)
    return b


def clipped_case():
    """70 x 37: cells clipped on both edges at every B, B = 64 taller than the image and wider than one cell row; the scalar
    path (2590 pixels).  Three pairs, two of them on one reference."""
    w, h = 70, 37
    r0, t0 = K.pq_linear(w, h, 12, 203.0, 51)
    _, t1 = K.pq_linear(w, h, 12, 203.0, 51, noise=3)
    r2, t2 = K.pq_linear(w, h, 10, 80.0, 52, noise=200)
    return w, h, K.PARAMS[0], [("pq", r0, t0), ("pq_fine", r0, t1), ("pq_coarse", r2, t2)]


@pytest.mark.parametrize("shape_index", range(len(K.shape_cases())), ids=SHAPE_IDS)
def test_full_map_and_counts_equal_restatement_and_tie_to_the_scores(ce, gpu_ctx, shape_index):
    w, h, params, pairs = K.shape_cases()[shape_index]
    n = len(pairs)
    b = load(gpu_ctx, w, h, pairs)
    try:
        if (w, h) == (512, 256):  # 17 pairs bound to 4 shared reference slots
            assert n == 17 and len({b.pair_reference(p) for p in range(n)}) == 4
        for depth, white in params:
            maps, over = b.delta_e_itp_maps(0, n, depth, white, 1, THR)
            assert maps.dtype == np.uint32 and maps.shape == (n, h, w) and over.dtype == np.uint64 and over.shape == (n, 4)
            want = M.expected_maps(shape_index, depth, white)
            scores, restated = b.hdr_fidelity(n, depth, white), K.expected(shape_index, depth, white)
            tied = 0
            for p, (name, _, _) in enumerate(pairs):
                what = (w, h, depth, white, p, name)
                assert np.array_equal(maps[p], want[p]), what
                assert np.array_equal(over[p], M.over(want[p], THR)), what
                if restated[p]["itp_max_q20"] < (1 << 32):
                    assert int(maps[p].astype(np.uint64).sum()) == scores[p].itp_sum_q20 and int(maps[p].max()) == scores[p].itp_max_q20, what
                    tied += 1
            assert tied > 0 and maps.any()
            only_counts = b.delta_e_itp_maps(0, n, depth, white, 1, THR, maps=False)
            assert only_counts[0] is None and np.array_equal(only_counts[1], over)
            only_maps = b.delta_e_itp_maps(0, n, depth, white, 1)
            assert only_maps[1] is None and np.array_equal(only_maps[0], maps)
    finally:
        b.close()


@pytest.mark.parametrize("case", list(range(len(K.shape_cases()))) + ["70x37"], ids=SHAPE_IDS + ["70x37"])
def test_cell_maxima_slices_and_counts_whatever_the_block(ce, gpu_ctx, case):
    w, h, params, pairs = clipped_case() if case == "70x37" else K.shape_cases()[case]
    n = len(pairs)
    b = load(gpu_ctx, w, h, pairs)
    try:
        for depth, white in params:
            full, over = b.delta_e_itp_maps(0, n, depth, white, 1, THR)
            if case == "70x37":
                for p, (_, ref, test) in enumerate(pairs):
                    assert np.array_equal(full[p], M.full_map(ref, test, depth, white)), p
            first, count = (n // 2, n - n // 2 - 1) if n >= 3 else (0, n)  # first > 0 and first + count < n where there are pairs for it
            for block in (2, 8, 64):
                cells, over_b = b.delta_e_itp_maps(0, n, depth, white, block, THR)
                assert cells.dtype == np.uint32 and cells.shape == (n, -(-h // block), -(-w // block))
                for p in range(n):
                    assert np.array_equal(cells[p], M.block_max(full[p], block)), (depth, white, block, p)
                assert np.array_equal(over_b, over), block
                part, over_part = b.delta_e_itp_maps(first, count, depth, white, block, THR)
                assert np.array_equal(part, cells[first:first + count]) and np.array_equal(over_part, over[first:first + count]), block
            part, over_part = b.delta_e_itp_maps(first, count, depth, white, 1, THR[:2])
            assert np.array_equal(part, full[first:first + count]) and np.array_equal(over_part, over[first:first + count, :2])
            assert full.any()
        if case == "70x37":
            assert b.delta_e_itp_maps(0, n, depth, white, 8)[0].shape == (n, 5, 9) and b.delta_e_itp_maps(0, n, depth, white, 64)[0].shape == (n, 1, 2)
    finally:
        b.close()


def test_saturation_pair(ce, gpu_ctx):
    """5 x 3 with the pixel whose k needs 33 bits: the map saturates, the score does not."""
    w, h, depth, white = 5, 3, 10, 80.0
    ref, test = (a.copy() for a in K.pq_linear(w, h, 10, white, 61))
    ref[1, 2], test[1, 2] = M.saturating_pixels(white)
    want = M.full_map(ref, test, depth, white)
    assert int(want[1, 2]) == M.U32_MAX and int((want == M.U32_MAX).sum()) == 1
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        b.set_reference(0, ref)
        b.set_test(0, 0, test)
        maps, over = b.delta_e_itp_maps(0, 1, depth, white, 1, [M.U32_MAX, M.U32_MAX - 1])
        score = b.hdr_fidelity(1, depth, white)[0]
        cells = b.delta_e_itp_maps(0, 1, depth, white, 4)[0]
    finally:
        b.close()
    assert np.array_equal(maps[0], want) and over.tolist() == [[0, 1]]
    assert score.itp_max_q20 == F.fidelity(ref, test, depth, white)["itp_max_q20"] == 6861206437 > (1 << 32)
    assert np.array_equal(cells[0], M.block_max(want, 4)) and int(cells.max()) == M.U32_MAX


@pytest.mark.parametrize("shape_index", (1, 2, 3), ids=[SHAPE_IDS[i] for i in (1, 2, 3)])
def test_leaf_equals_batch(ce, gpu_ctx, shape_index):
    w, h, params, pairs = K.shape_cases()[shape_index]
    depth, white = params[1]
    want = M.expected_maps(shape_index, depth, white)
    p = len(pairs) - 1
    maps, over = gpu_ctx.delta_e_itp_map(pairs[p][1], pairs[p][2], w, h, depth, white, 1, THR)
    assert maps.shape == (1, h, w) and np.array_equal(maps[0], want[p]) and np.array_equal(over[0], M.over(want[p], THR))
    cells, over8 = gpu_ctx.delta_e_itp_map(pairs[p][1], pairs[p][2], w, h, depth, white, 8, THR)
    assert np.array_equal(cells[0], M.block_max(want[p], 8)) and np.array_equal(over8, over)
    assert np.array_equal(gpu_ctx.delta_e_itp_map(pairs[0][1], pairs[0][2], w, h, depth, white, maps=False, thresholds_q20=THR)[1][0],
                          M.over(want[0], THR))
    # the ingest of a linear image applies: NaN -> 0, the clamp to +-1024
    ref = pairs[p][1].copy()
    ref[0, 0] = (np.nan, 5000.0, -5000.0)
    clean = ref.copy()
    clean[0, 0] = (0.0, 1024.0, -1024.0)
    assert np.array_equal(gpu_ctx.delta_e_itp_map(ref, pairs[p][2], w, h, depth, white)[0], gpu_ctx.delta_e_itp_map(clean, pairs[p][2], w, h, depth, white)[0])


def test_nothing_else_is_disturbed(ce, gpu_ctx):
    w, h, params, pairs = K.shape_cases()[3]  # 96 x 64
    depth, white = params[0]
    pairs = pairs[:3]
    b = load(gpu_ctx, w, h, pairs)
    try:
        config = ce.MetricConfig(dssim=True)
        plain = b.run(3, config)
        before = b.hdr_fidelity(3, depth, white)
        b.launch(3, config)
        maps, over = b.delta_e_itp_maps(0, 3, depth, white, 1, THR)
        again = b.collect(3)
        key = lambda s: (bits(s.dssim), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in plain] and all(s.valid == config.mask for s in again)
        assert b.hdr_fidelity(3, depth, white) == before
        # a new test image reaches the next call
        other = pairs[2][2]
        assert not np.array_equal(other, pairs[0][2])
        b.set_test(0, b.pair_reference(0), other)
        maps2, over2 = b.delta_e_itp_maps(0, 3, depth, white, 1, THR)
        want0 = M.full_map(pairs[0][1], other, depth, white)
        assert np.array_equal(maps2[0], want0) and not np.array_equal(maps2[0], maps[0]) and np.array_equal(over2[0], M.over(want0, THR))
        assert np.array_equal(maps2[1:], maps[1:]) and np.array_equal(over2[1:], over[1:])
    finally:
        b.close()


def test_refusals_leave_the_batch_usable(ce, gpu_ctx):
    w, h, params, pairs = K.shape_cases()[2]  # 97 x 35
    depth, white = params[0]
    b = load(gpu_ctx, w, h, pairs[:2])
    L = ce.lib()
    try:
        good_map, good_over = b.delta_e_itp_maps(0, 2, depth, white, 1, THR)
        m = np.zeros(2 * h * w, np.uint32)
        thr = np.array(THR + [7] * 5, np.uint32)
        cnt = np.zeros(2 * 9, np.uint64)
        mp, tp, cp = m.ctypes.data, thr.ctypes.data, cnt.ctypes.data
        cells8 = 2 * -(-h // 8) * -(-w // 8)

        def ok():
            got = b.delta_e_itp_maps(0, 2, depth, white, 1, THR)
            assert np.array_equal(got[0], good_map) and np.array_equal(got[1], good_over)

        refused = {
            "depth 8": (b._h, 0, 2, 8, white, 1, mp, m.size, tp, 4, cp),
            "depth 14": (b._h, 0, 2, 14, white, 1, mp, m.size, tp, 4, cp),
            "white 0": (b._h, 0, 2, depth, 0.0, 1, mp, m.size, tp, 4, cp),
            "white < 0": (b._h, 0, 2, depth, -203.0, 1, mp, m.size, tp, 4, cp),
            "white inf": (b._h, 0, 2, depth, math.inf, 1, mp, m.size, tp, 4, cp),
            "white nan": (b._h, 0, 2, depth, math.nan, 1, mp, m.size, tp, 4, cp),
            "both outputs null": (b._h, 0, 2, depth, white, 1, None, 0, None, 0, None),
            "count 0": (b._h, 0, 0, depth, white, 1, mp, 0, tp, 4, cp),
            "range past max_pairs": (b._h, 1, 2, depth, white, 1, mp, m.size, tp, 4, cp),
            "first past max_pairs": (b._h, 3, 1, depth, white, 1, mp, h * w, tp, 4, cp),
            "block 0": (b._h, 0, 2, depth, white, 0, mp, m.size, tp, 4, cp),
            "block 3": (b._h, 0, 2, depth, white, 3, mp, m.size, tp, 4, cp),
            "block 128": (b._h, 0, 2, depth, white, 128, mp, 2, tp, 4, cp),
            "map_len short": (b._h, 0, 2, depth, white, 1, mp, m.size - 1, tp, 4, cp),
            "map_len of another block": (b._h, 0, 2, depth, white, 8, mp, m.size, tp, 4, cp),
            "map_len without a map": (b._h, 0, 2, depth, white, 1, None, m.size, tp, 4, cp),
            "map with map_len 0": (b._h, 0, 2, depth, white, 1, mp, 0, tp, 4, cp),
            "nine thresholds": (b._h, 0, 2, depth, white, 1, mp, m.size, tp, 9, cp),
            "over without a count of thresholds": (b._h, 0, 2, depth, white, 1, mp, m.size, tp, 0, cp),
            "over without thresholds": (b._h, 0, 2, depth, white, 1, mp, m.size, None, 4, cp),
            "thresholds without over": (b._h, 0, 2, depth, white, 1, mp, m.size, tp, 4, None),
        }
        for why, args in refused.items():
            assert L.ce_batch_delta_e_itp_map(*args) == ce.CE_ERR_INVALID_ARG, why
            assert gpu_ctx._err() != "", why
            ok()
        assert L.ce_batch_delta_e_itp_map(None, 0, 2, depth, white, 1, mp, m.size, tp, 4, cp) == ce.CE_ERR_INVALID_ARG
        ok()
        assert L.ce_batch_delta_e_itp_map(b._h, 0, 2, depth, white, 8, mp, cells8, tp, 8, cp) == ce.CE_OK  # eight thresholds are allowed
        # a batch that is not linear
        plain = ce.Batch(gpu_ctx, w, h, 1, 1)
        deep = gpu_ctx.batch_deep(w, h, 1, 1, 10, 10)
        try:
            for other in (plain, deep):
                with pytest.raises(ce.CodecEvalError) as e:
                    other.delta_e_itp_maps(0, 1, depth, white)
                assert e.value.status == ce.CE_ERR_INVALID_ARG and "linear" in str(e.value)
                ok()
        finally:
            plain.close()
            deep.close()
        # the leaf: wrong lengths in ce_eval_pair_hdr_fidelity's order, null images, an empty image, a parameter, an output
        r, t = pairs[0][1], pairs[0][2]
        rp, tpx, one = r.ctypes.data, t.ctypes.data, h * w
        leaf = L.ce_eval_pair_delta_e_itp_map
        assert leaf(gpu_ctx._h, rp, r.nbytes - 4, tpx, t.nbytes, w, h, depth, white, 1, mp, one, tp, 4, cp) == ce.CE_ERR_BAD_LENGTH
        assert leaf(gpu_ctx._h, rp, r.nbytes, tpx, t.nbytes + 12, w, h, depth, white, 1, mp, one, tp, 4, cp) == ce.CE_ERR_BAD_LENGTH
        assert leaf(gpu_ctx._h, rp, r.nbytes - 4, tpx, t.nbytes, w, h, 11, white, 1, mp, one, tp, 4, cp) == ce.CE_ERR_INVALID_ARG  # the depth first
        assert leaf(gpu_ctx._h, None, r.nbytes, tpx, t.nbytes, w, h, depth, white, 1, mp, one, tp, 4, cp) == ce.CE_ERR_INVALID_ARG
        assert leaf(gpu_ctx._h, rp, r.nbytes, tpx, t.nbytes, 0, h, depth, white, 1, mp, one, tp, 4, cp) == ce.CE_ERR_INVALID_ARG
        assert leaf(gpu_ctx._h, rp, r.nbytes, tpx, t.nbytes, w, h, depth, white, 3, mp, one, tp, 4, cp) == ce.CE_ERR_INVALID_ARG
        assert leaf(gpu_ctx._h, rp, r.nbytes, tpx, t.nbytes, w, h, depth, white, 1, None, 0, None, 0, None) == ce.CE_ERR_INVALID_ARG
        got = gpu_ctx.delta_e_itp_map(r, t, w, h, depth, white, 1, THR)
        assert np.array_equal(got[0][0], good_map[0]) and np.array_equal(got[1][0], good_over[0])
        ok()
    finally:
        b.close()
