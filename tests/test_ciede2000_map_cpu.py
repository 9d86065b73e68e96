"""The CIEDE2000 maps without a device (include/ce_metrics.h: ce_batch_ciede2000_map, ce_ciede2000_pixel_terms; DESIGN.md section
34): the numpy restatement (tests/ciede2000_map_restatement.py) against ciede2000_restatement.q20, against cases worked out by
hand and against a plain loop for the cells and counts, and ce_ciede2000_pixel_terms - the kernel's pixel text compiled for the
host - against the restatement on every integer."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_cases as K  # noqa: E402
import ciede2000_map_restatement as M  # noqa: E402
import ciede2000_restatement as R  # noqa: E402
import test_ciede2000_cpu as T  # noqa: E402  (host_inputs: the content ce_ciede2000_pixels is held to)

Q = 1 << 20


@pytest.fixture(scope="module", autouse=True)
def tables(ce):
    K.use(ce)
    return K.TABLES


def extra_inputs():
    """Noise at every depth and at unequal depths beyond host_inputs' - (name, reference [n, 3], depth, test [n, 3], depth)."""
    rng = np.random.default_rng(3400)
    for dr, dt in ((8, 8), (10, 10), (12, 12), (16, 16), (8, 16), (16, 10), (12, 8)):
        r = rng.integers(0, 1 << dr, (20000, 3))
        yield f"noise at {dr} / {dt}", r, dr, rng.integers(0, 1 << dt, (20000, 3)), dt
        if dr == dt:
            yield f"noise moved by +-3 codes at {dr}", r, dr, np.clip(r + rng.integers(-3, 4, r.shape), 0, (1 << dr) - 1), dt


def test_host_function_equals_the_restatement_on_every_value(ce, tables):
    names = []
    for name, r, dr, t, dt in list(T.host_inputs()) + list(extra_inputs()):
        got = ce.ciede2000_pixel_terms(r, t, dr, dt)
        want = M.terms(r, dr, tables[dr], t, dt, tables[dt])
        assert got.dtype == np.uint32 and got.shape == (len(r), 4)
        assert np.array_equal(got, want), (name, [int(np.abs(got[:, k].astype(np.int64) - want[:, k]).max()) for k in M.WHATS])
        # the DE column is the very q of the scores: the restatement's own, the score restatement's and the host function's
        assert np.array_equal(want[:, M.DE], R.q20(r, dr, tables[dr], t, dt, tables[dt])), name
        assert np.array_equal(got[:, M.DE], ce.ciede2000_pixels(r, t, dr, dt)), name
        names.append(name)
    assert "all grey pairs" in names and any("lattice" in n for n in names) and sum("switch" in n for n in names) == 4


def test_de_of_the_restatement_is_the_score_restatement_on_the_shared_cases(tables):
    for kind in K.KINDS:
        for w, h in ((5, 3), (16, 8)):
            want = M.expected(w, h, kind)
            for p in range(5):
                assert np.array_equal(want[p, :, :, M.DE].reshape(-1), K.pair_q(w, h, kind, p)), (kind, w, h, p)


def test_worked_cases(ce, tables):
    black, white = np.array([[0, 0, 0]]), np.array([[255, 255, 255]])
    for a, b in ((black, white), (white, black)):
        for dr, dt, sa, sb in ((8, 8, 1, 1), (16, 16, 257, 257), (8, 16, 1, 257)):
            want = [[100 * Q, 100 * Q, 0, 0]]
            assert ce.ciede2000_pixel_terms(a * sa, b * sb, dr, dt).tolist() == want
            assert M.terms(a * sa, dr, tables[dr], b * sb, dt, tables[dt]).tolist() == want
    # identical triples, and 8-bit v against 16-bit 257 v, which read the same table values: four zeros
    rng = np.random.default_rng(3401)
    for d in K.DEPTHS:
        v = rng.integers(0, 1 << d, (5000, 3))
        assert not ce.ciede2000_pixel_terms(v, v, d, d).any() and not M.terms(v, d, tables[d], v, d, tables[d]).any()
    v = np.concatenate([rng.integers(0, 256, (5000, 3)), np.array(K.ANCHORS)[:, 0]])
    assert not ce.ciede2000_pixel_terms(v, 257 * v, 8, 16).any() and not M.terms(v, 8, tables[8], 257 * v, 16, tables[16]).any()
    # a pure lightness step between greys: no chroma and no hue term, and dE is the lightness term
    g = ce.ciede2000_pixel_terms([[64, 64, 64]], [[200, 200, 200]])[0]
    assert g[M.DC] == 0 and g[M.DH] == 0 and g[M.DE] == g[M.DL] > 0


def test_swapping_the_sides_changes_no_value(ce, tables):
    rng = np.random.default_rng(3402)
    r, t = rng.integers(0, 256, (50000, 3)), rng.integers(0, 256, (50000, 3))
    near = np.clip(r + rng.integers(-3, 4, r.shape), 0, 255)
    for a, b in ((r, t), (r[:25000], near[:25000])):
        fwd, back = ce.ciede2000_pixel_terms(a, b), ce.ciede2000_pixel_terms(b, a)
        assert np.array_equal(fwd, back), np.nonzero((fwd != back).any(axis=1))[0][:5]
        assert np.array_equal(M.terms(a, 8, tables[8], b, 8, tables[8]), M.terms(b, 8, tables[8], a, 8, tables[8]))


def test_ranges_need_no_saturation_and_terms_may_exceed_de(ce, tables):
    rng = np.random.default_rng(2000)  # test_ciede2000_cpu.fixed_seed_sets' first set, and every pair of cube corners
    n = 400000
    r, t = rng.integers(0, 256, (n, 3)), rng.integers(0, 256, (n, 3))
    corners = np.array([[255 * ((i >> 2) & 1), 255 * ((i >> 1) & 1), 255 * (i & 1)] for i in range(8)])
    r = np.concatenate([r, np.repeat(corners, 8, 0)])
    t = np.concatenate([t, np.tile(corners, (8, 1))])
    v = ce.ciede2000_pixel_terms(r, t)
    assert int(v.max()) < 1 << 27
    top = v.max(axis=0) / Q
    print("largest dE, |tl|, |tc|, |th|:", top)  # include/ce_metrics.h states them for this set: 115.37, 100, 33.36, 109.56
    # L runs from 0 to 100 and S_L >= 1, so black against white - among the corners - is the largest lightness term there is
    assert top[M.DL] == 100.0
    # moved by up to +-3 codes the rotation term takes more than a little: a term above its dE is a fact of the formula, which
    # neither the header promises away nor any test may assert away
    near = np.clip(r + rng.integers(-3, 4, r.shape), 0, 255)
    v = ce.ciede2000_pixel_terms(r, near)
    assert int(v.max()) < 1 << 27
    above = int((v[:, M.DC] > v[:, M.DE]).sum()), int((v[:, M.DH] > v[:, M.DE]).sum())
    print("pairs within +-3 codes with |tc| > dE, |th| > dE:", above)
    assert above[0] > 0 and above[1] > 0


def test_the_shared_cases_hold_a_term_above_its_de(tables):
    """A condition on the content the device tests run: at least one pixel's chroma or hue term exceeds its dE."""
    found = 0
    for kind in K.KINDS:
        v = M.expected(16, 8, kind).reshape(-1, 4).astype(np.int64)
        found += int(((v[:, M.DC] > v[:, M.DE]) | (v[:, M.DH] > v[:, M.DE])).sum())
    v = M.expected(333, 251, (0, 0)).reshape(-1, 4).astype(np.int64)
    found += int(((v[:, M.DC] > v[:, M.DE]) | (v[:, M.DH] > v[:, M.DE])).sum())
    assert found > 0


def test_cells_and_counts_against_a_plain_loop():
    rng = np.random.default_rng(3403)
    m = rng.integers(0, 1 << 27, (3, 5), dtype=np.uint32)  # 5 x 3: h = 3, w = 5
    for block in (2, 4):
        ch, cw = -(-3 // block), -(-5 // block)
        want = np.zeros((ch, cw), np.uint32)
        for y in range(3):
            for x in range(5):
                want[y // block, x // block] = max(want[y // block, x // block], m[y, x])
        got = M.block_max(m, block)
        assert got.shape == (ch, cw) and got.dtype == np.uint32 and np.array_equal(got, want)
    assert M.block_max(m, 64).shape == (1, 1) and M.block_max(m, 64)[0, 0] == m.max()
    thr = [0, int(m.min()), int(np.sort(m.reshape(-1))[7]), int(m.max()), (1 << 32) - 1]
    want = [sum(1 for v in m.reshape(-1) if int(v) > t) for t in thr]
    assert M.over(m, thr).tolist() == want and want[0] == 15 - int((m == 0).sum()) and want[3] == 0 and want[4] == 0


def test_abi_and_refusals_without_a_device(ce):
    L = ce.lib()
    for name in ("ce_batch_ciede2000_map", "ce_eval_pair_ciede2000_map", "ce_eval_pair_ciede2000_map_deep", "ce_ciede2000_pixel_terms"):
        assert name in ce.ABI_SYMBOLS and hasattr(L, name)
    assert (ce.CIEDE2000_MAP_DE, ce.CIEDE2000_MAP_DL, ce.CIEDE2000_MAP_DC, ce.CIEDE2000_MAP_DH) == M.WHATS
    assert callable(ce.Batch.ciede2000_maps) and callable(ce.Context.ciede2000_map)
    rgb, out = np.zeros(6, np.uint16), np.ones(8, np.uint32)
    for dr, dt in ((9, 8), (8, 0), (16, 17)):
        assert L.ce_ciede2000_pixel_terms(rgb.ctypes.data, dr, rgb.ctypes.data, dt, 2, out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ciede2000_pixel_terms(None, 8, rgb.ctypes.data, 8, 2, out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ciede2000_pixel_terms(rgb.ctypes.data, 8, None, 8, 2, out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ciede2000_pixel_terms(rgb.ctypes.data, 8, rgb.ctypes.data, 8, 2, None) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ciede2000_pixel_terms(rgb.ctypes.data, 8, rgb.ctypes.data, 8, 2, out.ctypes.data) == ce.CE_OK and not out.any()
    with pytest.raises(ValueError):
        ce.ciede2000_pixel_terms(np.zeros(6), np.zeros(9))
    # a null batch and a null context are refused before any device is touched
    m, thr, cnt = np.zeros(4, np.uint32), np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    img = np.zeros(12, np.uint8)
    assert L.ce_batch_ciede2000_map(None, 0, 1, 0, 1, m.ctypes.data, 4, thr.ctypes.data, 1, cnt.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert b"null batch" in L.ce_last_error(None)
    assert L.ce_eval_pair_ciede2000_map(None, img.ctypes.data, 12, img.ctypes.data, 12, 2, 2, 0, 1, m.ctypes.data, 4, thr.ctypes.data, 1,
                                        cnt.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_ciede2000_map_deep(None, img.ctypes.data, 24, img.ctypes.data, 24, 8, 8, 2, 2, 0, 1, m.ctypes.data, 4, thr.ctypes.data,
                                             1, cnt.ctypes.data) == ce.CE_ERR_INVALID_ARG
