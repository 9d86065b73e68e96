"""Butteraugli diffmaps on the device (CE_FLAG_BUTTERAUGLI_DIFFMAP, ButteraugliResult.diffmap of src/metrics/prelude.rs:64-65):
the stored map is the oracle's map bit for bit with the two device switches on, storing it changes no score, the block
readouts are exact block maxima, and every readout path returns the maps of the launch it names."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ba_diffmap_shim as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.Shim(tmp_path_factory.mktemp("ba_shim"))


def _one_pair(ce, ctx, ref, t, w, h, diffmap=True, it=80.0):
    b = ce.Batch(ctx, w, h, 1, 1)
    b.set_reference(0, ref)
    b.set_test(0, 0, t)
    s = b.run(1, ce.MetricConfig(butteraugli=True), it, butteraugli_diffmap=diffmap)
    assert s[0].status == 0
    out = (s[0].butteraugli, float(b.butteraugli_pnorm3(1)[0]), b.butteraugli_diffmaps(0, 1)[0] if diffmap else None)
    b.close()
    return out


def _parity_cases(workloads):
    cases = []
    for (w, h, seed, q) in ((64, 33, 1, 40), (129, 65, 2, 75), (200, 136, 3, 90), (768, 512, 4, 85), (9, 301, 6, 50)):
        ref = workloads.make_reference(w, h, 900 + seed)
        cases.append((w, h, ref, workloads.distort(ref, q, seed % 2 == 0)))
    flat = workloads.make_reference(96, 96, 5, "flat")
    noisy = np.clip(flat.astype(np.int16) + np.random.default_rng(5).integers(-3, 4, flat.shape), 0, 255).astype(np.uint8)
    cases.append((96, 96, flat, noisy))
    return cases


def test_device_map_is_the_oracle_map_bit_for_bit(gpu_ctx, ce, workloads, shim):
    """The same shapes as test_device_is_the_oracle_with_two_named_switches_bit_for_bit, plus 9 x 301 (one level only):
    with ba_malta_f32 + ba_l2_early on, every pixel of the device's map equals the oracle's; max(map) is the score and the
    map's f64 p-norm the device's 3-norm."""
    shim.set_device_switches(True)
    try:
        for w, h, ref, t in _parity_cases(workloads):
            score, p3, dm = _one_pair(ce, gpu_ctx, ref, t, w, h)
            want = shim.diffmap(ref, t, w, h)
            assert dm.shape == (h, w) and dm.dtype == np.float32
            bad = np.argwhere(dm.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (w, h, len(bad), bad[:4].tolist())
            assert float(dm.max()) == score, (w, h)
            assert abs(S.pnorm3(dm) - p3) <= 1e-12 * p3, (w, h)
    finally:
        shim.set_device_switches(False)


def _grid(ce, ctx, workloads, w, h, n_refs, per_ref, seed=70):
    b = ce.Batch(ctx, w, h, n_refs, n_refs * per_ref)
    refs, tests = [], []
    for r in range(n_refs):
        ref = workloads.make_reference(w, h, seed + r)
        refs.append(ref)
        b.set_reference(r, ref)
        for k in range(per_ref):
            t = workloads.distort(ref, 30 + 60 * k / max(per_ref - 1, 1), k % 2 == 1)
            tests.append((r, t))
            b.set_test(r * per_ref + k, r, t)
    return b, refs, tests


@pytest.mark.parametrize("n_pairs", [1, 11])
def test_maps_change_no_score_and_reduce_to_it(gpu_ctx, ce, workloads, n_pairs):
    """n_pairs * w * h on either side of the two-stream threshold (4e6 pixels) at 768 x 512."""
    w, h = 768, 512
    b, _, _ = _grid(ce, gpu_ctx, workloads, w, h, 1, n_pairs)
    cfg = ce.MetricConfig(butteraugli=True)
    plain = b.run(n_pairs, cfg)
    p_plain = b.butteraugli_pnorm3(n_pairs)
    mapped = b.run(n_pairs, cfg, butteraugli_diffmap=True)
    p_mapped = b.butteraugli_pnorm3(n_pairs)
    maps = b.butteraugli_diffmaps(0, n_pairs)
    all_plain = b.run(n_pairs, ce.MetricConfig.all())
    all_mapped = b.run(n_pairs, ce.MetricConfig.all(), butteraugli_diffmap=True)
    b.close()
    assert [s.butteraugli for s in plain] == [s.butteraugli for s in mapped]
    assert p_plain.tobytes() == p_mapped.tobytes()
    assert [(s.psnr, s.ssimulacra2, s.dssim, s.butteraugli) for s in all_plain] == \
           [(s.psnr, s.ssimulacra2, s.dssim, s.butteraugli) for s in all_mapped]
    assert maps.shape == (n_pairs, h, w)
    for i in range(n_pairs):
        assert float(maps[i].max()) == mapped[i].butteraugli
        assert abs(S.pnorm3(maps[i]) - p_mapped[i]) <= 1e-12 * p_mapped[i]


BATCH_SCRIPT = r"""
import importlib, json, sys
sys.path.insert(0, %r)
import numpy as np
ce = importlib.import_module("codec-eval_amd")
wl = importlib.import_module("codec-eval_amd.workloads")
ctx = ce.Context(0)
bad = []
for (w, h) in [(200, 136), (129, 65)]:
    b = ce.Batch(ctx, w, h, 3, 7)
    owner = [0, 0, 1, 1, 1, 2, 2]
    refs = [wl.make_reference(w, h, 300 + r) for r in range(3)]
    tests = [wl.distort(refs[r], 25 + 10 * i, i %% 2 == 0) for i, r in enumerate(owner)]
    for r in range(3):
        b.set_reference(r, refs[r])
    for i, r in enumerate(owner):
        b.set_test(i, r, tests[i])
    b.run(7, ce.MetricConfig.perceptual(), butteraugli_diffmap=True)
    maps = b.butteraugli_diffmaps(0, 7)
    b.close()
    for i, r in enumerate(owner):
        one = ce.Batch(ctx, w, h, 1, 1)
        one.set_reference(0, refs[r])
        one.set_test(0, 0, tests[i])
        one.run(1, ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
        m1 = one.butteraugli_diffmaps(0, 1)[0]
        one.close()
        if m1.tobytes() != maps[i].tobytes():
            bad.append([w, h, i])
ctx.close()
print(json.dumps(bad))
""" % ROOT


def test_batch_map_is_the_one_pair_map():
    """Pair i of a three-reference batch of mixed distortions has the map of its one-pair batch."""
    r = subprocess.run([sys.executable, "-c", BATCH_SCRIPT], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == []


@pytest.mark.parametrize("w,h", [(200, 136), (129, 65), (768, 512)])
def test_block_maps_are_block_maxima(gpu_ctx, ce, workloads, w, h):
    b, _, _ = _grid(ce, gpu_ctx, workloads, w, h, 2, 3)
    b.run(6, ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
    full = b.butteraugli_diffmaps(0, 6)
    for B in (2, 8, 64):
        got = b.butteraugli_diffmaps(0, 6, B)
        assert got.shape == (6, -(-h // B), -(-w // B))
        assert got.tobytes() == S.block_max(full, B).tobytes(), (w, h, B)
        mid = b.butteraugli_diffmaps(2, 3, B)  # a range in the middle of the batch
        assert mid.tobytes() == got[2:5].tobytes(), (w, h, B)
    assert b.butteraugli_diffmaps(1, 4).tobytes() == full[1:5].tobytes()
    b.close()


def test_reference_handle_maps(gpu_ctx, ce, workloads):
    w, h = 200, 136
    ref = workloads.make_reference(w, h, 81)
    tests = [workloads.distort(ref, q) for q in (35, 60, 85)]
    b = ce.Batch(gpu_ctx, w, h, 1, 3)
    b.set_reference(0, ref)
    for i, t in enumerate(tests):
        b.set_test(i, 0, t)
    b.run(3, ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
    want = b.butteraugli_diffmaps(0, 3)
    b.close()
    h_ = ce.ReferenceHandle(gpu_ctx, ref, w, h, butteraugli_diffmap=True)
    cfg = ce.MetricConfig(butteraugli=True, ssimulacra2=True)
    for _ in range(2):  # the first compare builds the reference side, the second reuses it
        h_.compare_many(tests, cfg)
        assert h_.stats()[2] == 1
        assert h_.butteraugli_diffmaps(0, 3).tobytes() == want.tobytes()
        assert h_.butteraugli_diffmaps(1, 2, 8).tobytes() == S.block_max(want[1:], 8).tobytes()
    h_.compare_many(tests[::-1][:2], cfg)
    assert h_.stats()[2] == 1
    assert h_.butteraugli_diffmaps(0, 2).tobytes() == want[::-1][:2].tobytes()
    with pytest.raises(ce.CodecEvalError):  # two tests in the last compare
        h_.butteraugli_diffmaps(0, 3)
    h_.compare_many(tests + tests, cfg)  # a larger batch takes over the handle: the maps are the new batch's
    assert h_.butteraugli_diffmaps(0, 6).tobytes() == np.concatenate([want, want]).tobytes()
    h_.compare_many(tests, ce.MetricConfig.ssimulacra2_only())  # no Butteraugli: no maps
    with pytest.raises(ce.CodecEvalError) as e:
        h_.butteraugli_diffmaps(0, 1)
    assert e.value.status == ce.CE_ERR_INVALID_ARG
    h_.close()
    plain = ce.ReferenceHandle(gpu_ctx, ref, w, h)
    plain.compare_many(tests, cfg)
    with pytest.raises(ce.CodecEvalError):
        plain.butteraugli_diffmaps(0, 1)
    plain.close()


def test_leaf_call(gpu_ctx, ce, workloads):
    for (w, h) in ((96, 80), (129, 65)):
        ref = workloads.make_reference(w, h, 91)
        t = workloads.distort(ref, 50)
        for it in (80.0, 250.0, 30.0):
            r = gpu_ctx.calculate_butteraugli_diffmap(ref, t, w, h, it)
            assert r.score == gpu_ctx.calculate_butteraugli_with_intensity(ref, t, w, h, it)
            assert r.diffmap.shape == (h, w) and float(r.diffmap.max()) == r.score
            assert r.diffmap.tobytes() == _one_pair(ce, gpu_ctx, ref, t, w, h, it=it)[2].tobytes()
    with pytest.raises(ce.MetricCalculation):
        gpu_ctx.calculate_butteraugli_diffmap(ref[:7, :7], ref[:7, :7], 7, 7)
    with pytest.raises(ce.DimensionMismatch):
        gpu_ctx.calculate_butteraugli_diffmap(ref, ref[:-1], w, h)


def test_locality(gpu_ctx, ce, workloads):
    w = h = 256
    ref = workloads.make_reference(w, h, 101)
    t = ref.copy()
    y0, x0 = 96, 160
    t[y0:y0 + 32, x0:x0 + 32] = workloads.distort(ref, 10)[y0:y0 + 32, x0:x0 + 32] // 2
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    b.set_reference(0, ref)
    b.set_test(0, 0, t)
    b.run(1, ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
    cells = b.butteraugli_diffmaps(0, 1, 8)[0]
    b.close()
    cy, cx = np.unravel_index(int(np.argmax(cells)), cells.shape)
    assert y0 // 8 - 1 <= cy <= (y0 + 31) // 8 + 1 and x0 // 8 - 1 <= cx <= (x0 + 31) // 8 + 1, (cy, cx)


def test_invalid_readouts(gpu_ctx, ce, workloads):
    L = ce.lib()
    w, h = 100, 60
    ref = workloads.make_reference(w, h, 111)
    t = workloads.distort(ref, 40)
    b = ce.Batch(gpu_ctx, w, h, 1, 4)
    b.set_reference(0, ref)
    for i in range(4):
        b.set_test(i, 0, t)
    buf = np.zeros(4 * w * h, np.float32)

    def read(first, count, block, n):
        return L.ce_batch_butteraugli_diffmap(b._h, first, count, block, buf.ctypes.data, n)

    assert read(0, 1, 1, w * h) == ce.CE_ERR_INVALID_ARG  # before any flagged launch
    b.run(3, ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
    assert read(0, 3, 1, 3 * w * h) == ce.CE_OK
    assert read(2, 2, 1, 2 * w * h) == ce.CE_ERR_INVALID_ARG  # past the three stored pairs
    assert read(3, 1, 1, w * h) == ce.CE_ERR_INVALID_ARG
    for block in (0, 3, 128):
        n = -(-w // max(block, 1)) * -(-h // max(block, 1))
        assert read(0, 1, block, n) == ce.CE_ERR_INVALID_ARG
    assert read(0, 1, 8, 13 * 8 + 1) == ce.CE_ERR_INVALID_ARG  # wrong out_floats
    assert read(0, 1, 8, 13 * 8) == ce.CE_OK
    assert L.ce_batch_butteraugli_diffmap(b._h, 0, 1, 1, None, w * h) == ce.CE_ERR_INVALID_ARG
    b.run(3, ce.MetricConfig(butteraugli=True))  # a launch without the flag forgets the maps
    assert read(0, 1, 1, w * h) == ce.CE_ERR_INVALID_ARG
    b.run(3, ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
    b.run(3, ce.MetricConfig(ssimulacra2=True), butteraugli_diffmap=True)  # ... and so does one without Butteraugli
    assert read(0, 1, 1, w * h) == ce.CE_ERR_INVALID_ARG
    b.close()
    pairs = (ce.CePairDesc * 1)()
    r_, t_ = np.ascontiguousarray(ref).reshape(-1), np.ascontiguousarray(t).reshape(-1)
    pairs[0].reference, pairs[0].reference_len, pairs[0].test, pairs[0].test_len = r_.ctypes.data, r_.size, t_.ctypes.data, t_.size
    pairs[0].width, pairs[0].height = w, h
    out = (ce.CeScores * 1)()
    flags = ce.FLAG_BUTTERAUGLI_DIFFMAP
    assert L.ce_eval_batch(gpu_ctx._h, 1, pairs, ce.METRIC_BUTTERAUGLI, flags, 80.0, out) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair(gpu_ctx._h, r_.ctypes.data, r_.size, t_.ctypes.data, t_.size, w, h, ce.METRIC_BUTTERAUGLI, flags, 80.0,
                          ctypes.byref(out[0])) == ce.CE_ERR_INVALID_ARG


# Launch geometry the shapes below sit on (butteraugli.hip): front tiles FT = 32 x 32; the row blur's blocks (gh3 of
# ce_launch_butteraugli) 256 columns x 8 * BH_TILES = 32 rows; the fused column / blur tiles (k_ba_blur_v_split) 64 x 32;
# the Malta tiles MT = 64 columns x 32 rows.  The half-resolution level is ((w + 1) / 2, (h + 1) / 2) and exists when it
# is at least 8 x 8 (ba_levels).  Entries: (w, h, the half level's (w, h) or None for one level) - the test asserts the
# third field, so that a comment here cannot claim a level that is not built.
BA_EDGE_SHAPES = [
    (8, 8, None),  # the 8 x 8 minimum
    (14, 40, None), (15, 41, (8, 21)), (16, 42, (8, 21)),  # one / two levels in w
    (40, 14, None), (41, 15, (21, 8)), (42, 16, (21, 8)),  # ... and in h
    (31, 31, (16, 16)), (32, 32, (16, 16)), (33, 33, (17, 17)),  # the front tiles and the 32-row blocks, both axes
    (61, 61, (31, 31)),  # half level one under the front tiles and the 32-row blocks
    (63, 63, (32, 32)), (64, 64, (32, 32)), (65, 65, (33, 33)),  # the 64-column fused-blur and Malta tiles; half level on /
    # over the front tiles and the 32-row blocks
    (125, 20, (63, 10)), (127, 16, (64, 8)), (129, 17, (65, 9)),  # half level under / on / over the 64-column tiles
    (255, 63, (128, 32)), (256, 64, (128, 32)), (257, 65, (129, 33)),  # the row blur's 256-column block, 2 x 32 rows
    (509, 15, (255, 8)), (511, 16, (256, 8)), (513, 17, (257, 9)),  # half level under / on / over the 256-column block
    (40, 125, (20, 63)), (70, 129, (35, 65)),  # half level one under / over 64 rows
    (256, 10, None), (257, 11, None), (100, 12, None), (90, 13, None),  # one level, heights under the 33-tap halo
    (1000, 9, None),  # a wide one-level strip
    (9, 700, None),  # a tall one-level strip
    (768, 512, (384, 256)),  # the headline shape
]


def ba_half_level(w, h):
    """ce_batch's Butteraugli levels: the half-resolution (w, h), or None where it would be under 8 x 8."""
    hw, hh = (w + 1) // 2, (h + 1) // 2
    return (hw, hh) if hw >= 8 and hh >= 8 else None


def _first_difference(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size == 0:
        return None
    y, x = bad[0].tolist()
    return {"pixels": len(bad), "first": [y, x], "got": float(got[y, x]), "want": float(want[y, x])}


def _edge_batch(workloads, w, h):
    """2 references x 2 distorted images, the second of each with 4:2:0 chroma."""
    refs = [workloads.make_reference(w, h, 500 + 7 * w + h + r) for r in range(2)]
    pairs = [(r, workloads.distort(refs[r], 35 + 40 * k, k == 1)) for r in range(2) for k in range(2)]
    return refs, pairs


def _run_edge_batch(ce, ctx, w, h, refs, pairs):
    b = ce.Batch(ctx, w, h, len(refs), len(pairs))
    for r, ref in enumerate(refs):
        b.set_reference(r, ref)
    for i, (r, t) in enumerate(pairs):
        b.set_test(i, r, t)
    s = b.run(len(pairs), ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
    assert all(x.status == 0 for x in s)
    out = ([x.butteraugli for x in s], b.butteraugli_pnorm3(len(pairs)), b.butteraugli_diffmaps(0, len(pairs)))
    b.close()
    return out


@pytest.fixture(scope="module")
def serial_ctx(ce):
    """A second context with serial profiling: no second stream for the half level (two_streams) and no metric fork."""
    ctx = ce.Context(0)
    ctx.prof_enable(True, serial=True)
    yield ctx
    ctx.prof_enable(False)
    ctx.close()


@pytest.mark.parametrize("w,h,half", BA_EDGE_SHAPES)
def test_edge_shapes_map_is_the_oracle_map_bit_for_bit(gpu_ctx, serial_ctx, ce, workloads, shim, w, h, half):
    """Every pair's map is the oracle's (device switches on) pixel for pixel, its maximum is the score and its f64 p-norm
    the device's 3-norm; the serial schedule gives the same maps and scores bit for bit."""
    assert ba_half_level(w, h) == half, (w, h, ba_half_level(w, h), half)
    refs, pairs = _edge_batch(workloads, w, h)
    scores, p3, maps = _run_edge_batch(ce, gpu_ctx, w, h, refs, pairs)
    assert maps.shape == (len(pairs), h, w) and maps.dtype == np.float32
    shim.set_device_switches(True)
    try:
        want = [shim.diffmap(refs[r], t, w, h) for r, t in pairs]
    finally:
        shim.set_device_switches(False)
    for i in range(len(pairs)):
        assert _first_difference(maps[i], want[i]) is None, (w, h, i, _first_difference(maps[i], want[i]))
        assert float(maps[i].max()) == scores[i], (w, h, i)
        assert abs(S.pnorm3(maps[i]) - p3[i]) <= 1e-12 * p3[i], (w, h, i)
    s_scores, s_p3, s_maps = _run_edge_batch(ce, serial_ctx, w, h, refs, pairs)
    for i in range(len(pairs)):
        assert _first_difference(s_maps[i], maps[i]) is None, ("serial", w, h, i, _first_difference(s_maps[i], maps[i]))
    assert s_scores == scores and s_p3.tobytes() == p3.tobytes()


def test_batch_past_the_two_stream_limit_has_the_one_pair_maps(gpu_ctx, ce, workloads):
    """257 x 129 x 128 pairs = 4.24e6 pixels, over the 4e6 under which the half level gets a stream of its own: the batch
    runs both levels on one stream, each pair's map is its one-pair call's (two streams) bit for bit."""
    w, h, n_refs, per_ref = 257, 129, 4, 32
    assert n_refs * per_ref * w * h > 4e6
    b = ce.Batch(gpu_ctx, w, h, n_refs, n_refs * per_ref)
    refs, pairs = [], []
    for r in range(n_refs):
        refs.append(workloads.make_reference(w, h, 620 + r))
        b.set_reference(r, refs[r])
        for k in range(per_ref):
            t = workloads.distort(refs[r], 20 + 2 * k, k % 3 == 0)
            b.set_test(len(pairs), r, t)
            pairs.append((r, t))
    s = b.run(len(pairs), ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
    maps = b.butteraugli_diffmaps(0, len(pairs))
    b.close()
    one = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        for i, (r, t) in enumerate(pairs):
            one.set_reference(0, refs[r])
            one.set_test(0, 0, t)
            s1 = one.run(1, ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
            m1 = one.butteraugli_diffmaps(0, 1)[0]
            assert _first_difference(maps[i], m1) is None, (i, _first_difference(maps[i], m1))
            assert s[i].butteraugli == s1[0].butteraugli, i
    finally:
        one.close()
