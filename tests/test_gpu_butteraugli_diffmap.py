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
