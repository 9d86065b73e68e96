"""DSSIM's SsimMap on the device (dssim-core's Dssim::compare -> (Val, Vec<SsimMap>), re-exported at
src/metrics/prelude.rs:45): every level's stored SSIM map is the oracle's map bit for bit, SsimMap.ssim is the oracle's
per-scale score, the block readouts are exact cell minima, and every readout path returns the maps of the launch it
names."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dssim_map_shim as S
from test_gpu_parity import DSSIM_SHAPES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = (1, 2, 4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.Shim(tmp_path_factory.mktemp("dssim_shim"))


def _first_difference(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size == 0:
        return None
    y, x = bad[0].tolist()
    return {"pixels": len(bad), "first": [y, x], "got": float(got[y, x]), "want": float(want[y, x])}


def _check_against_shim(shim, ref, t, w, h, score, maps, where):
    want_d, want = shim.maps(ref, t, w, h)
    assert [(m.map.shape[1], m.map.shape[0]) for m in maps] == shim.levels(w, h), where
    for l, (m, (wm, ws)) in enumerate(zip(maps, want)):
        assert m.map.dtype == np.float32
        diff = _first_difference(m.map, wm)
        assert diff is None, (where, l, diff)
        assert abs(m.ssim - ws) <= 1e-12, (where, l, m.ssim, ws)
    assert abs(S.dssim_from_scores([m.ssim for m in maps]) - score) <= 1e-12 * max(abs(score), 1e-300), where
    assert abs(score - want_d) <= 1e-9 * max(abs(want_d), 1e-6), where


@pytest.mark.parametrize("w,h", DSSIM_SHAPES)
def test_full_maps_are_the_oracle_maps_bit_for_bit(gpu_ctx, workloads, shim, w, h):
    ref = workloads.make_reference(w, h, 300 + w)
    for q in (30, 75, 95):
        t = workloads.distort(ref, q)
        score, maps = gpu_ctx.calculate_dssim_with_ssim_maps(ref, t, w, h)
        assert score == gpu_ctx.calculate_dssim(ref, t, w, h)
        _check_against_shim(shim, ref, t, w, h, score, maps, (w, h, q))


def test_flat_plus_noise(gpu_ctx, workloads, shim):
    w = h = 96
    flat = workloads.make_reference(w, h, 5, "flat")
    noisy = np.clip(flat.astype(np.int16) + np.random.default_rng(5).integers(-3, 4, flat.shape), 0, 255).astype(np.uint8)
    score, maps = gpu_ctx.calculate_dssim_with_ssim_maps(flat, noisy, w, h)
    _check_against_shim(shim, flat, noisy, w, h, score, maps, "flat+noise")


def _grid(ce, ctx, workloads, w, h, n_refs, per_ref, seed=170):
    b = ce.Batch(ctx, w, h, n_refs, n_refs * per_ref)
    pairs = []
    for r in range(n_refs):
        ref = workloads.make_reference(w, h, seed + r)
        b.set_reference(r, ref)
        for k in range(per_ref):
            t = workloads.distort(ref, 25 + 70 * k / max(per_ref - 1, 1), k % 2 == 1)
            pairs.append((ref, t))
            b.set_test(r * per_ref + k, r, t)
    return b, pairs


def test_batch_maps_are_the_one_pair_maps(ce, gpu_ctx, workloads):
    """512 x 512, 64 pairs: the compare kernel walks 32 rows at level 0 (a one-pair call walks 4); pair i's maps and scores
    of every level are its one-pair call's bit for bit."""
    w = h = 512
    b, pairs = _grid(ce, gpu_ctx, workloads, w, h, 4, 16)
    s = b.run(64, ce.MetricConfig(dssim=True))
    levels = ce.dssim_levels(w, h)
    got = [b.dssim_ssim_maps(l, 0, 64) for l in range(len(levels))]
    b.close()
    for i, (ref, t) in enumerate(pairs):
        score, maps = gpu_ctx.calculate_dssim_with_ssim_maps(ref, t, w, h)
        assert len(maps) == len(levels)
        for l, m in enumerate(maps):
            assert got[l][0][i].tobytes() == m.map.tobytes(), (i, l, _first_difference(got[l][0][i], m.map))
            assert got[l][1][i] == m.ssim, (i, l, got[l][1][i], m.ssim)
        assert s[i].dssim == score, (i, s[i].dssim, score)


@pytest.mark.parametrize("w,h", [(200, 136), (129, 65), (768, 512), (9, 301)])
def test_block_readout_is_the_cell_minimum(ce, gpu_ctx, workloads, w, h):
    b, _ = _grid(ce, gpu_ctx, workloads, w, h, 2, 3)
    b.run(6, ce.MetricConfig(dssim=True))
    for l, (lw, lh) in enumerate(ce.dssim_levels(w, h)):
        full, ssim = b.dssim_ssim_maps(l, 0, 6)
        assert full.shape == (6, lh, lw) and ssim.shape == (6,)
        for B in BLOCKS:
            got, s2 = b.dssim_ssim_maps(l, 0, 6, B)
            assert got.shape == (6, -(-lh // B), -(-lw // B))
            assert got.tobytes() == S.block_min(full, B).tobytes(), (w, h, l, B)
            assert s2.tobytes() == ssim.tobytes()
            for first, count in ((2, 3), (5, 1), (0, 1)):
                mid, sm = b.dssim_ssim_maps(l, first, count, B)
                assert mid.tobytes() == got[first:first + count].tobytes(), (w, h, l, B, first, count)
                assert sm.tobytes() == ssim[first:first + count].tobytes()
    b.close()


def test_reference_handle_maps(ce, gpu_ctx, workloads, shim):
    w, h = 200, 136
    ref = workloads.make_reference(w, h, 181)
    tests = [workloads.distort(ref, q) for q in (35, 60, 85)]
    levels = ce.dssim_levels(w, h)
    one = [gpu_ctx.calculate_dssim_with_ssim_maps(ref, t, w, h)[1] for t in tests]

    def check(handle, idx):
        for l in range(len(levels)):
            maps, ssim = handle.dssim_ssim_maps(l, 0, len(idx))
            for j, i in enumerate(idx):
                assert maps[j].tobytes() == one[i][l].map.tobytes(), (l, j, i)
                assert abs(ssim[j] - one[i][l].ssim) <= 1e-12

    hd = ce.ReferenceHandle(gpu_ctx, ref, w, h)
    cfg = ce.MetricConfig(dssim=True, ssimulacra2=True)
    hd.compare_many(tests, cfg)
    assert hd.stats()[1] == 1
    check(hd, [0, 1, 2])
    hd.compare_many(tests + tests, cfg)  # a larger batch takes over the handle
    check(hd, [0, 1, 2, 0, 1, 2])
    builds = hd.stats()
    for i in (2, 0, 1):  # further compares with the cached pyramid: the maps of the latest call
        hd.compare(tests[i], cfg)
        assert hd.stats() == builds
        check(hd, [i])
    with pytest.raises(ce.CodecEvalError):  # one test in the last compare
        hd.dssim_ssim_maps(0, 1, 1)
    hd.compare_many(tests, ce.MetricConfig.ssimulacra2_only())  # no DSSIM: no maps
    with pytest.raises(ce.CodecEvalError) as e:
        hd.dssim_ssim_maps(0, 0, 1)
    assert e.value.status == ce.CE_ERR_INVALID_ARG
    hd.close()

    rt = ce.ReferenceHandle(gpu_ctx, ref, w, h, xyb_roundtrip=True)
    rt.compare_many(tests, ce.MetricConfig(dssim=True))
    rref = gpu_ctx.xyb_roundtrip(ref, w, h)
    for i, t in enumerate(tests):
        _, want = shim.maps(rref, t, w, h)
        for l, (wm, ws) in enumerate(want):
            maps, ssim = rt.dssim_ssim_maps(l, i, 1)
            assert _first_difference(maps[0], wm) is None, (i, l)
            assert abs(ssim[0] - ws) <= 1e-12
    rt.close()


def test_invalidation_and_rejected_arguments(ce, gpu_ctx, workloads):
    L = ce.lib()
    w, h = 100, 60
    ref = workloads.make_reference(w, h, 211)
    t = workloads.distort(ref, 40)
    b = ce.Batch(gpu_ctx, w, h, 1, 4)
    b.set_reference(0, ref)
    for i in range(4):
        b.set_test(i, 0, t)
    levels = ce.dssim_levels(w, h)  # (100, 60), (50, 30), (25, 15), (12, 7)
    assert len(levels) == 4
    maps = np.zeros(4 * w * h, np.float32)
    ssim = np.zeros(4, np.float64)

    def read(level, first, count, block, n, m=maps.ctypes.data, s=ssim.ctypes.data):
        return L.ce_batch_dssim_ssim_maps(b._h, level, first, count, block, m, n, s)

    assert read(0, 0, 1, 1, w * h) == ce.CE_ERR_INVALID_ARG  # before any launch
    b.run(3, ce.MetricConfig(dssim=True))
    assert read(0, 0, 3, 1, 3 * w * h) == ce.CE_OK
    assert read(3, 0, 3, 1, 3 * 12 * 7) == ce.CE_OK
    assert read(4, 0, 1, 1, 1) == ce.CE_ERR_INVALID_ARG  # level >= n_levels
    assert read(0, 0, 0, 1, 0) == ce.CE_ERR_INVALID_ARG  # count = 0
    assert read(0, 2, 2, 1, 2 * w * h) == ce.CE_ERR_INVALID_ARG  # past the three stored pairs
    assert read(0, 3, 1, 1, w * h) == ce.CE_ERR_INVALID_ARG
    for block in (0, 3, 128):
        n = -(-w // max(block, 1)) * -(-h // max(block, 1))
        assert read(0, 0, 1, block, n) == ce.CE_ERR_INVALID_ARG
    assert read(0, 0, 1, 8, 13 * 8 + 1) == ce.CE_ERR_INVALID_ARG  # wrong maps_floats
    assert read(0, 0, 1, 8, 13 * 8) == ce.CE_OK
    assert read(0, 0, 1, 1, 0, m=None) == ce.CE_OK  # scores only
    assert read(0, 0, 1, 1, w * h, m=None) == ce.CE_ERR_INVALID_ARG  # no maps output: maps_floats 0
    assert read(0, 0, 1, 1, w * h, s=None) == ce.CE_OK  # maps only
    assert read(0, 0, 1, 1, 0, m=None, s=None) == ce.CE_ERR_INVALID_ARG  # neither
    b.run(3, ce.MetricConfig(ssimulacra2=True))  # a launch without DSSIM forgets the maps
    assert read(0, 0, 1, 1, w * h) == ce.CE_ERR_INVALID_ARG
    b.close()

    # the one-pair call keeps ce_calculate_dssim's errors and checks maps_floats
    r_, t_ = np.ascontiguousarray(ref).reshape(-1), np.ascontiguousarray(t).reshape(-1)
    total = sum(a * c for a, c in levels)
    big = np.zeros(total + 1, np.float32)
    lv, d = np.zeros(5, np.float64), ctypes.c_double()

    def leaf(rl, tl, ww, hh, n):
        return L.ce_calculate_dssim_ssim_maps(gpu_ctx._h, r_.ctypes.data, rl, t_.ctypes.data, tl, ww, hh, ctypes.byref(d), lv.ctypes.data,
                                              big.ctypes.data, n)

    assert leaf(r_.size, t_.size, w, h, total) == ce.CE_OK
    assert leaf(r_.size, t_.size, w, h, total + 1) == ce.CE_ERR_INVALID_ARG
    assert leaf(r_.size, t_.size, w, h, total - 1) == ce.CE_ERR_INVALID_ARG
    assert leaf(r_.size, t_.size - 3, w, h, total) == ce.CE_ERR_DIM_MISMATCH
    assert leaf(r_.size, t_.size, w, h - 1, total) == ce.CE_ERR_BAD_LENGTH
    assert leaf(r_.size, t_.size, 0, h, 0) == ce.CE_ERR_INVALID_ARG
    assert leaf(r_.size, t_.size, w, 0, 0) == ce.CE_ERR_INVALID_ARG
    with pytest.raises(ce.DimensionMismatch):
        gpu_ctx.calculate_dssim_with_ssim_maps(ref, t[:-1], w, h)
    assert np.isnan(lv[4]) and not np.isnan(lv[3])


def test_dssim_and_butteraugli_maps_together_and_scores_unchanged(ce, gpu_ctx, workloads):
    w, h = 129, 65
    b, pairs = _grid(ce, gpu_ctx, workloads, w, h, 1, 4)
    cfg = ce.MetricConfig(dssim=True, butteraugli=True)
    plain = b.run(4, cfg)
    plain_all = b.run(4, ce.MetricConfig.all())
    mapped = b.run(4, cfg, butteraugli_diffmap=True)
    dm = b.butteraugli_diffmaps(0, 4)
    sm = [b.dssim_ssim_maps(l, 0, 4) for l in range(len(ce.dssim_levels(w, h)))]
    again = b.run(4, ce.MetricConfig.all())
    for l in range(len(sm)):
        b.dssim_ssim_maps(l, 0, 4, 8)
    after_read = b.run(4, ce.MetricConfig.all())
    b.close()
    key = lambda ss: [(s.psnr, s.ssimulacra2, s.dssim, s.butteraugli) for s in ss]
    assert [(s.dssim, s.butteraugli) for s in plain] == [(s.dssim, s.butteraugli) for s in mapped]
    assert key(plain_all) == key(again) == key(after_read)
    for i, (ref, t) in enumerate(pairs):
        assert float(dm[i].max()) == mapped[i].butteraugli
        _, one = gpu_ctx.calculate_dssim_with_ssim_maps(ref, t, w, h)
        for l, m in enumerate(one):
            assert sm[l][0][i].tobytes() == m.map.tobytes()


def test_identical_images_give_maps_of_one(gpu_ctx, workloads):
    for w, h in ((64, 48), (7, 9), (200, 136)):
        ref = workloads.make_reference(w, h, 7 + w)
        score, maps = gpu_ctx.calculate_dssim_with_ssim_maps(ref, ref, w, h)
        assert score == 0.0
        for m in maps:
            assert np.all(m.map == 1.0) and m.ssim == 1.0


def test_cpp_mirror(ce, gpu_ctx, workloads, tmp_path):
    """tests/cpp/test_dssim_maps_mirror.cpp: calculate_dssim_with_ssim_maps of the C++ host mirror, built with g++ as
    test_host_cpp.py builds its programs, returns what the Python binding returns."""
    exe = str(tmp_path / "test_dssim_maps_mirror")
    libdir = os.path.dirname(ce.LIB_PATH)
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "host"),
        os.path.join(ROOT, "tests", "cpp", "test_dssim_maps_mirror.cpp"), "-o", exe,
        "-L", libdir, "-lce_metrics_hip", f"-Wl,-rpath,{libdir}", "-pthread",
    ])
    w, h = 97, 61
    ref = workloads.make_reference(w, h, 77)
    t = workloads.distort(ref, 45)
    rf, tf = tmp_path / "ref.rgb", tmp_path / "test.rgb"
    rf.write_bytes(ref.tobytes())
    tf.write_bytes(t.tobytes())
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([exe, str(rf), str(tf), str(w), str(h), str(out_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    score, maps = gpu_ctx.calculate_dssim_with_ssim_maps(ref, t, w, h)
    lines = r.stdout.strip().splitlines()
    assert float.fromhex(lines[0]) == score
    assert len(lines) == 1 + len(maps)
    for l, m in enumerate(maps):
        lw, lh, ssim = lines[1 + l].split()
        assert (int(lw), int(lh)) == (m.map.shape[1], m.map.shape[0])
        assert float.fromhex(ssim) == m.ssim
        assert (out_dir / f"level{l}.f32").read_bytes() == m.map.tobytes()


WALKS = (2, 4, 8, 16, 32, 64)  # every walk length stream_rows can pick (dssim_stream.hip)
# heights one row under / over one, two and three walks of the longer lengths, at a one-strip and a two-strip width (60
# output columns per strip): the top block (i0 = -1), the surplus steps at the bottom and a last block of 1 .. r rows
WALK_SHAPES = sorted({(w, h) for w in (61, 121) for r in (8, 16, 32, 64) for h in (r - 1, r + 1, 2 * r - 1, 3 * r + 1)})


def _walk_batch(ce, ctx, workloads, w, h):
    """2 references x 2 distorted images (the second with 4:2:0 chroma)."""
    b = ce.Batch(ctx, w, h, 2, 4)
    pairs = []
    for r in range(2):
        ref = workloads.make_reference(w, h, 700 + 3 * w + h + r)
        b.set_reference(r, ref)
        for k in range(2):
            t = workloads.distort(ref, 30 + 45 * k, k == 1)
            b.set_test(len(pairs), r, t)
            pairs.append((ref, t))
    return b, pairs


def _set_tests(b, pairs, identical=False):
    for i, (ref, t) in enumerate(pairs):
        b.set_test(i, i // 2, ref if identical else t)


@pytest.mark.parametrize("w,h", DSSIM_SHAPES + WALK_SHAPES)
def test_every_walk_length_gives_the_oracle_maps(ce, gpu_ctx, workloads, shim, w, h):
    """Forced walk lengths (ce_debug_dssim_walk_rows) of the create and compare streams: at every level every pair's map is
    the oracle's bit for bit, and its per-level ssim and DSSIM score are the same bits for all six walks."""
    b, pairs = _walk_batch(ce, gpu_ctx, workloads, w, h)
    want = [shim.maps(ref, t, w, h) for ref, t in pairs]
    n_levels = len(ce.dssim_levels(w, h))
    first = None
    try:
        for rows in WALKS:
            b.debug_dssim_walk_rows(rows)
            # identical pairs first (every map 1.0), so that a pixel the walk does not store cannot keep the last walk's value
            _set_tests(b, pairs, identical=True)
            assert all(x.dssim == 0.0 for x in b.run(len(pairs), ce.MetricConfig(dssim=True))), (w, h, rows)
            _set_tests(b, pairs)
            s = b.run(len(pairs), ce.MetricConfig(dssim=True))
            got = [b.dssim_ssim_maps(l, 0, len(pairs)) for l in range(n_levels)]
            for i, (want_d, want_levels) in enumerate(want):
                assert len(want_levels) == n_levels
                for l, (wm, ws) in enumerate(want_levels):
                    diff = _first_difference(got[l][0][i], wm)
                    assert diff is None, (w, h, rows, i, l, diff)
                    assert abs(got[l][1][i] - ws) <= 1e-12, (w, h, rows, i, l, got[l][1][i], ws)
                assert abs(s[i].dssim - want_d) <= 1e-9 * max(abs(want_d), 1e-6), (w, h, rows, i)
            bits = ([x.dssim for x in s], [g[1].tobytes() for g in got])
            if first is None:
                first = bits
            assert bits == first, (w, h, rows, "scores differ from the 2-row walk's", [x.dssim for x in s], first[0])
    finally:
        b.close()


def test_walk_rows_hook_rejects_other_lengths(ce, gpu_ctx, workloads):
    L = ce.lib()
    b, pairs = _walk_batch(ce, gpu_ctx, workloads, 61, 33)
    for rows in (1, 3, 6, 48, 65, 128, 1 << 31):
        assert L.ce_debug_dssim_walk_rows(b._h, rows) == ce.CE_ERR_INVALID_ARG, rows
    auto = b.run(4, ce.MetricConfig(dssim=True))
    b.debug_dssim_walk_rows(64)
    forced = b.run(4, ce.MetricConfig(dssim=True))
    b.debug_dssim_walk_rows(0)  # back to the automatic choice
    again = b.run(4, ce.MetricConfig(dssim=True))
    b.close()
    assert [x.dssim for x in auto] == [x.dssim for x in forced] == [x.dssim for x in again]


def test_natural_64_row_walk_is_the_one_pair_walk(ce, gpu_ctx, workloads):
    """Without the hook: at 768 x 512 (13 strips of 60 columns, 8 blocks of 64 rows) 80 pairs make 13 * 8 * 80 = 8320
    waves, at least the 8192 at which stream_rows keeps 64 rows for level 0, where a one-pair call walks 4.  Every pair's
    maps, per-level ssim and score are its one-pair call's bit for bit."""
    # stream_rows' threshold is the A/B knob CE_STREAM_MIN_WAVES (default 8192): set, this batch could walk fewer rows
    assert "CE_STREAM_MIN_WAVES" not in os.environ, "unset CE_STREAM_MIN_WAVES: this test needs stream_rows' default"
    w, h, n_refs, per_ref = 768, 512, 4, 20
    n = n_refs * per_ref
    assert 13 * 8 * n >= 8192
    b, pairs = _grid(ce, gpu_ctx, workloads, w, h, n_refs, per_ref, seed=730)
    s = b.run(n, ce.MetricConfig(dssim=True))
    levels = ce.dssim_levels(w, h)
    got = [b.dssim_ssim_maps(l, 0, n) for l in range(len(levels))]
    b.close()
    for i, (ref, t) in enumerate(pairs):
        score, maps = gpu_ctx.calculate_dssim_with_ssim_maps(ref, t, w, h)
        for l, m in enumerate(maps):
            assert got[l][0][i].tobytes() == m.map.tobytes(), (i, l, _first_difference(got[l][0][i], m.map))
            assert got[l][1][i] == m.ssim, (i, l, got[l][1][i], m.ssim)
        assert s[i].dssim == score, (i, s[i].dssim, score)
