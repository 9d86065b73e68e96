"""SSIMULACRA2's error maps on the device (CE_FLAG_SSIMULACRA2_MAPS): every scale's SSIM-error map is the oracle's bit for
bit and the artifact / detail-lost maps match it to a few ulp with the same zeros, across the row-pass parity shapes, the
4-row group edges of the column pass and its 64-column strips, in both the level-0 and the merged levels-1..5 launch; the
norms are the pooled values the score weighs; scores do not change with the flag; and every readout path returns the maps
of the launch it names."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ssim2_map_shim as S
from test_gpu_ssim2_row_streams import ROW_SHAPES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_REL = 2.0 ** -20
MAX_EDGE_DEV = [0.0]  # largest relative deviation of an artifact / detail-lost value seen (reported by the last test)

# heights at 4k - 1, 4k, 4k + 1 and under 16 rows (the head / tail loops of the column pass's 4-row DMA groups), widths at
# 64k +- 1 (the column pass's 64-column strips), the Kodak shapes
GROUP_SHAPES = [(40, 8), (40, 9), (40, 11), (40, 12), (40, 13), (40, 15), (37, 16), (37, 17), (70, 31), (70, 32), (70, 33),
                (63, 47), (65, 48), (127, 49), (129, 20), (191, 23), (193, 24), (257, 19)]
SHAPES = ROW_SHAPES + GROUP_SHAPES + [(768, 512), (512, 768)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.Shim(tmp_path_factory.mktemp("ssim2_map_shim"))


def _check_scale(dev, want, where):
    """dev: float32 [3 channels, 3 kinds, h, w]; want: the shim's (d [3, h, w], edge [3, 2, h, w])."""
    d, e = want
    assert dev.shape == (3, 3) + d.shape[1:], where
    for c in range(3):
        got = dev[c, 0]
        bad = np.argwhere(got.view(np.uint32) != d[c].view(np.uint32))
        assert bad.size == 0, (where, c, "ssim", len(bad), bad[0].tolist(), float(got[tuple(bad[0])]), float(d[c][tuple(bad[0])]))
        for k in (1, 2):
            got, ref = dev[c, k], e[c, k - 1]
            assert np.array_equal(got > 0, ref > 0), (where, c, k, int(np.sum((got > 0) != (ref > 0))))
            assert np.all(got >= 0), (where, c, k)
            nz = ref > 0
            if np.any(nz):
                r32 = ref[nz].astype(np.float32).astype(np.float64)
                dev_rel = float(np.max(np.abs(got[nz].astype(np.float64) - r32) / r32))
                MAX_EDGE_DEV[0] = max(MAX_EDGE_DEV[0], dev_rel)
                assert dev_rel <= EDGE_REL, (where, c, k, dev_rel)


def _check_pair(shim, ref, t, w, h, scales, where):
    want = shim.maps(ref, t, w, h)
    assert len(scales) == len(want) and [(m.shape[3], m.shape[2]) for m in scales] == S.Shim.scales(shim, w, h), where
    for s, (dev, ws) in enumerate(zip(scales, want)):
        _check_scale(dev, ws, where + (s,))


@pytest.mark.parametrize("w,h", SHAPES)
def test_one_pair_maps_match_the_oracle(gpu_ctx, ce, workloads, shim, w, h):
    ref = workloads.make_reference(w, h, 900 + w + h)
    for q in (30, 90):
        t = workloads.distort(ref, q)
        score, feats, scales = gpu_ctx.calculate_ssimulacra2_with_maps(ref, t, w, h)
        assert score == gpu_ctx.calculate_ssimulacra2(ref, t, w, h)
        assert [(m.shape[3], m.shape[2]) for m in scales] == ce.ssimulacra2_scales(w, h)
        assert feats.shape == (6, 3, 6) and np.all(np.isnan(feats[len(scales):])) and not np.any(np.isnan(feats[:len(scales)]))
        _check_pair(shim, ref, t, w, h, scales, (w, h, q))


def _read_all(b, n_scales, first, count, block=1, maps=True):
    """{(s, c, k): (maps, norms)} of a Batch or ReferenceHandle."""
    return {(s, c, k): b.ssimulacra2_maps(s, c, k, first, count, block, maps) for s in range(n_scales) for c in range(3) for k in range(3)}


def _pair_scales(reads, n_scales, q):
    return [np.stack([np.stack([reads[(s, c, k)][0][q] for k in range(3)]) for c in range(3)]) for s in range(n_scales)]


def _build_batch(ce, ctx, workloads, w, h, per_ref):
    b = ce.Batch(ctx, w, h, len(per_ref), sum(per_ref))
    refs, pairs = [], []
    for r, n in enumerate(per_ref):
        ref = workloads.make_reference(w, h, 40 + 7 * r)
        b.set_reference(r, ref)
        refs.append(ref)
        for j in range(n):
            t = workloads.distort(ref, 25 + 60 * j / max(n, 1), j % 2 == 1)
            b.set_test(len(pairs), r, t)
            pairs.append((r, t))
    return b, refs, pairs


def _score_tuple(s):
    return (s.valid, s.status, s.dssim, s.ssimulacra2, s.butteraugli, s.psnr)


@pytest.mark.parametrize("w,h,per_ref", [(97, 61, (3, 1, 4)), (257, 260, (2, 3)), (70, 33, (1, 1, 1))])
def test_batch_maps_norms_and_scores(ce, gpu_ctx, workloads, oracle, shim, w, h, per_ref):
    b, refs, pairs = _build_batch(ce, gpu_ctx, workloads, w, h, per_ref)
    n = len(pairs)
    cfg = ce.MetricConfig.all()
    plain = b.run(n, cfg)
    plain_norms = _read_all(b, len(ce.ssimulacra2_scales(w, h)), 0, n, maps=False)
    flagged = b.run(n, cfg, ssimulacra2_maps=True)
    assert [_score_tuple(s) for s in flagged] == [_score_tuple(s) for s in plain]  # bit for bit, all four metrics
    ns = len(ce.ssimulacra2_scales(w, h))
    reads = _read_all(b, ns, 0, n)
    for key, (_, norms) in reads.items():
        assert norms.tobytes() == plain_norms[key][1].tobytes(), key
    for q, (r, t) in enumerate(pairs):
        scales = _pair_scales(reads, ns, q)
        _check_pair(shim, refs[r], t, w, h, scales, (w, h, q))
        avg = b.debug_averages(q)
        host = np.zeros((ns, 3, 6))
        for (s, c, k), (maps, norms) in reads.items():
            assert norms[q].tobytes() == avg[s, c, 2 * k:2 * k + 2].tobytes(), (q, s, c, k)
            host[s, c, 2 * k:2 * k + 2] = S.pool(maps[q])
        assert np.all(np.abs(host - avg) <= 1e-6 * np.abs(avg) + 1e-12), (q, np.max(np.abs(host - avg)))
        score = flagged[q].ssimulacra2
        assert abs(oracle.ssimulacra2_score(host) - score) <= 1e-6 * max(1.0, abs(score)), (q, oracle.ssimulacra2_score(host), score)
    # block readouts: exact cell maxima of the full maps, edge cells clipped
    for B in (2, 8, 64):
        for key in ((0, 0, 0), (0, 1, 1), (ns - 1, 2, 2), (min(1, ns - 1), 0, 1)):
            cells, norms = b.ssimulacra2_maps(*key, 0, n, B)
            assert cells.tobytes() == S.cell_max(reads[key][0], B).tobytes(), (key, B)
            assert norms.tobytes() == reads[key][1].tobytes()
    # a sub-range reads the same pairs
    if n > 2:
        m, nr = b.ssimulacra2_maps(0, 1, 2, 1, n - 2)
        assert m.tobytes() == reads[(0, 1, 2)][0][1:n - 1].tobytes() and nr.tobytes() == reads[(0, 1, 2)][1][1:n - 1].tobytes()
    b.close()


def test_xyb_roundtrip_batch(ce, gpu_ctx, workloads, shim):
    w, h = 97, 61
    b, refs, pairs = _build_batch(ce, gpu_ctx, workloads, w, h, (2, 2))
    n = len(pairs)
    cfg = ce.MetricConfig.ssimulacra2_only().with_xyb_roundtrip()
    plain = b.run(n, cfg)
    flagged = b.run(n, cfg, ssimulacra2_maps=True)
    assert [_score_tuple(s) for s in flagged] == [_score_tuple(s) for s in plain]
    ns = len(ce.ssimulacra2_scales(w, h))
    reads = _read_all(b, ns, 0, n)
    for q, (r, t) in enumerate(pairs):
        rt = gpu_ctx.xyb_roundtrip(refs[r], w, h).reshape(h, w, 3)
        _check_pair(shim, rt, t, w, h, _pair_scales(reads, ns, q), ("xyb", q))
    b.close()


def test_reference_handle_and_one_pair_paths_agree(ce, gpu_ctx, workloads):
    w, h = 129, 65
    ref = workloads.make_reference(w, h, 11)
    tests = [workloads.distort(ref, q) for q in (20, 50, 85)]
    ns = len(ce.ssimulacra2_scales(w, h))
    b = ce.Batch(gpu_ctx, w, h, 1, len(tests))
    b.set_reference(0, ref)
    for i, t in enumerate(tests):
        b.set_test(i, 0, t)
    b.run(len(tests), ce.MetricConfig.ssimulacra2_only(), ssimulacra2_maps=True)
    want = _read_all(b, ns, 0, len(tests))
    handle = ce.ReferenceHandle(gpu_ctx, ref, w, h, ssimulacra2_maps=True)
    for rnd in range(2):  # the second round runs on the cached reference pyramid
        res = handle.compare_many(tests)
        got = _read_all(handle, ns, 0, len(tests))
        for key in want:
            assert got[key][0].tobytes() == want[key][0].tobytes() and got[key][1].tobytes() == want[key][1].tobytes(), (rnd, key)
        for i, t in enumerate(tests):
            handle.compare(t)
            one = _read_all(handle, ns, 0, 1)
            for key in want:
                assert one[key][0][0].tobytes() == want[key][0][i].tobytes() and one[key][1][0].tobytes() == want[key][1][i].tobytes()
            score, feats, scales = gpu_ctx.calculate_ssimulacra2_with_maps(ref, t, w, h)
            assert score == res[i].ssimulacra2
            for s in range(ns):
                for c in range(3):
                    for k in range(3):
                        assert scales[s][c, k].tobytes() == want[(s, c, k)][0][i].tobytes()
                        assert feats[s, c, 2 * k:2 * k + 2].tobytes() == want[(s, c, k)][1][i].tobytes()
    assert handle.stats()[0] == 1
    handle.close()
    b.close()


def test_error_paths(ce, gpu_ctx, workloads):
    w, h = 97, 61
    L = ce.lib()
    b, refs, pairs = _build_batch(ce, gpu_ctx, workloads, w, h, (2,))
    n = len(pairs)
    ns = len(ce.ssimulacra2_scales(w, h))
    sw, sh = ce.ssimulacra2_scales(w, h)[0]
    buf = np.zeros(n * sw * sh, np.float32)
    norms = np.zeros((n, 2), np.float64)

    def call(scale=0, channel=0, kind=0, first=0, count=n, block=1, maps=True, floats=None, nrm=True):
        f = (n * sw * sh if floats is None else floats) if maps else 0
        return L.ce_batch_ssimulacra2_maps(b._h, scale, channel, kind, first, count, block, buf.ctypes.data if maps else None, f,
                                           norms.ctypes.data if nrm else None)

    assert call() == ce.CE_ERR_INVALID_ARG  # nothing launched yet
    b.run(n, ce.MetricConfig.ssimulacra2_only(), ssimulacra2_maps=True)
    assert call() == ce.CE_OK and call(maps=False) == ce.CE_OK and call(nrm=False) == ce.CE_OK
    bad = [dict(scale=ns), dict(scale=ns, maps=False), dict(channel=3), dict(kind=3), dict(count=0), dict(first=1), dict(first=n, count=1),
           dict(block=3), dict(block=128), dict(block=0), dict(floats=n * sw * sh - 1), dict(maps=False, nrm=False)]
    for kw in bad:
        assert call(**kw) == ce.CE_ERR_INVALID_ARG, kw
        assert gpu_ctx._err(), kw
    # an unflagged launch keeps the norms readable, not the maps
    b.run(n, ce.MetricConfig.ssimulacra2_only())
    assert call() == ce.CE_ERR_INVALID_ARG and "CE_FLAG_SSIMULACRA2_MAPS" in gpu_ctx._err()
    assert call(maps=False) == ce.CE_OK
    with pytest.raises(ce.CodecEvalError):
        b.ssimulacra2_maps(0, 0, 0, 0, n)
    _, nr = b.ssimulacra2_maps(0, 0, 0, 0, n, maps=False)
    assert nr.tobytes() == norms.tobytes()
    # a launch without SSIMULACRA2 leaves neither
    b.run(n, ce.MetricConfig(psnr=True))
    assert call(maps=False) == ce.CE_ERR_INVALID_ARG
    # a limited pyramid limits the readable scales
    b.debug_limit_scales(2)
    b.run(n, ce.MetricConfig.ssimulacra2_only(), ssimulacra2_maps=True)
    assert call(scale=1, floats=n * ce.ssimulacra2_scales(w, h)[1][0] * ce.ssimulacra2_scales(w, h)[1][1]) == ce.CE_OK
    assert call(scale=2, maps=False) == ce.CE_ERR_INVALID_ARG
    b.close()
    # the pooled paths reject the flag
    s = ce.CeScores()
    r, t = refs[0].reshape(-1), pairs[0][1].reshape(-1)
    assert L.ce_eval_pair(gpu_ctx._h, r.ctypes.data, r.size, t.ctypes.data, t.size, w, h, ce.METRIC_SSIMULACRA2, ce.FLAG_SSIMULACRA2_MAPS,
                          80.0, ctypes.byref(s)) == ce.CE_ERR_INVALID_ARG
    assert "CE_FLAG_SSIMULACRA2_MAPS" in gpu_ctx._err()
    d = ce.CePairDesc(r.ctypes.data, r.size, t.ctypes.data, t.size, w, h)
    assert L.ce_eval_batch(gpu_ctx._h, 1, ctypes.byref(d), ce.METRIC_SSIMULACRA2, ce.FLAG_SSIMULACRA2_MAPS, 80.0, ctypes.byref(s)) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_batch_lut(gpu_ctx._h, 1, ctypes.byref(d), None, ce.METRIC_SSIMULACRA2, ce.FLAG_SSIMULACRA2_MAPS, 80.0,
                               ctypes.byref(s)) == ce.CE_ERR_INVALID_ARG
    # the one-pair call: length and dimension errors first, as ce_calculate_ssimulacra2, then the map size
    feats = np.zeros(108, np.float64)
    total = 9 * sum(a * c for a, c in ce.ssimulacra2_scales(w, h))
    mp = np.zeros(total, np.float32)
    sc = ctypes.c_double()

    def one(rl=r.size, tl=t.size, ww=w, hh=h, floats=total):
        return L.ce_calculate_ssimulacra2_maps(gpu_ctx._h, r.ctypes.data, rl, t.ctypes.data, tl, ww, hh, ctypes.byref(sc), feats.ctypes.data,
                                               mp.ctypes.data, floats)

    def leaf(rl=r.size, tl=t.size, ww=w, hh=h):
        return L.ce_calculate_ssimulacra2(gpu_ctx._h, r.ctypes.data, rl, t.ctypes.data, tl, ww, hh, ctypes.byref(sc))

    for kw in (dict(tl=t.size - 3), dict(rl=r.size - 3, tl=r.size - 3), dict(ww=w - 1), dict(ww=0), dict(hh=0)):
        assert one(**kw) == leaf(**kw) != ce.CE_OK, kw
    small = np.zeros(7 * 9 * 3, np.uint8)
    assert L.ce_calculate_ssimulacra2_maps(gpu_ctx._h, small.ctypes.data, small.size, small.ctypes.data, small.size, 7, 9, ctypes.byref(sc),
                                           feats.ctypes.data, mp.ctypes.data, 0) == ce.CE_ERR_TOO_SMALL
    assert L.ce_calculate_ssimulacra2(gpu_ctx._h, small.ctypes.data, small.size, small.ctypes.data, small.size, 7, 9,
                                      ctypes.byref(sc)) == ce.CE_ERR_TOO_SMALL
    assert one(floats=total - 1) == ce.CE_ERR_INVALID_ARG and one(floats=total + 9) == ce.CE_ERR_INVALID_ARG
    assert one() == ce.CE_OK


def test_cpp_mirror(ce, gpu_ctx, workloads, tmp_path):
    """tests/cpp/test_ssim2_maps_mirror.cpp: calculate_ssimulacra2_with_maps of the C++ host mirror, built with g++ as
    test_host_cpp.py builds its programs, returns what the Python binding returns."""
    exe = str(tmp_path / "test_ssim2_maps_mirror")
    libdir = os.path.dirname(ce.LIB_PATH)
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "host"),
        os.path.join(ROOT, "tests", "cpp", "test_ssim2_maps_mirror.cpp"), "-o", exe,
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
    score, feats, scales = gpu_ctx.calculate_ssimulacra2_with_maps(ref, t, w, h)
    lines = r.stdout.strip().splitlines()
    assert float.fromhex(lines[0]) == score
    got = np.array([float.fromhex(x) for x in lines[1:109]])
    assert got.tobytes() == feats.reshape(-1).tobytes()
    assert len(lines) == 109 + len(scales)
    for s, m in enumerate(scales):
        assert lines[109 + s].split() == [str(m.shape[3]), str(m.shape[2])]
        assert (out_dir / f"scale{s}.f32").read_bytes() == m.tobytes()


def test_report_edge_deviation():
    """The largest relative deviation of an artifact / detail-lost value from the oracle's f64 value rounded to f32, over
    the tests above (they run first in this module)."""
    print(f"\nSSIMULACRA2 maps: largest artifact / detail-lost deviation {MAX_EDGE_DEV[0]:.3e} "
          f"({MAX_EDGE_DEV[0] / 2.0 ** -24:.1f} x 2^-24)")
    assert MAX_EDGE_DEV[0] <= EDGE_REL
