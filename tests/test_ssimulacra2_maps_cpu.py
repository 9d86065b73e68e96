"""SSIMULACRA2's error maps without a GPU: the five entry points, CE_FLAG_SSIMULACRA2_MAPS and the ce_ssim2_map kinds
agree across the header, the Rust declarations and the ctypes layer, and reject null handles; ce_ssimulacra2_scales (a
host function) is the oracle's scale rule; and the oracle's maps (the shim of ssim2_map_shim.py, which the GPU tests
compare the device's maps with) pool to the oracle's own features and score."""
import ctypes
import os
import re

import numpy as np
import pytest

import ssim2_map_shim as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
SYS = open(os.path.join(ROOT, "bindings", "rust", "codec-eval-hip", "src", "sys.rs")).read()
NEW = {"ce_ssimulacra2_scales": 5, "ce_calculate_ssimulacra2_maps": 11, "ce_batch_ssimulacra2_maps": 10,
       "ce_ref_ssimulacra2_maps": 10}


def test_declared_everywhere_with_the_same_arity(ce):
    header = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, arity in NEW.items():
        c = re.search(r"\b" + name + r"\(([^;]*?)\);", header, flags=re.S)
        r = re.search(r"pub fn " + name + r"\((.*?)\)\s*->", SYS, flags=re.S)
        assert c and r, name
        assert len(c.group(1).split(",")) == arity and len([a for a in r.group(1).split(",") if a.strip()]) == arity, name
        assert name in ce.ABI_SYMBOLS and hasattr(ce.lib(), name)
        assert len(getattr(ce.lib(), name).argtypes) == arity
    assert int(re.search(r"#define CE_SSIM2_MAX_SCALES (\d+)", HEADER).group(1)) == 6
    assert int(re.search(r"pub const CE_SSIM2_MAX_SCALES: usize = (\d+);", SYS).group(1)) == 6
    assert ce.SSIM2_MAX_SCALES == 6 == S.MAX_SCALES
    assert int(re.search(r"CE_FLAG_SSIMULACRA2_MAPS = 1u << (\d+)", HEADER).group(1)) == 2
    assert int(re.search(r"pub const CE_FLAG_SSIMULACRA2_MAPS: u32 = 1 << (\d+);", SYS).group(1)) == 2
    assert ce.FLAG_SSIMULACRA2_MAPS == 4
    for k, name in enumerate(("SSIM", "ARTIFACT", "DETAIL_LOST")):
        assert int(re.search(r"CE_SSIM2_MAP_" + name + r" = (\d+)", HEADER).group(1)) == k
        assert int(re.search(r"pub const CE_SSIM2_MAP_" + name + r": u32 = (\d+);", SYS).group(1)) == k
        assert getattr(ce, "SSIM2_MAP_" + name) == k


def test_null_handles_are_invalid_arguments(ce):
    L = ce.lib()
    a = np.zeros(16 * 16 * 3, np.uint8)
    maps = np.zeros(9 * (16 * 16 + 8 * 8), np.float32)
    feats = np.zeros(108, np.float64)
    norms = np.zeros(2, np.float64)
    d = ctypes.c_double()
    assert L.ce_calculate_ssimulacra2_maps(None, a.ctypes.data, a.size, a.ctypes.data, a.size, 16, 16, ctypes.byref(d), feats.ctypes.data,
                                           maps.ctypes.data, maps.size) == ce.CE_ERR_INVALID_ARG
    for fn in (L.ce_batch_ssimulacra2_maps, L.ce_ref_ssimulacra2_maps):
        assert fn(None, 0, 0, 0, 0, 1, 1, maps.ctypes.data, 256, norms.ctypes.data) == ce.CE_ERR_INVALID_ARG
        assert fn(None, 0, 0, 0, 0, 1, 1, None, 0, norms.ctypes.data) == ce.CE_ERR_INVALID_ARG
        assert L.ce_last_error(None)  # a message without a context


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.Shim(tmp_path_factory.mktemp("ssim2_map_shim"))


def _rule(w, h):
    """The lineage's loop: test the size before halving (ceiling), at most six scales."""
    out = []
    for s in range(6):
        if w < 8 or h < 8:
            break
        if s:
            w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


SCALE_SHAPES = [(1, 1), (7, 7), (7, 8), (8, 7), (8, 8), (9, 9), (15, 15), (16, 16), (17, 17), (8, 1000), (1000, 8), (15, 16),
                (16, 17), (31, 33), (768, 512), (512, 768), (4096, 4096), (4095, 17), (65535, 8), (65537, 9)]


@pytest.mark.parametrize("w,h", SCALE_SHAPES)
def test_scales_are_the_lineage_rule(ce, shim, w, h):
    want = _rule(w, h)
    assert shim.scales(w, h) == want
    assert ce.ssimulacra2_scales(w, h) == want
    n, sw, sh = ctypes.c_uint32(), (ctypes.c_uint32 * 6)(), (ctypes.c_uint32 * 6)()
    assert ce.lib().ce_ssimulacra2_scales(w, h, ctypes.byref(n), sw, sh) == ce.CE_OK
    assert [(sw[s], sh[s]) for s in range(n.value)] == want
    assert n.value <= 6


def test_scale_edges():
    assert _rule(7, 100) == [] and _rule(8, 8) == [(8, 8), (4, 4)] and _rule(9, 9) == [(9, 9), (5, 5)]
    assert _rule(15, 15) == [(15, 15), (8, 8), (4, 4)] and _rule(16, 16) == [(16, 16), (8, 8), (4, 4)]
    assert _rule(17, 17) == [(17, 17), (9, 9), (5, 5)] and _rule(8, 1000) == [(8, 1000), (4, 500)]
    assert len(_rule(4096, 4096)) == 6 and _rule(4096, 4096)[-1] == (128, 128)


def test_scales_reject_zero_sizes_and_null_pointers(ce):
    L = ce.lib()
    n, sw, sh = ctypes.c_uint32(), (ctypes.c_uint32 * 6)(), (ctypes.c_uint32 * 6)()
    for w, h in ((0, 5), (5, 0), (0, 0)):
        assert L.ce_ssimulacra2_scales(w, h, ctypes.byref(n), sw, sh) == ce.CE_ERR_INVALID_ARG
        with pytest.raises(ce.CodecEvalError):
            ce.ssimulacra2_scales(w, h)
    assert L.ce_ssimulacra2_scales(8, 8, None, sw, sh) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ssimulacra2_scales(8, 8, ctypes.byref(n), None, sh) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ssimulacra2_scales(8, 8, ctypes.byref(n), sw, None) == ce.CE_ERR_INVALID_ARG


def _oracle_features(oracle, ref, t, w, h):
    """The oracle's avg with the SSIM term in its CEO_V_SSIM2_F32_POOL form (the device's) and the edge terms in the
    default form, blur mode 1."""
    _, edge = oracle.ssimulacra2_detail(ref, t, w, h, 1)
    oracle.set_variant("ssim2_f32_pool", 1)
    try:
        _, f32 = oracle.ssimulacra2_detail(ref, t, w, h, 1)
    finally:
        oracle.set_variant("ssim2_f32_pool", 0)
    avg = edge.copy()
    avg[..., 0:2] = f32[..., 0:2]
    return avg


def _close(a, b, rel):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300))


@pytest.mark.parametrize("w,h", [(97, 61), (8, 8), (9, 301), (15, 17), (64, 64), (200, 136)])
def test_shim_maps_pool_to_the_oracle(shim, workloads, oracle, w, h):
    ref = workloads.make_reference(w, h, 60 + w)
    for q in (30, 75, 95):
        t = workloads.distort(ref, q)
        scales = shim.maps(ref, t, w, h)
        assert [(d.shape[2], d.shape[1]) for d, _ in scales] == shim.scales(w, h) == _rule(w, h)
        assert all(d.dtype == np.float32 and e.dtype == np.float64 for d, e in scales)
        assert all(np.all(d >= 0) and np.all(e >= 0) and not np.any((e[:, 0] > 0) & (e[:, 1] > 0)) for d, e in scales)
        got = S.features(scales)
        want = _oracle_features(oracle, ref, t, w, h)
        assert got.shape == want.shape
        assert _close(got, want, 1e-12), np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
        assert abs(oracle.ssimulacra2_score(got) - oracle.ssimulacra2_score(want)) <= 1e-12 * abs(oracle.ssimulacra2_score(want))


def test_shim_identical_images_give_zero_maps(shim, workloads):
    ref = workloads.make_reference(40, 24, 5)
    for d, e in shim.maps(ref, ref, 40, 24):
        assert np.all(d == 0.0) and np.all(e == 0.0)


def test_cell_max_helper():
    m = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
    got = S.cell_max(m, 4)
    assert got.shape == (2, 2)
    assert got.tolist() == [[m[:4, :4].max(), m[:4, 4:].max()], [m[4:, :4].max(), m[4:, 4:].max()]]
