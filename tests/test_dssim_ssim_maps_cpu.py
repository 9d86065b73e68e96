"""DSSIM's SsimMap without a GPU: the four entry points and CE_DSSIM_MAX_LEVELS agree across the header, the Rust
declarations and the ctypes layer and reject null handles; ce_dssim_levels (a host function) is create_image's level rule;
and the oracle's maps (the shim of dssim_map_shim.py, which the GPU tests compare the device's maps with) reduce to the
oracle's own per-scale scores and score."""
import ctypes
import os
import re

import numpy as np
import pytest

import dssim_map_shim as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
DEBUG_HEADER = open(os.path.join(ROOT, "include", "ce_metrics_debug.h")).read()
SYS = open(os.path.join(ROOT, "bindings", "rust", "codec-eval-hip", "src", "sys.rs")).read()
NEW = {"ce_dssim_levels": 5, "ce_calculate_dssim_ssim_maps": 11, "ce_batch_dssim_ssim_maps": 8, "ce_ref_dssim_ssim_maps": 8}


def test_declared_everywhere_with_the_same_arity(ce):
    header = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, arity in NEW.items():
        c = re.search(r"\b" + name + r"\(([^;]*?)\);", header, flags=re.S)
        r = re.search(r"pub fn " + name + r"\((.*?)\)\s*->", SYS, flags=re.S)
        assert c and r, name
        assert len(c.group(1).split(",")) == arity and len([a for a in r.group(1).split(",") if a.strip()]) == arity, name
        assert name in ce.ABI_SYMBOLS and hasattr(ce.lib(), name)
        assert len(getattr(ce.lib(), name).argtypes) == arity
    assert int(re.search(r"#define CE_DSSIM_MAX_LEVELS (\d+)", HEADER).group(1)) == 5
    assert int(re.search(r"pub const CE_DSSIM_MAX_LEVELS: usize = (\d+);", SYS).group(1)) == 5
    assert ce.DSSIM_MAX_LEVELS == 5 == len(S.WEIGHTS)


def test_walk_rows_hook_is_declared_everywhere_with_the_same_arity(ce):
    """ce_debug_dssim_walk_rows (the test hook that forces the streaming kernels' walk length) in the debug header, the
    Rust declarations and the ctypes layer, with the Batch method the GPU tests call."""
    name = "ce_debug_dssim_walk_rows"
    c = re.search(r"\bint " + name + r"\(([^;]*?)\);", re.sub(r"/\*.*?\*/", "", DEBUG_HEADER, flags=re.S), flags=re.S)
    r = re.search(r"pub fn " + name + r"\((.*?)\)\s*->\s*c_int;", SYS, flags=re.S)
    assert c and r
    assert [a.split()[-1].lstrip("*") for a in c.group(1).split(",")] == ["b", "rows"]
    assert [a.split(":")[0].strip() for a in r.group(1).split(",")] == ["b", "rows"]
    assert "uint32_t rows" in c.group(1) and "rows: u32" in r.group(1)
    assert name in ce.ABI_SYMBOLS and hasattr(ce.lib(), name)
    assert len(getattr(ce.lib(), name).argtypes) == 2
    assert callable(getattr(ce.Batch, "debug_dssim_walk_rows", None))


def test_null_handles_are_invalid_arguments(ce):
    L = ce.lib()
    a = np.zeros(16 * 16 * 3, np.uint8)
    maps = np.zeros(16 * 16 + 8 * 8, np.float32)
    lv = np.zeros(5, np.float64)
    d = ctypes.c_double()
    assert L.ce_calculate_dssim_ssim_maps(None, a.ctypes.data, a.size, a.ctypes.data, a.size, 16, 16, ctypes.byref(d), lv.ctypes.data,
                                          maps.ctypes.data, maps.size) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_dssim_ssim_maps(None, 0, 0, 1, 1, maps.ctypes.data, 256, lv.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ref_dssim_ssim_maps(None, 0, 0, 1, 1, maps.ctypes.data, 256, lv.ctypes.data) == ce.CE_ERR_INVALID_ARG
    for rows in (0, 2, 64, 3, 128):  # a null batch is rejected whatever the walk length
        assert L.ce_debug_dssim_walk_rows(None, rows) == ce.CE_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.Shim(tmp_path_factory.mktemp("dssim_shim"))


LEVEL_SHAPES = [(1, 1), (7, 9), (9, 7), (8, 8), (9, 301), (15, 17), (16, 16), (31, 16), (32, 32), (59, 9), (64, 63), (100, 7),
                (127, 128), (128, 128), (255, 129), (768, 512), (512, 768), (4096, 4096), (4095, 17), (1, 4096), (65535, 8)]


@pytest.mark.parametrize("w,h", LEVEL_SHAPES)
def test_levels_are_create_images_rule(ce, shim, w, h):
    want = shim.levels(w, h)
    assert ce.dssim_levels(w, h) == want
    n, lw, lh = ctypes.c_uint32(), (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)()
    assert ce.lib().ce_dssim_levels(w, h, ctypes.byref(n), lw, lh) == ce.CE_OK
    assert [(lw[l], lh[l]) for l in range(n.value)] == want
    assert 1 <= n.value <= 5


def test_levels_reject_zero_sizes_and_null_pointers(ce):
    L = ce.lib()
    n, lw, lh = ctypes.c_uint32(), (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)()
    for w, h in ((0, 5), (5, 0), (0, 0)):
        assert L.ce_dssim_levels(w, h, ctypes.byref(n), lw, lh) == ce.CE_ERR_INVALID_ARG
        with pytest.raises(ce.CodecEvalError):
            ce.dssim_levels(w, h)
    assert L.ce_dssim_levels(8, 8, None, lw, lh) == ce.CE_ERR_INVALID_ARG
    assert L.ce_dssim_levels(8, 8, ctypes.byref(n), None, lh) == ce.CE_ERR_INVALID_ARG
    assert L.ce_dssim_levels(8, 8, ctypes.byref(n), lw, None) == ce.CE_ERR_INVALID_ARG


@pytest.mark.parametrize("w,h", [(97, 61), (9, 301), (7, 9), (1, 1), (64, 64), (200, 136)])
def test_shim_maps_reduce_to_the_oracle_scores(shim, workloads, oracle, w, h):
    ref = workloads.make_reference(w, h, 60 + w)
    for q in (30, 75, 95):
        t = workloads.distort(ref, q)
        d, levels = shim.maps(ref, t, w, h)
        want_d, want_scores = oracle.dssim_detail(ref, t, w, h)
        assert [(m.shape[1], m.shape[0]) for m, _ in levels] == shim.levels(w, h)
        assert all(m.dtype == np.float32 for m, _ in levels)
        assert np.array([s for _, s in levels]).tobytes() == want_scores.tobytes()  # bit for bit
        assert d == want_d == oracle.dssim(ref, t, w, h)
        assert S.dssim_from_scores([s for _, s in levels]) == d


def test_shim_identical_images_give_maps_of_one(shim, workloads):
    ref = workloads.make_reference(40, 24, 5)
    d, levels = shim.maps(ref, ref, 40, 24)
    assert d == 0.0
    for m, s in levels:
        assert np.all(m == 1.0) and s == 1.0


def test_block_min_helper():
    m = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
    got = S.block_min(m, 4)
    assert got.shape == (2, 2)
    assert got.tolist() == [[m[:4, :4].min(), m[:4, 4:].min()], [m[4:, :4].min(), m[4:, 4:].min()]]
