"""Deep input (10-, 12- and 16-bit images at their own precision), the parts that need no GPU: the shim that is the CPU side
of tests/test_gpu_deep_input.py is pinned to the oracle, the two exactness anchors of DESIGN.md section 11 are checked on
the tables, and the new ABI is declared everywhere it has to be."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deep_input_shim as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory, oracle):
    return D.Shim(tmp_path_factory.mktemp("deep_input_shim"))


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_depth8_tables_are_the_oracles(shim, oracle):
    assert np.array_equal(bits(shim.table(8, 0)), bits(oracle.ssim2_srgb_lut()))
    powf = np.array([oracle.srgb_u8_to_linear(i) for i in range(256)], np.float32)
    assert np.array_equal(bits(shim.table(8, 1)), bits(powf))


@pytest.mark.parametrize("rule", [0, 1])
def test_depth16_entries_257v_are_the_depth8_entries(shim, rule):
    """Anchor 2: v8 * 257 / 65535 and v8 / 255 are the same real number, both operands are exact in f32 and f64 and the
    division is correctly rounded - so the tables agree entry for entry, in both rules."""
    assert np.array_equal(bits(shim.table(16, rule)[::257]), bits(shim.table(8, rule)))


@pytest.mark.parametrize("depth", D.DEPTHS)
def test_tables_are_monotone_and_span_0_1(shim, depth):
    for rule in (0, 1):
        t = shim.table(depth, rule)
        assert t.size == 1 << depth and t[0] == 0.0 and t[-1] == 1.0 and np.all(np.diff(t.astype(np.float64)) >= 0.0)


@pytest.mark.parametrize("w,h,seed", [(37, 29, 1), (64, 48, 2), (9, 8, 3)])
def test_shim_on_depth8_samples_is_the_oracle_bit_for_bit(shim, oracle, w, h, seed):
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    t = np.clip(r.astype(np.int32) + rng.integers(-12, 13, r.shape), 0, 255).astype(np.uint8)
    r16, t16 = r.astype(np.uint16), t.astype(np.uint16)
    for mode in (0, 1):
        assert shim.ssimulacra2(r16, 8, t16, 8, w, h, mode) == oracle.ssimulacra2(r, t, w, h, mode)
    assert shim.dssim(r16, 8, t16, 8, w, h) == oracle.dssim(r, t, w, h)
    assert shim.butteraugli(r16, 8, t16, 8, w, h) == oracle.butteraugli(r, t, w, h)
    assert shim.sse(r16, t16) == oracle.sse(r, t)
    assert D.psnr_from_sse(shim.sse(r16, t16), w, h, 8) == oracle.psnr(r, t, w, h)
    # anchor 2 on whole images: the same pictures as depth-16 samples v8 * 257
    assert shim.ssimulacra2(r16 * 257, 16, t16 * 257, 16, w, h, 1) == oracle.ssimulacra2(r, t, w, h, 1)
    assert shim.dssim(r16 * 257, 16, t16, 8, w, h) == oracle.dssim(r, t, w, h)
    assert shim.butteraugli(r16, 8, t16 * 257, 16, w, h) == oracle.butteraugli(r, t, w, h)


def test_shim_clamps_samples_above_the_depth(shim):
    rng = np.random.default_rng(5)
    r = rng.integers(0, 1024, (16, 16, 3)).astype(np.uint16)
    t = rng.integers(0, 1024, (16, 16, 3)).astype(np.uint16)
    over = t.copy()
    over[t == 1023] = 40000
    over[0, 0, :] = 65535
    t[0, 0, :] = 1023
    assert shim.ssimulacra2(r, 10, over, 10, 16, 16) == shim.ssimulacra2(r, 10, t, 10, 16, 16)
    assert shim.dssim(r, 10, over, 10, 16, 16) == shim.dssim(r, 10, t, 10, 16, 16)


def test_a_ramp_differs_below_the_8bit_step(shim):
    """The CPU half of 'the test that fails today': pairs that to_8bit maps to the same bytes are not the same image."""
    ref, test, changed = below_8bit_step_pair(64, 48)
    assert changed >= 0.25
    assert np.array_equal(D.to_8bit(ref), D.to_8bit(test)) and not np.array_equal(ref, test)
    assert shim.sse(ref, test) > 0
    assert shim.dssim(ref, 10, test, 10, 64, 48) > 0.0
    assert shim.butteraugli(ref, 10, test, 10, 64, 48)[0] > 0.0
    assert shim.ssimulacra2(ref, 10, test, 10, 64, 48) < 100.0


def below_8bit_step_pair(w, h):
    """A smooth 10-bit ramp and a copy moved by +-1 LSB wherever to_8bit does not notice; the share of samples moved."""
    y, x = np.mgrid[0:h, 0:w]
    ref = np.stack([(x * 1023) // max(w - 1, 1), (y * 1023) // max(h - 1, 1), ((x + y) * 1023) // max(w + h - 2, 1)], axis=-1).astype(np.uint16)
    up = np.minimum(ref.astype(np.int32) + 1, 1023).astype(np.uint16)
    down = np.maximum(ref.astype(np.int32) - 1, 0).astype(np.uint16)
    test = ref.copy()
    can_up = D.to_8bit(up) == D.to_8bit(ref)
    can_down = D.to_8bit(down) == D.to_8bit(ref)
    test[can_up] = up[can_up]
    only_down = can_down & ~can_up
    test[only_down] = down[only_down]
    return ref, test, float(np.mean(test != ref))


# ---- ABI ---------------------------------------------------------------------------------------------------------------
NEW = {"ce_pixel_bytes": 1, "ce_batch_create_deep": 8, "ce_estimate_batch_bytes_deep": 7, "ce_eval_pair_deep": 13}


def _header_functions():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ce_metrics.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^[A-Za-z_][A-Za-z0-9_ \*]*?\b(ce_[a-z0-9_]+)\(([^;{]*?)\);", text, flags=re.M | re.S):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
    return out


def test_new_symbols_are_declared_with_their_arity_everywhere(ce):
    hdr = _header_functions()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "codec-eval-hip", "src", "sys.rs")).read()
    protos = {p[0]: p for p in ce._PROTOTYPES}
    L = C.CDLL(ce.LIB_PATH)
    for name, arity in NEW.items():
        assert hdr[name] == arity, name
        assert hasattr(L, name), name
        assert len(protos[name][2]) == arity, name
        m = re.search(r"pub fn " + name + r"\((.*?)\)", sys_rs, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == arity, name
    for const, value in (("CE_PIXEL_RGB16", 4), ("CE_PIXEL_RGBA16", 5)):
        assert re.search(const + r"\s*=\s*%d\b" % value, open(os.path.join(ROOT, "include", "ce_metrics.h")).read())
        assert re.search(r"pub const " + const + r": c_int = %d;" % value, sys_rs)
    assert (ce.PIXEL_RGB16, ce.PIXEL_RGBA16) == (4, 5)


def test_pure_host_entry_points(ce):
    L = ce.lib()
    assert [L.ce_pixel_bytes(f) for f in range(7)] == [3, 4, 6, 8, 6, 8, 0]
    cfg = ce.MetricConfig.all()
    base = ce.estimate_batch_bytes(768, 512, 2, 8, cfg)
    deep = ce.estimate_batch_bytes_deep(768, 512, 2, 8, cfg, 10, 16)
    assert deep >= base + 3 * 768 * 512 * 10
    assert ce.estimate_batch_bytes_deep(768, 512, 2, 8, cfg, 9, 16) == 0
    assert ce.estimate_batch_bytes_deep(768, 512, 2, 8, cfg, 8, 14) == 0


def test_create_deep_argument_errors_need_no_device(ce):
    """Null handles are refused before anything touches a device."""
    L = ce.lib()
    out = C.c_void_p()
    assert L.ce_batch_create_deep(None, 16, 16, 1, 1, 10, 10, C.byref(out)) == ce.CE_ERR_INVALID_ARG
    assert L.ce_eval_pair_deep(None, None, 0, 10, None, 0, 10, 16, 16, 8, 0, 80.0, None) == ce.CE_ERR_INVALID_ARG


def test_session_image_data_deep(ce):
    import importlib

    S = importlib.import_module("codec-eval_amd.session")
    px = np.arange(2 * 3 * 3, dtype=np.uint16).reshape(2, 3, 3) * 50
    img = S.ImageData.rgb16(px, 3, 2, 10)
    assert img.depth == 10 and (img.width, img.height) == (3, 2)
    assert np.array_equal(img.to_rgb8_vec(), D.to_8bit(px).reshape(-1))
    rgba = np.concatenate([px, np.full((2, 3, 1), 1023, np.uint16)], axis=-1)
    assert np.array_equal(S.ImageData.rgba16(rgba, 3, 2, 10).to_rgb8_vec(), D.to_8bit(px).reshape(-1))
    with pytest.raises(ValueError):
        S.ImageData.rgb16(px, 3, 2, 9)
