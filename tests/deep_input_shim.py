"""Builds and loads tests/cpp/deep_input_shim.c: the CPU oracle's metrics on deep input (packed uint16 RGB of a declared
depth per side), for the deep-input tests.  Compiled into a caller's directory with the CFLAGS of oracle/Makefile and
-I oracle.  Also the host helpers the tests share: the PSNR expression, to_8bit, and the image generators."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from ba_diffmap_shim import ORACLE, ROOT, oracle_cflags

SRC = os.path.join(ROOT, "tests", "cpp", "deep_input_shim.c")
DEPTHS = (8, 10, 12, 16)


def _u16(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, np.uint16).reshape(-1))


def _p16(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


class Shim:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libdeep_input_shim.so")
        subprocess.check_call(["gcc", *oracle_cflags(), "-shared", "-Wl,-Bsymbolic", "-I", ORACLE, "-o", so, SRC, "-lm"])
        self.lib = L = C.CDLL(so)
        u16p, f32p, f64p, sz, u32 = C.POINTER(C.c_uint16), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_size_t, C.c_uint32
        L.shim_deep_table.argtypes, L.shim_deep_table.restype = [u32, C.c_int, f32p], None
        L.shim_deep_sse.argtypes, L.shim_deep_sse.restype = [u16p, u16p, sz], C.c_uint64
        L.shim_deep_ssimulacra2.argtypes = [u16p, u32, u16p, u32, sz, sz, C.c_int, f64p]
        L.shim_deep_dssim.argtypes = [u16p, u32, u16p, u32, sz, sz, f64p]
        L.shim_deep_butteraugli.argtypes = [u16p, u32, u16p, u32, sz, sz, C.c_float, f64p, f64p]

    def table(self, depth: int, rule: int) -> np.ndarray:
        """rule 0: the f64 curve rounded to f32 (SSIMULACRA2, Butteraugli); 1: f32 powf (DSSIM)."""
        out = np.empty(1 << depth, np.float32)
        self.lib.shim_deep_table(depth, rule, out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def sse(self, a, b) -> int:
        x, y = _u16(a), _u16(b)
        assert x.size == y.size
        return int(self.lib.shim_deep_sse(_p16(x), _p16(y), x.size))

    def ssimulacra2(self, ref, rd, test, td, w, h, blur_mode=1) -> float:
        r, t, out = _u16(ref), _u16(test), C.c_double()
        rc = self.lib.shim_deep_ssimulacra2(_p16(r), rd, _p16(t), td, w, h, blur_mode, C.byref(out))
        assert rc == 0, rc
        return out.value

    def dssim(self, ref, rd, test, td, w, h) -> float:
        r, t, out = _u16(ref), _u16(test), C.c_double()
        rc = self.lib.shim_deep_dssim(_p16(r), rd, _p16(t), td, w, h, C.byref(out))
        assert rc == 0, rc
        return out.value

    def butteraugli(self, ref, rd, test, td, w, h, intensity_target=80.0):
        """-> (score, 3-norm)"""
        r, t, s, p = _u16(ref), _u16(test), C.c_double(), C.c_double()
        rc = self.lib.shim_deep_butteraugli(_p16(r), rd, _p16(t), td, w, h, intensity_target, C.byref(s), C.byref(p))
        assert rc == 0, rc
        return s.value, p.value


def psnr_from_sse(sse: int, w: int, h: int, depth: int) -> float:
    """calculate_psnr's f64 expression with 255 replaced by 2^depth - 1, from the exact integer SSE (the host's libm)."""
    maxv = float((1 << depth) - 1)
    mse = float(sse) / float(w * h * 3)
    if mse == 0.0:
        return math.inf
    return 10.0 * math.log10(maxv * maxv / mse)


def to_8bit(v: np.ndarray) -> np.ndarray:
    """to_8bit of a 10-bit sample, as CE_PIXEL_RGB16_10BIT applies it: ((v * 255 + 512) / 1023).min(255)."""
    return np.minimum((v.astype(np.uint32) * 255 + 512) // 1023, 255).astype(np.uint8)


# ---- images -----------------------------------------------------------------------------------------------------------
def random_pair(w, h, depth_r, depth_t, seed):
    """Independent smooth-ish random content: a reference and a noisy copy, each quantised to its own depth."""
    rng = np.random.default_rng(seed)
    base = rng.random((h, w, 3))
    test = np.clip(base + rng.normal(0.0, 0.02, base.shape), 0.0, 1.0)
    return quantise(base, depth_r), quantise(test, depth_t)


def gradient_noise_pair(w, h, depth_r, depth_t, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x / max(w - 1, 1), y / max(h - 1, 1), (x + y) / max(w + h - 2, 1)], axis=-1)
    base = np.clip(base + rng.normal(0.0, 0.01, base.shape), 0.0, 1.0)
    test = np.clip(base + rng.normal(0.0, 0.004, base.shape), 0.0, 1.0)
    return quantise(base, depth_r), quantise(test, depth_t)


def blocky_pair(w, h, depth_r, depth_t, seed):
    """The test is the reference with every 8 x 8 block pulled towards its mean (a coarse-quantisation look)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.3 * np.sin(x / 7.0)[..., None] * np.cos(y / 5.0)[..., None] + rng.normal(0.0, 0.03, (h, w, 3))
    base = np.clip(base, 0.0, 1.0)
    test = base.copy()
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            blk = test[by:by + 8, bx:bx + 8]
            blk[...] = 0.5 * blk + 0.5 * blk.mean(axis=(0, 1), keepdims=True)
    return quantise(base, depth_r), quantise(test, depth_t)


def quantise(img01: np.ndarray, depth: int) -> np.ndarray:
    maxv = (1 << depth) - 1
    return np.round(img01 * maxv).astype(np.uint16)
