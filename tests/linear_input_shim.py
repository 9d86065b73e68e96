"""Builds and loads tests/cpp/linear_input_shim.c: the CPU oracle's metrics on linear input (packed float32 RGB, linear
light with sRGB primaries, any range), for the linear-input tests.  Compiled into a caller's directory with the CFLAGS of
oracle/Makefile and -I oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

from ba_diffmap_shim import ORACLE, ROOT, oracle_cflags

SRC = os.path.join(ROOT, "tests", "cpp", "linear_input_shim.c")


def _f32(a) -> np.ndarray:
    a = np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a.reshape(-1))


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Shim:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "liblinear_input_shim.so")
        subprocess.check_call(["gcc", *oracle_cflags(), "-shared", "-Wl,-Bsymbolic", "-I", ORACLE, "-o", so, SRC, "-lm"])
        self.lib = L = C.CDLL(so)
        f32p, f64p, sz = C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_size_t
        L.shim_linear_ssimulacra2.argtypes = [f32p, f32p, sz, sz, C.c_int, f64p]
        L.shim_linear_dssim.argtypes = [f32p, f32p, sz, sz, f64p]
        L.shim_linear_butteraugli.argtypes = [f32p, f32p, sz, sz, C.c_float, f64p, f64p]

    def ssimulacra2(self, ref, test, w, h, blur_mode=1) -> float:
        r, t, out = _f32(ref), _f32(test), C.c_double()
        rc = self.lib.shim_linear_ssimulacra2(_p(r), _p(t), w, h, blur_mode, C.byref(out))
        assert rc == 0, rc
        return out.value

    def dssim(self, ref, test, w, h) -> float:
        r, t, out = _f32(ref), _f32(test), C.c_double()
        rc = self.lib.shim_linear_dssim(_p(r), _p(t), w, h, C.byref(out))
        assert rc == 0, rc
        return out.value

    def butteraugli(self, ref, test, w, h, intensity_target=80.0):
        """-> (score, 3-norm)"""
        r, t, s, p = _f32(ref), _f32(test), C.c_double(), C.c_double()
        rc = self.lib.shim_linear_butteraugli(_p(r), _p(t), w, h, intensity_target, C.byref(s), C.byref(p))
        assert rc == 0, rc
        return s.value, p.value
