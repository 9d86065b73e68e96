"""Builds and loads tests/cpp/ssim2_rows_shim.c: the CPU oracle's SSIMULACRA2 row pass of the five blurred streams of one
XYB channel, for the row-stream tests.  Compiled into a caller's directory with the CFLAGS of oracle/Makefile and -I oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

from ba_diffmap_shim import ORACLE, ROOT, oracle_cflags

SRC = os.path.join(ROOT, "tests", "cpp", "ssim2_rows_shim.c")
STREAMS = 5  # {a, b, a*a, b*b, a*b}: CE_SSIM2_STREAMS


class Shim:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libssim2_rows_shim.so")
        subprocess.check_call(["gcc", *oracle_cflags(), "-shared", "-Wl,-Bsymbolic", "-I", ORACLE, "-o", so, SRC, "-lm"])
        self.lib = L = C.CDLL(so)
        f32p, sz = C.POINTER(C.c_float), C.c_size_t
        L.shim_ssim2_row_streams.argtypes = [f32p, f32p, sz, sz, f32p]
        L.shim_ssim2_col_pass.argtypes = [f32p, sz, sz, f32p]

    def row_streams(self, a: np.ndarray, b: np.ndarray) -> np.ndarray:
        """[5, h, w] float32: the row pass of a, b, a*a, b*b, a*b (a = the reference's XYB plane, b = the distorted one's)."""
        a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
        assert a.shape == b.shape and a.ndim == 2
        h, w = a.shape
        out = np.empty((STREAMS, h, w), np.float32)
        f32p = C.POINTER(C.c_float)
        rc = self.lib.shim_ssim2_row_streams(a.ctypes.data_as(f32p), b.ctypes.data_as(f32p), w, h, out.ctypes.data_as(f32p))
        assert rc == 0, rc
        return out

    def col_pass(self, plane: np.ndarray) -> np.ndarray:
        p = np.ascontiguousarray(plane, np.float32)
        h, w = p.shape
        out = np.empty_like(p)
        f32p = C.POINTER(C.c_float)
        rc = self.lib.shim_ssim2_col_pass(p.ctypes.data_as(f32p), w, h, out.ctypes.data_as(f32p))
        assert rc == 0, rc
        return out


def xyb_pyramid(oracle, rgb, w: int, h: int, scale: int) -> np.ndarray:
    """[3, h_s, w_s] float32: the oracle's positive XYB planes of `scale` (linear RGB, `scale` 2x2 box steps, XYB)."""
    lin = oracle.ssim2_linear_planar(rgb, w, h)
    for _ in range(scale):
        lin = oracle.ssim2_downscale(lin)
    return oracle.ssim2_xyb_positive(lin)
