"""Builds and loads tests/cpp/ba_diffmap_shim.c: the CPU oracle's Butteraugli diffmap, for the diffmap tests.  Compiled into
a caller's directory with the CFLAGS of oracle/Makefile and -I oracle."""
import ctypes as C
import os
import re
import shlex
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ba_diffmap_shim.c")
ORACLE = os.path.join(ROOT, "oracle")
BA_MALTA_F32, BA_L2_EARLY = 5, 8  # ce_oracle.h: CEO_V_BA_MALTA_F32, CEO_V_BA_L2_EARLY


def oracle_cflags():
    text = open(os.path.join(ORACLE, "Makefile")).read()
    return shlex.split(re.search(r"^CFLAGS\s*\?=\s*(.*)$", text, flags=re.M).group(1))


class Shim:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libba_diffmap_shim.so")
        subprocess.check_call(["gcc", *oracle_cflags(), "-shared", "-Wl,-Bsymbolic", "-I", ORACLE, "-o", so, SRC, "-lm"])
        self.lib = L = C.CDLL(so)
        u8p, f32p, f64p, sz = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_size_t
        L.shim_set_variant.argtypes, L.shim_set_variant.restype = [C.c_int, C.c_int], None
        L.shim_butteraugli_diffmap.argtypes = [u8p, u8p, sz, sz, C.c_float, f32p]
        L.ceo_butteraugli.argtypes = [u8p, sz, u8p, sz, sz, sz, C.c_float, f64p, f64p]

    def set_device_switches(self, on: bool):
        """The two switches with which the oracle is the device's arithmetic (tests/test_gpu_butteraugli.py)."""
        for k in (BA_MALTA_F32, BA_L2_EARLY):
            self.lib.shim_set_variant(k, int(on))

    def diffmap(self, ref, test, w, h, intensity_target=80.0) -> np.ndarray:
        r, t = np.ascontiguousarray(ref, np.uint8).reshape(-1), np.ascontiguousarray(test, np.uint8).reshape(-1)
        out = np.empty((h, w), np.float32)
        rc = self.lib.shim_butteraugli_diffmap(r.ctypes.data_as(C.POINTER(C.c_uint8)), t.ctypes.data_as(C.POINTER(C.c_uint8)), w, h,
                                               intensity_target, out.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == 0, rc
        return out

    def score(self, ref, test, w, h, intensity_target=80.0):
        """ceo_butteraugli of this copy (same switches as diffmap): (score, pnorm3)."""
        r, t = np.ascontiguousarray(ref, np.uint8).reshape(-1), np.ascontiguousarray(test, np.uint8).reshape(-1)
        s, p = C.c_double(), C.c_double()
        rc = self.lib.ceo_butteraugli(r.ctypes.data_as(C.POINTER(C.c_uint8)), r.size, t.ctypes.data_as(C.POINTER(C.c_uint8)), t.size, w, h,
                                      intensity_target, C.byref(s), C.byref(p))
        assert rc == 0, rc
        return s.value, p.value


def pnorm3(dm: np.ndarray) -> float:
    """libjxl's p-norm of a diffmap in f64, as the oracle sums it (pixel order)."""
    d = dm.astype(np.float64).reshape(-1)
    d3 = d * d * d
    d6 = d3 * d3
    n = d.size
    s3, s6, s12 = float(np.sum(d3)), float(np.sum(d6)), float(np.sum(d6 * d6))
    return ((s3 / n) ** (1 / 3) + (s6 / n) ** (1 / 6) + (s12 / n) ** (1 / 12)) / 3.0


def block_max(dm: np.ndarray, B: int) -> np.ndarray:
    """[.., h, w] -> [.., ceil(h / B), ceil(w / B)] cell maxima, edge cells clipped to the image."""
    h, w = dm.shape[-2:]
    bh, bw = -(-h // B), -(-w // B)
    pad = np.full(dm.shape[:-2] + (bh * B, bw * B), -np.inf, np.float32)
    pad[..., :h, :w] = dm
    return pad.reshape(dm.shape[:-2] + (bh, B, bw, B)).max(axis=(-3, -1))
