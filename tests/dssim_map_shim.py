"""Builds and loads tests/cpp/dssim_map_shim.c: the CPU oracle's DSSIM SSIM maps (one per scale), for the SSIM map tests.
Compiled into a caller's directory with the CFLAGS of oracle/Makefile and -I oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

from ba_diffmap_shim import ORACLE, ROOT, oracle_cflags

SRC = os.path.join(ROOT, "tests", "cpp", "dssim_map_shim.c")
MAX_LEVELS = 5
WEIGHTS = (0.028, 0.197, 0.322, 0.298, 0.155)  # dssim-core's DEFAULT_WEIGHTS (oracle/dssim.c)


class Shim:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libdssim_map_shim.so")
        subprocess.check_call(["gcc", *oracle_cflags(), "-shared", "-Wl,-Bsymbolic", "-I", ORACLE, "-o", so, SRC, "-lm"])
        self.lib = L = C.CDLL(so)
        u8p, f32p, f64p, sz = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_size_t
        L.shim_dssim_levels.argtypes, L.shim_dssim_levels.restype = [sz, sz, C.POINTER(sz), C.POINTER(sz)], C.c_int
        L.shim_dssim_maps.argtypes = [u8p, u8p, sz, sz, C.POINTER(C.c_int), f32p, f64p, f64p]

    def levels(self, w, h):
        """[(w_l, h_l), ...]: create_image's scale sizes."""
        lw, lh = (C.c_size_t * MAX_LEVELS)(), (C.c_size_t * MAX_LEVELS)()
        n = self.lib.shim_dssim_levels(w, h, lw, lh)
        return [(int(lw[l]), int(lh[l])) for l in range(n)]

    def maps(self, ref, test, w, h):
        """(dssim, [(map [h_l, w_l] float32, score), ...]): every scale of Dssim::compare."""
        r, t = np.ascontiguousarray(ref, np.uint8).reshape(-1), np.ascontiguousarray(test, np.uint8).reshape(-1)
        sizes = self.levels(w, h)
        buf = np.empty(sum(a * b for a, b in sizes), np.float32)
        scores = np.zeros(MAX_LEVELS, np.float64)
        n, out = C.c_int(), C.c_double()
        rc = self.lib.shim_dssim_maps(r.ctypes.data_as(C.POINTER(C.c_uint8)), t.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, C.byref(n),
                                      buf.ctypes.data_as(C.POINTER(C.c_float)), scores.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
        assert rc == 0 and n.value == len(sizes), (rc, n.value, sizes)
        res, off = [], 0
        for l, (lw, lh) in enumerate(sizes):
            res.append((buf[off:off + lw * lh].reshape(lh, lw).copy(), float(scores[l])))
            off += lw * lh
        return out.value, res


def dssim_from_scores(scores) -> float:
    """Dssim::compare's weighting of per-scale scores and to_dssim, in f64 (oracle/dssim.c: compare)."""
    s = w = 0.0
    for l, v in enumerate(scores):
        s += v * WEIGHTS[l]
        w += WEIGHTS[l]
    ssim = s / w
    if not ssim > 2.220446049250313e-16:
        ssim = 2.220446049250313e-16
    return 1.0 / ssim - 1.0


def block_min(m: np.ndarray, B: int) -> np.ndarray:
    """[.., h, w] -> [.., ceil(h / B), ceil(w / B)] cell minima, edge cells clipped to the map."""
    h, w = m.shape[-2:]
    bh, bw = -(-h // B), -(-w // B)
    pad = np.full(m.shape[:-2] + (bh * B, bw * B), np.inf, np.float32)
    pad[..., :h, :w] = m
    return pad.reshape(m.shape[:-2] + (bh, B, bw, B)).min(axis=(-3, -1))
