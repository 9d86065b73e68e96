"""Builds and loads tests/cpp/ssim2_map_shim.c: the CPU oracle's SSIMULACRA2 per-pixel error maps (three per XYB channel
and scale), for the SSIMULACRA2 map tests.  Compiled into a caller's directory with the CFLAGS of oracle/Makefile and
-I oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

from ba_diffmap_shim import ORACLE, ROOT, oracle_cflags

SRC = os.path.join(ROOT, "tests", "cpp", "ssim2_map_shim.c")
MAX_SCALES = 6


class Shim:
    def __init__(self, out_dir):
        so = os.path.join(str(out_dir), "libssim2_map_shim.so")
        subprocess.check_call(["gcc", *oracle_cflags(), "-shared", "-Wl,-Bsymbolic", "-I", ORACLE, "-o", so, SRC, "-lm"])
        self.lib = L = C.CDLL(so)
        u8p, f32p, f64p, sz = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_size_t
        L.shim_ssim2_scales.argtypes, L.shim_ssim2_scales.restype = [sz, sz, C.POINTER(sz), C.POINTER(sz)], C.c_int
        L.shim_ssim2_maps.argtypes = [u8p, u8p, sz, sz, C.POINTER(C.c_int), f32p, f64p]

    def scales(self, w, h):
        """[(w_s, h_s), ...]: the oracle's scale sizes."""
        sw, sh = (C.c_size_t * MAX_SCALES)(), (C.c_size_t * MAX_SCALES)()
        n = self.lib.shim_ssim2_scales(w, h, sw, sh)
        return [(int(sw[s]), int(sh[s])) for s in range(n)]

    def maps(self, ref, test, w, h):
        """Per scale (d float32 [3, h_s, w_s], edge float64 [3, 2, h_s, w_s] = artifact, detail_lost)."""
        r, t = np.ascontiguousarray(ref, np.uint8).reshape(-1), np.ascontiguousarray(test, np.uint8).reshape(-1)
        sizes = self.scales(w, h)
        npx = sum(a * b for a, b in sizes)
        d = np.empty(3 * npx, np.float32)
        e = np.empty(6 * npx, np.float64)
        n = C.c_int()
        rc = self.lib.shim_ssim2_maps(r.ctypes.data_as(C.POINTER(C.c_uint8)), t.ctypes.data_as(C.POINTER(C.c_uint8)), w, h, C.byref(n),
                                      d.ctypes.data_as(C.POINTER(C.c_float)), e.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0 and n.value == len(sizes), (rc, n.value, sizes)
        out, off = [], 0
        for sw, sh in sizes:
            out.append((d[3 * off:3 * (off + sw * sh)].reshape(3, sh, sw).copy(), e[6 * off:6 * (off + sw * sh)].reshape(3, 2, sh, sw).copy()))
            off += sw * sh
        return out


def pool(m) -> tuple:
    """(mean, 4-norm) of one map in f64, as ssim_map / edge_diff_map pool it."""
    v = np.asarray(m, np.float64).reshape(-1)
    v2 = v * v
    return float(np.sum(v) / v.size), float(np.sqrt(np.sqrt(np.sum(v2 * v2) / v.size)))


def features(scales) -> np.ndarray:
    """[n_scales, 3, 6] pooled values of shim maps (per scale (d [3, h, w], edge [3, 2, h, w]))."""
    out = np.zeros((len(scales), 3, 6), np.float64)
    for s, (d, e) in enumerate(scales):
        for c in range(3):
            out[s, c, 0:2] = pool(d[c])
            out[s, c, 2:4] = pool(e[c, 0])
            out[s, c, 4:6] = pool(e[c, 1])
    return out


def cell_max(m: np.ndarray, B: int) -> np.ndarray:
    """[.., h, w] -> [.., ceil(h / B), ceil(w / B)] cell maxima, edge cells clipped to the map."""
    h, w = m.shape[-2:]
    bh, bw = -(-h // B), -(-w // B)
    pad = np.full(m.shape[:-2] + (bh * B, bw * B), -np.inf, np.float32)
    pad[..., :h, :w] = m
    return pad.reshape(m.shape[:-2] + (bh, B, bw, B)).max(axis=(-3, -1))
