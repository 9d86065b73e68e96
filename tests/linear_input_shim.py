"""Builds and loads tests/cpp/linear_input_shim.c: the CPU oracle's metrics on linear input (packed float32 RGB, linear
light with sRGB primaries, any range), for the linear-input and wide-content tests - scores, every per-pixel map, and the
operand ranges of the oracle's hand-expandable divisions.  Compiled into a caller's directory with the CFLAGS of
oracle/Makefile and -I oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

from ba_diffmap_shim import ORACLE, ROOT, oracle_cflags

SRC = os.path.join(ROOT, "tests", "cpp", "linear_input_shim.c")
BA_MALTA_F32, BA_L2_EARLY = 5, 8  # ce_oracle.h: CEO_V_BA_MALTA_F32, CEO_V_BA_L2_EARLY
MAX_LEVELS, MAX_SCALES = 5, 6
DIV_SITES = ("cbrt_poly step 1", "cbrt_poly step 2", "fast_log2f yp/yq", "gamma(p)/p", "malta norm2_0gt1/(norm1+|v|)",
             "malta norm2_0lt1/(norm1+|v|)")  # ce_oracle.h: enum ceo_div_site
PROBE_FIELDS = ("num_min", "num_max", "den_min", "den_max", "quot_min", "quot_max", "signs", "num_zero", "den_zero", "num_subnormal",
                "den_subnormal", "quot_subnormal", "quot_nonfinite", "count")


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
        L.shim_linear_butteraugli_map.argtypes = [f32p, f32p, sz, sz, C.c_float, f64p, f64p, f32p]
        L.shim_linear_dssim_maps.argtypes = [f32p, f32p, sz, sz, C.POINTER(C.c_int), f32p, f64p, f64p]
        L.shim_linear_ssim2_maps.argtypes = [f32p, f32p, sz, sz, C.POINTER(C.c_int), f32p, f64p, f32p]
        L.shim_set_variant.argtypes, L.shim_set_variant.restype = [C.c_int, C.c_int], None
        L.shim_probe_reset.argtypes, L.shim_probe_reset.restype = [], None
        L.shim_probe_read.argtypes, L.shim_probe_read.restype = [f64p], None
        L.shim_probe_cbrt_den.argtypes, L.shim_probe_cbrt_den.restype = [C.c_float, C.c_int], C.c_float

    def set_variant(self, key: int, value: int):
        self.lib.shim_set_variant(key, value)

    def set_device_switches(self, on: bool):
        """The two switches with which the oracle is the device's arithmetic (tests/test_gpu_butteraugli.py)."""
        for k in (BA_MALTA_F32, BA_L2_EARLY):
            self.lib.shim_set_variant(k, int(on))

    def probe_reset(self):
        self.lib.shim_probe_reset()

    def probe(self) -> dict:
        """{site: {field: value}} over every division since the last probe_reset (tests/cpp/linear_input_shim.c)."""
        out = np.zeros((len(DIV_SITES), len(PROBE_FIELDS)), np.float64)
        self.lib.shim_probe_read(out.ctypes.data_as(C.POINTER(C.c_double)))
        return {site: dict(zip(PROBE_FIELDS, (float(v) for v in row))) for site, row in zip(DIV_SITES, out)}

    def cbrt_den(self, x, step=1) -> float:
        """The denominator of cbrt_poly's Halley step `step` (1 or 2) at float32 x."""
        return float(self.lib.shim_probe_cbrt_den(float(np.float32(x)), step))

    def butteraugli_map(self, ref, test, w, h, intensity_target=80.0):
        """-> (score, 3-norm, diffmap float32 [h, w])"""
        r, t, s, p = _f32(ref), _f32(test), C.c_double(), C.c_double()
        out = np.empty((h, w), np.float32)
        rc = self.lib.shim_linear_butteraugli_map(_p(r), _p(t), w, h, intensity_target, C.byref(s), C.byref(p), _p(out))
        assert rc == 0, rc
        return s.value, p.value, out

    def dssim_maps(self, ref, test, w, h):
        """-> (dssim, [(map float32 [h_l, w_l], score), ...]): every scale of Dssim::compare"""
        r, t = _f32(ref), _f32(test)
        sizes = dssim_levels(w, h)
        buf = np.empty(sum(a * b for a, b in sizes), np.float32)
        scores = np.zeros(MAX_LEVELS, np.float64)
        n, out = C.c_int(), C.c_double()
        rc = self.lib.shim_linear_dssim_maps(_p(r), _p(t), w, h, C.byref(n), _p(buf), scores.ctypes.data_as(C.POINTER(C.c_double)), C.byref(out))
        assert rc == 0 and n.value == len(sizes), (rc, n.value, sizes)
        res, off = [], 0
        for l, (lw, lh) in enumerate(sizes):
            res.append((buf[off:off + lw * lh].reshape(lh, lw).copy(), float(scores[l])))
            off += lw * lh
        return out.value, res

    def ssim2_maps(self, ref, test, w, h):
        """Per scale (d float32 [3, h_s, w_s], edge float64 [3, 2, h_s, w_s] = artifact, detail_lost, the same two in f32)."""
        r, t = _f32(ref), _f32(test)
        sizes = ssim2_scales(w, h)
        npx = sum(a * b for a, b in sizes)
        d, e, f = np.empty(3 * npx, np.float32), np.empty(6 * npx, np.float64), np.empty(6 * npx, np.float32)
        n = C.c_int()
        rc = self.lib.shim_linear_ssim2_maps(_p(r), _p(t), w, h, C.byref(n), _p(d), e.ctypes.data_as(C.POINTER(C.c_double)), _p(f))
        assert rc == 0 and n.value == len(sizes), (rc, n.value, sizes)
        out, off = [], 0
        for sw, sh in sizes:
            out.append((d[3 * off:3 * (off + sw * sh)].reshape(3, sh, sw).copy(), e[6 * off:6 * (off + sw * sh)].reshape(3, 2, sh, sw).copy(),
                        f[6 * off:6 * (off + sw * sh)].reshape(3, 2, sh, sw).copy()))
            off += sw * sh
        return out

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


def dssim_levels(w, h):
    """create_image's scale sizes (oracle/dssim.c; tests/cpp/dssim_map_shim.c: shim_dssim_levels)."""
    out = []
    for scale in range(MAX_LEVELS):
        out.append((w, h))
        if scale + 1 >= MAX_LEVELS or w < 8 or h < 8:
            break
        w, h = w // 2, h // 2
    return out


def ssim2_scales(w, h):
    """ceo_ssimulacra2_detail's scale sizes (tests/cpp/ssim2_map_shim.c: shim_ssim2_scales)."""
    out = []
    for scale in range(MAX_SCALES):
        if w < 8 or h < 8:
            break
        if scale > 0:
            w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out
