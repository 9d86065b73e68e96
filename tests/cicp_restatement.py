"""The CICP ingest (include/ce_metrics.h: ce_batch_set_*_cicp, ce_cicp_to_linear, ce_transfer_table, ce_colour_matrix)
restated in numpy / Python floats, for the CICP tests: H.273 code points -> linear light with BT.709 / sRGB primaries.

The tables and the matrix are built per entry in Python floats (IEEE f64, the host libm's pow - the functions the library's
host code calls) in the order the header states and rounded once to float32; the per-pixel part is numpy float32, whose
products and sums are each rounded separately, as the device's are.  So the device equals this bit for bit."""
import functools
import math

import numpy as np

LINEAR_MAX = np.float32(1024.0)
PRIMARIES = (1, 9, 12)
TRANSFERS = (13, 8, 16)
DEPTHS = (8, 10, 12, 16)
# H.273 chromaticities: x, y of red, green, blue, white (D65)
CHROMATICITIES = {
    1: (0.640, 0.330, 0.300, 0.600, 0.150, 0.060, 0.3127, 0.3290),
    9: (0.708, 0.292, 0.170, 0.797, 0.131, 0.046, 0.3127, 0.3290),
    12: (0.680, 0.320, 0.265, 0.690, 0.150, 0.060, 0.3127, 0.3290),
}
# SMPTE ST 2084
PQ_M1, PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
PQ_C1, PQ_C2, PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0


def pq_nits(e: float) -> float:
    """ST 2084's EOTF in f64: the non-linear value e in [0, 1] -> cd/m^2."""
    p = math.pow(e, 1.0 / PQ_M2)
    return 10000.0 * math.pow(max(p - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * p), 1.0 / PQ_M1)


def srgb_linear(e: float) -> float:
    return e / 12.92 if e <= 0.04045 else math.pow((e + 0.055) / 1.055, 2.4)


@functools.lru_cache(maxsize=None)
def _transfer_table(transfer: int, depth: int, white_nits: float) -> np.ndarray:
    maxv = (1 << depth) - 1
    white = float(np.float32(white_nits))  # the ABI carries it as a float
    if transfer == 13:
        vals = [srgb_linear(i / maxv) for i in range(maxv + 1)]
    elif transfer == 8:
        vals = [i / maxv for i in range(maxv + 1)]
    elif transfer == 16:
        vals = [pq_nits(i / maxv) / white for i in range(maxv + 1)]
    else:
        raise ValueError(transfer)
    out = np.array(vals, np.float64).astype(np.float32)
    out.setflags(write=False)  # shared between callers
    return out


def transfer_table(transfer: int, depth: int, white_nits: float = 203.0) -> np.ndarray:
    return _transfer_table(int(transfer), int(depth), float(white_nits))


def _inv3(a):
    c00 = a[4] * a[8] - a[5] * a[7]
    c01 = a[5] * a[6] - a[3] * a[8]
    c02 = a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c00 + a[1] * c01) + a[2] * c02
    return [c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
            c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
            c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det]


def rgb_to_xyz(xy):
    """XYZ <- RGB of a set of chromaticities, row-major, in f64: RGB = (1, 1, 1) is the white point with Y = 1."""
    p = [0.0] * 9
    for c in range(3):
        x, y = xy[2 * c], xy[2 * c + 1]
        p[c], p[3 + c], p[6 + c] = x / y, 1.0, ((1.0 - x) - y) / y
    wx, wy, wz = xy[6] / xy[7], 1.0, ((1.0 - xy[6]) - xy[7]) / xy[7]
    pi = _inv3(p)
    m = [0.0] * 9
    for c in range(3):
        s = (pi[3 * c] * wx + pi[3 * c + 1] * wy) + pi[3 * c + 2] * wz
        for r in range(3):
            m[3 * r + c] = p[3 * r + c] * s
    return m


def colour_matrix_f64(primaries: int) -> np.ndarray:
    """inv(XYZ <- sRGB) * (XYZ <- src) in f64."""
    ai = _inv3(rgb_to_xyz(CHROMATICITIES[1]))
    s = rgb_to_xyz(CHROMATICITIES[primaries])
    return np.array([[(ai[3 * r] * s[c] + ai[3 * r + 1] * s[3 + c]) + ai[3 * r + 2] * s[6 + c] for c in range(3)] for r in range(3)])


def colour_matrix(primaries: int) -> np.ndarray:
    if primaries == 1:
        return np.eye(3, dtype=np.float32)
    return colour_matrix_f64(primaries).astype(np.float32)


def sanitise(a: np.ndarray) -> np.ndarray:
    """A linear image's ingest: NaN -> 0, then the clamp to +-1024; everything else bit for bit."""
    a = np.asarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(0.0), np.clip(a, -LINEAR_MAX, LINEAR_MAX)).astype(np.float32)


def to_linear(pixels: np.ndarray, primaries: int, transfer: int, depth: int, white_nits: float = 203.0) -> np.ndarray:
    """[..., 3 or 4] uint8 / uint16 code values -> [..., 3] float32 (alpha dropped)."""
    v = np.minimum(np.asarray(pixels)[..., :3].astype(np.int64), (1 << depth) - 1)
    t = transfer_table(transfer, depth, white_nits)[v]
    if primaries == 1:
        return sanitise(t)
    m = colour_matrix(primaries)
    r, g, b = t[..., 0], t[..., 1], t[..., 2]
    out = np.stack([(m[i, 0] * r + m[i, 1] * g) + m[i, 2] * b for i in range(3)], axis=-1)
    assert out.dtype == np.float32
    return sanitise(out)
