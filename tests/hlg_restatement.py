"""The HLG ingest (include/ce_metrics.h: ce_batch_set_*_hlg, ce_hlg_to_linear, ce_hlg_table, ce_hlg_params) restated in
numpy / Python floats, for the HLG tests: BT.2100 HLG code values -> display light through the inverse OETF and the OOTF ->
linear light with BT.709 / sRGB primaries, 1.0 = white_nits.

The table and the five parameters are built in Python floats (IEEE f64, the host libm's exp and log10 - the functions the
library's host code calls) in the order the header states; the per-pixel part is numpy float64 and float32, whose products
and sums are each rounded separately, as the device's are.  hlg_pow is the header's fixed sequence of f64 operations, not
numpy.power.  So the device equals this bit for bit."""
import functools
import math

import numpy as np

import cicp_restatement as R

PRIMARIES = R.PRIMARIES
DEPTHS = R.DEPTHS
# BT.2100's published constants of the HLG OETF
HLG_A, HLG_B, HLG_C = 0.17883277, 0.28466892, 0.55991073
GAMMA_MIN, GAMMA_MAX = 0.8, 1.6

LN2 = 0.6931471805599453
SQRT2 = 1.4142135623730951
LOG_COEFFS = tuple(1.0 / k for k in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0))
EXP_COEFFS = tuple(1.0 / f for f in (87178291200.0, 6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0,
                                     720.0, 120.0, 24.0, 6.0, 2.0, 1.0))


def hlg_pow(x, g) -> np.ndarray:
    """x^g for normal f64 x > 0, as the fixed sequence of IEEE f64 operations the device runs: x = m 2^e with m in
    [sqrt(1/2), sqrt(2)); ln m = 2 t P(t^2), t = (m - 1) / (m + 1), P the odd-reciprocal series to 1/21 in Horner form;
    y = g (ln m + e ln2); n = rint(y / ln2), f = y - n ln2; exp f as the degree-14 Taylor series in Horner form; times 2^n
    built from bits."""
    x = np.ascontiguousarray(x, np.float64)
    g = np.float64(g)
    bits = x.view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)).view(np.float64)
    big = m >= SQRT2
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    p = np.full_like(t, LOG_COEFFS[0])
    for c in LOG_COEFFS[1:]:
        p = p * t2 + c
    p = p * t2 + 1.0
    ln_m = (2.0 * t) * p
    y = g * (ln_m + e.astype(np.float64) * LN2)
    n = np.rint(y / LN2)
    f = y - n * LN2
    q = np.full_like(f, EXP_COEFFS[0])
    for c in EXP_COEFFS[1:]:
        q = q * f + c
    q = q * f + 1.0
    scale = ((n.astype(np.int64) + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
    return q * scale


def inverse_oetf(x: float) -> float:
    """BT.2100's HLG inverse OETF in f64: the non-linear signal x in [0, 1] -> scene light in [0, 1]."""
    return x * x / 3.0 if x <= 0.5 else (math.exp((x - HLG_C) / HLG_A) + HLG_B) / 12.0


@functools.lru_cache(maxsize=None)
def _table(depth: int) -> np.ndarray:
    maxv = (1 << depth) - 1
    out = np.array([inverse_oetf(i / maxv) for i in range(maxv + 1)], np.float64).astype(np.float32)
    out.setflags(write=False)  # shared between callers
    return out


def hlg_table(depth: int) -> np.ndarray:
    return _table(int(depth))


def system_gamma(peak_nits: float, given: float = 0.0) -> float:
    """gamma as given (a float of the ABI) if non-zero, else BT.2100's rule 1.2 + 0.42 log10(L_W / 1000) in f64."""
    given = float(np.float32(given))
    if given != 0.0:
        return given
    return 1.2 + 0.42 * math.log10(float(np.float32(peak_nits)) / 1000.0)


def luminance_coefficients(primaries: int):
    """The Y row of the f64 XYZ <- src matrix of the tagged primaries."""
    return tuple(R.rgb_to_xyz(R.CHROMATICITIES[primaries])[3:6])


def hlg_params(primaries: int, peak_nits: float, gamma: float = 0.0, white_nits: float = 203.0):
    """kR, kG, kB, gamma - 1, A = peak / white: the five doubles the kernel is handed (ce_hlg_params)."""
    g = system_gamma(peak_nits, gamma)
    if not (GAMMA_MIN <= g <= GAMMA_MAX):
        raise ValueError(f"system gamma {g} outside [{GAMMA_MIN}, {GAMMA_MAX}]")
    kr, kg, kb = luminance_coefficients(primaries)
    return kr, kg, kb, g - 1.0, float(np.float32(peak_nits)) / float(np.float32(white_nits))


def ootf_scale(e: np.ndarray, params) -> np.ndarray:
    """Steps 2 and 3: e [..., 3] float32 scene light -> k [...] float32, the factor from scene to display light."""
    kr, kg, kb, gm1, a = (np.float64(v) for v in params)
    er, eg, eb = (e[..., c].astype(np.float64) for c in range(3))
    ys = (kr * er + kg * eg) + kb * eb
    s = np.where(ys > 0.0, hlg_pow(np.where(ys > 0.0, ys, 1.0), gm1), 0.0)
    return (a * s).astype(np.float32)


def to_linear(pixels: np.ndarray, primaries: int, depth: int, peak_nits: float = 1000.0, gamma: float = 0.0,
              white_nits: float = 203.0) -> np.ndarray:
    """[..., 3 or 4] uint8 / uint16 HLG code values -> [..., 3] float32 (alpha dropped)."""
    v = np.minimum(np.asarray(pixels)[..., :3].astype(np.int64), (1 << depth) - 1)
    e = hlg_table(depth)[v]
    k = ootf_scale(e, hlg_params(primaries, peak_nits, gamma, white_nits))
    d = k[..., None] * e
    assert d.dtype == np.float32
    if primaries == 1:
        return R.sanitise(d)
    m = R.colour_matrix(primaries)
    r, g, b = d[..., 0], d[..., 1], d[..., 2]
    out = np.stack([(m[i, 0] * r + m[i, 1] * g) + m[i, 2] * b for i in range(3)], axis=-1)
    assert out.dtype == np.float32
    return R.sanitise(out)


def grey_nits(signal: float, peak_nits: float = 1000.0, gamma: float = 0.0) -> float:
    """Display luminance in cd/m^2 of the grey HLG signal `signal` in [0, 1], all in f64 (the published pins)."""
    e = inverse_oetf(signal)
    if e <= 0.0:
        return 0.0
    g = system_gamma(peak_nits, gamma)
    return peak_nits * float(hlg_pow(np.array([e]), g - 1.0)[0]) * e


# (peak_nits, system_gamma, white_nits) the tests walk through: gamma derived at three peaks, and gamma given as 1.0 with
# peak == white, the identity of the OOTF
DISPLAYS = ((1000.0, 0.0, 203.0), (400.0, 0.0, 203.0), (4000.0, 0.0, 203.0), (600.0, 1.0, 600.0))


def yuv_to_linear(y, cb, cr, w, h, sub, matrix, range_, mode, d, msb, primaries, depth, peak_nits=1000.0, gamma=0.0, white_nits=203.0):
    """The Y'CbCr route's definition: integer RGB of `depth` bits by tests/yuv_restatement.py, then to_linear above."""
    import yuv_restatement as Y
    rgb = Y.yuv_to_rgb(y, cb, cr, w, h, sub, matrix, range_, mode, d, depth, msb)
    return to_linear(rgb, primaries, depth, peak_nits, gamma, white_nits)
