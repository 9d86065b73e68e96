"""The gain-map ingest (include/ce_metrics.h: ce_batch_set_*_gainmap, ce_gainmap_to_linear, ce_gainmap_tables,
ce_gainmap_weight) restated in numpy / Python floats, for the gain-map tests: an SDR base image read by a CICP description,
times the gain an 8-bit map and its metadata describe -> linear light with BT.709 / sRGB primaries.

The weight and the log2-gain tables are built in Python floats (IEEE f64, the host libm's pow - the function the library's
host code calls) in the order the header states; the per-pixel part is numpy int64, float64 and float32, whose products and
sums are each rounded separately, as the device's are.  gm_exp2 is the header's fixed sequence of f64 operations, not
numpy.exp2.  So the device equals this bit for bit."""
import dataclasses
import math

import numpy as np

import cicp_restatement as R
import hlg_restatement as H

LN2 = H.LN2
GAIN_LIMIT, OFFSET_LIMIT = 16.0, 1.0


@dataclasses.dataclass(frozen=True)
class Meta:
    """ce_gainmap: every field a float of the ABI (rounded to f32 on the way in); log2 gains and headrooms"""
    gain_min: tuple = (0.0, 0.0, 0.0)
    gain_max: tuple = (2.0, 2.0, 2.0)
    gamma: tuple = (1.0, 1.0, 1.0)
    base_offset: tuple = (0.0, 0.0, 0.0)
    alternate_offset: tuple = (0.0, 0.0, 0.0)
    base_headroom: float = 0.0
    alternate_headroom: float = 2.0
    display_headroom: float = 2.0

    def f32(self, name):
        v = getattr(self, name)
        return tuple(float(np.float32(x)) for x in v) if isinstance(v, tuple) else float(np.float32(v))


def gm_exp2(y) -> np.ndarray:
    """2^y as the fixed sequence of IEEE f64 operations the device runs: n = rint(y), f = (y - n) ln2, exp f as the degree-14
    Taylor series in Horner form (hlg_pow's second half, with its coefficients), times 2^n built from bits."""
    y = np.ascontiguousarray(y, np.float64)
    n = np.rint(y)
    f = (y - n) * LN2
    q = np.full_like(f, H.EXP_COEFFS[0])
    for c in H.EXP_COEFFS[1:]:
        q = q * f + c
    q = q * f + 1.0
    scale = ((n.astype(np.int64) + 1023).astype(np.uint64) << np.uint64(52)).view(np.float64)
    return q * scale


def weight(meta: Meta) -> float:
    """W = clamp((display - base) / (alternate - base), 0, 1) in f64 (ce_gainmap_weight)."""
    base, alt, disp = meta.f32("base_headroom"), meta.f32("alternate_headroom"), meta.f32("display_headroom")
    w = (disp - base) / (alt - base)
    return 0.0 if w < 0.0 else (1.0 if w > 1.0 else w)


def tables(meta: Meta, channels: int) -> np.ndarray:
    """[channels, 256] float64: Y_c[v] = W * (gain_min_c + (gain_max_c - gain_min_c) * (v / 255)^(1 / gamma_c)), no power for
    gamma_c == 1 (ce_gainmap_tables)."""
    w = weight(meta)
    lo, hi, gamma = meta.f32("gain_min"), meta.f32("gain_max"), meta.f32("gamma")
    out = np.empty((channels, 256), np.float64)
    for c in range(channels):
        span, inv_gamma = hi[c] - lo[c], 1.0 / gamma[c]
        for v in range(256):
            x = v / 255.0
            e = x if gamma[c] == 1.0 else math.pow(x, inv_gamma)
            out[c, v] = w * (lo[c] + span * e)
    return out


def axis(n: int, gn: int):
    """Step 2 along one axis: base size n, map size gn -> i0 [n], i1 [n] int64 and the fraction f [n] float64."""
    p = np.arange(n, dtype=np.int64)
    c = np.clip((2 * p + 1) * gn - n, 0, (gn - 1) * 2 * n)
    i0 = c // (2 * n)
    i1 = np.minimum(i0 + 1, gn - 1)
    f = (c - i0 * (2 * n)).astype(np.float64) / np.float64(2 * n)
    return i0, i1, f


def lerp(a, b, f):
    return a + f * (b - a)


def log2_gain(gmap: np.ndarray, meta: Meta, w: int, h: int) -> np.ndarray:
    """Steps 2 and 3: the map [gh, gw, channels] uint8 -> y [h, w, channels] float64."""
    gh, gw, channels = gmap.shape
    ytab = tables(meta, channels)
    x0, x1, fx = axis(w, gw)
    y0, y1, fy = axis(h, gh)
    fx, fy = fx[None, :], fy[:, None]
    out = np.empty((h, w, channels), np.float64)
    for c in range(channels):
        t = ytab[c][gmap[..., c]]
        top = lerp(t[y0][:, x0], t[y0][:, x1], fx)
        bottom = lerp(t[y1][:, x0], t[y1][:, x1], fx)
        out[..., c] = lerp(top, bottom, fy)
    return out


def to_linear(pixels: np.ndarray, primaries: int, transfer: int, depth: int, gmap: np.ndarray, meta: Meta, white_nits: float = 203.0) -> np.ndarray:
    """base [h, w, 3 or 4] uint8 / uint16 code values and the map [gh, gw] or [gh, gw, 1 or 3] uint8 -> [h, w, 3] float32."""
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    gmap = np.asarray(gmap, np.uint8)
    gmap = gmap[..., None] if gmap.ndim == 2 else gmap
    channels = gmap.shape[2]
    v = np.minimum(pixels[..., :3].astype(np.int64), (1 << depth) - 1)
    t = R.transfer_table(transfer, depth, white_nits)[v]
    g = gm_exp2(log2_gain(gmap, meta, w, h))
    pick = (0, 1, 2) if channels == 3 else (0, 0, 0)
    kb, ka = meta.f32("base_offset"), meta.f32("alternate_offset")
    o = np.stack([((t[..., c].astype(np.float64) + np.float64(kb[k])) * g[..., k] - np.float64(ka[k])).astype(np.float32)
                  for c, k in enumerate(pick)], axis=-1)
    if primaries == 1:
        return R.sanitise(o)
    m = R.colour_matrix(primaries)
    r, gg, b = o[..., 0], o[..., 1], o[..., 2]
    out = np.stack([(m[i, 0] * r + m[i, 1] * gg) + m[i, 2] * b for i in range(3)], axis=-1)
    assert out.dtype == np.float32
    return R.sanitise(out)


def straight(pixels: np.ndarray, primaries: int, transfer: int, depth: int, gmap: np.ndarray, meta: Meta, white_nits: float = 203.0):
    """An independent plain-f64 form of steps 1 - 5 (numpy.power, numpy.exp2, bilinear interpolation on float coordinates and
    with the other association of the weights) -> o [h, w, 3] float64 before its rounding to f32, and the product
    (t + base_offset) g whose size bounds the rounding of either form."""
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    gmap = np.asarray(gmap, np.uint8)
    gmap = gmap[..., None] if gmap.ndim == 2 else gmap
    gh, gw, channels = gmap.shape
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)  # noqa: E731
    wgt = min(max((f32(meta.display_headroom) - f32(meta.base_headroom)) / (f32(meta.alternate_headroom) - f32(meta.base_headroom)), 0.0), 1.0)
    lo, hi, gamma = f32(meta.gain_min), f32(meta.gain_max), f32(meta.gamma)
    logs = wgt * (lo[:channels] + (hi - lo)[:channels] * np.power(gmap.astype(np.float64) / 255.0, 1.0 / gamma[:channels]))
    sx = np.clip((np.arange(w) + 0.5) * gw / w - 0.5, 0.0, gw - 1.0)
    sy = np.clip((np.arange(h) + 0.5) * gh / h - 0.5, 0.0, gh - 1.0)
    x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
    x1, y1 = np.minimum(x0 + 1, gw - 1), np.minimum(y0 + 1, gh - 1)
    fx, fy = (sx - x0)[None, :, None], (sy - y0)[:, None, None]
    y = ((1 - fy) * ((1 - fx) * logs[y0][:, x0] + fx * logs[y0][:, x1]) + fy * ((1 - fx) * logs[y1][:, x0] + fx * logs[y1][:, x1]))
    g = np.exp2(y)
    g = g if channels == 3 else np.repeat(g, 3, axis=-1)
    pick = slice(0, 3) if channels == 3 else [0, 0, 0]
    v = np.minimum(pixels[..., :3].astype(np.int64), (1 << depth) - 1)
    t = R.transfer_table(transfer, depth, white_nits)[v].astype(np.float64)
    product = (t + f32(meta.base_offset)[pick]) * g
    return product - f32(meta.alternate_offset)[pick], product


# the metadata the tests walk through: gamma 1 and 2.2, W in {0, 0.37, 1}, zero and non-zero offsets, per-channel values
METAS = (
    Meta(),
    Meta(gain_min=(-1.0, -0.5, 0.25), gain_max=(3.0, 2.5, 4.0), gamma=(2.2, 1.0, 0.8), base_offset=(1 / 64, 1 / 32, 0.0),
         alternate_offset=(1 / 64, 0.0, 1 / 16), base_headroom=0.0, alternate_headroom=3.0, display_headroom=1.11),
    Meta(gain_min=(0.0, 0.0, 0.0), gain_max=(3.0, 3.0, 3.0), base_headroom=0.5, alternate_headroom=3.0, display_headroom=0.25),
    Meta(gain_min=(-2.0, -2.0, -2.0), gain_max=(2.0, 1.0, 0.0), gamma=(2.2, 2.2, 2.2), base_offset=(0.015625, 0.015625, 0.015625),
         alternate_offset=(0.015625, 0.015625, 0.015625), base_headroom=0.0, alternate_headroom=2.0, display_headroom=5.0),
)
assert [round(weight(m), 2) for m in METAS] == [1.0, 0.37, 0.0, 1.0]
