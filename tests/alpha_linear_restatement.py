"""Linear-light compositing (include/ce_metrics.h: ce_batch_set_*_cicp_over, _hlg_over, _icc_over, _linear_over, their leaves
and ce_alpha_table) restated in numpy, for the alpha-in-linear-light tests.  This is the contract: the device equals it bit
for bit.

The pixel's linear value `v` comes from the restatement of the plain call of the same kind (cicp_restatement.to_linear,
hlg_restatement, icc_restatement, icc_lut_restatement), its final clamp included.  Everything here is numpy float32, whose
products and sums are each rounded separately, as the device's are."""
import numpy as np

LINEAR_MAX = np.float32(1024.0)
MAX_BACKGROUNDS = 8
ONE, ZERO = np.float32(1.0), np.float32(0.0)


def alpha_table(depth: int) -> np.ndarray:
    """atab[k] = float32(k) / float32(m): one correctly rounded f32 division per entry."""
    m = (1 << depth) - 1
    out = np.arange(m + 1, dtype=np.float32) / np.float32(m)
    assert out.dtype == np.float32
    return out


def linear_clamp(a: np.ndarray) -> np.ndarray:
    """The clamp of a linear image: NaN -> 0, then +-1024; everything else bit for bit (-0.0 stays -0.0)."""
    a = np.asarray(a, np.float32)
    a = np.where(a > LINEAR_MAX, LINEAR_MAX, np.where(a < -LINEAR_MAX, -LINEAR_MAX, a))
    return np.where(np.isnan(a), ZERO, a).astype(np.float32)


def coverage_int(alpha: np.ndarray, depth: int) -> np.ndarray:
    """Step 2 for an integer alpha plane of `depth` bits: t = atab[min(a, m)]."""
    m = (1 << depth) - 1
    return alpha_table(depth)[np.minimum(np.asarray(alpha).astype(np.int64), m)]


def coverage_f32(alpha: np.ndarray) -> np.ndarray:
    """A float image's coverage: NaN -> 0, then clamped to [0, 1] (-0.0 stays -0.0, which is == 0)."""
    a = np.asarray(alpha, np.float32)
    a = np.where(a > ONE, ONE, np.where(a < ZERO, ZERO, a))
    return np.where(np.isnan(a), ZERO, a).astype(np.float32)


def blend(v: np.ndarray, t: np.ndarray, bg) -> np.ndarray:
    """Steps 3 and 4: v [..., 3] float32 linear values, t [...] float32 coverage, bg three floats -> [..., 3] float32."""
    v = np.asarray(v, np.float32)
    t = np.asarray(t, np.float32)[..., None]
    bg = np.broadcast_to(np.asarray(bg, np.float32), v.shape)
    u = ONE - t
    mixed = (v * t) + (bg * u)
    assert mixed.dtype == np.float32
    o = np.where(t == ONE, v, np.where(t == ZERO, bg, mixed))
    return linear_clamp(o)


def blend_premultiplied(v: np.ndarray, t: np.ndarray, bg) -> np.ndarray:
    """The premultiplied form: v already holds colour * coverage; o = (u == 0) ? v : v + (bg * u)."""
    v = np.asarray(v, np.float32)
    t = np.asarray(t, np.float32)[..., None]
    bg = np.broadcast_to(np.asarray(bg, np.float32), v.shape)
    u = ONE - t
    mixed = v + (bg * u)
    assert mixed.dtype == np.float32
    return linear_clamp(np.where(u == ZERO, v, mixed))


def over_int(v: np.ndarray, alpha: np.ndarray, depth: int, backgrounds) -> np.ndarray:
    """One integer image over K backgrounds: v [..., 3] from the plain restatement, alpha [...] code values -> [K, ..., 3]."""
    t = coverage_int(alpha, depth)
    return np.stack([blend(v, t, bg) for bg in np.asarray(backgrounds, np.float32).reshape(-1, 3)])


def over_f32(rgba: np.ndarray, premultiplied: bool, backgrounds) -> np.ndarray:
    """One CE_PIXEL_RGBA_F32 image [..., 4] over K backgrounds -> [K, ..., 3]."""
    rgba = np.asarray(rgba, np.float32)
    v, t = linear_clamp(rgba[..., :3]), coverage_f32(rgba[..., 3])
    f = blend_premultiplied if premultiplied else blend
    return np.stack([f(v, t, bg) for bg in np.asarray(backgrounds, np.float32).reshape(-1, 3)])


# ---- the matrix the host-sanitizer test and the GPU test share --------------------------------------------------------------
# 1 x 1 and 3 x 1 are tail only, 2 x 2 has no tail, 5 x 3 and 7 x 9 have an odd w * h (slots >= 1 take the unaligned store
# route), 16 x 10 and 100 x 76 are aligned throughout and more than one block
SHAPES = ((1, 1), (3, 1), (2, 2), (5, 3), (7, 9), (16, 10), (100, 76))
CICP_PIXELS = ((1, 13), (12, 13), (9, 16), (1, 8))  # (primaries, transfer)
DEPTHS = (8, 10, 12, 16)
N_BGS = (1, 2, 8)
FIRST_SLOTS = (0, 3)
# negative values and values above 1 included; all within +-LINEAR_MAX
BACKGROUNDS = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [-0.25, 0.5, 4.0], [0.18, 0.18, 0.18], [1000.0, -1000.0, 2.5],
                        [0.5, 0.0, -0.0], [1e-3, 0.999, 1.001], [12.5, 0.75, -3.0]], np.float32)
