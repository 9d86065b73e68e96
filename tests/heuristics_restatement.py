"""A numpy restatement of compute_heuristics (crates/codec-compare/src/image_heuristics.rs:76-305), written from the
reference's arithmetic: every value is np.float32, one operation at a time, in the reference's order.

Two accumulation modes for the whole-image sums (the Tier B fields of ce_metrics.h):
  "f64"      the device's contract: the f32 terms added in f64, rounded once to f32
  "seq_f32"  the reference's own order: one f32 accumulator, element after element (np.add.accumulate; np.sum would add
             pairwise)
Per-pixel and per-block values, counts, thresholds and the maximum do not depend on the mode.
"""
from __future__ import annotations

import numpy as np

F = np.float32
MODES = ("f64", "seq_f32")

# the f32 fields whose value rests on a whole-image sum (they differ between the modes)
TIER_B = ("mean_luminance", "luminance_variance", "luminance_std", "edge_strength_mean", "block_variance_mean",
          "block_variance_std", "color_variance", "saturation_mean", "saturation_std", "local_contrast_mean",
          "local_contrast_std", "horizontal_complexity", "vertical_complexity", "diagonal_complexity")
TIER_A = ("edge_strength_max", "edge_density", "flat_block_pct", "low_var_block_pct", "mid_var_block_pct",
          "high_var_block_pct", "detail_block_pct", "analyze_detail_block_pct", "high_freq_energy", "low_freq_energy",
          "freq_ratio")


def _sum(terms, mode: str) -> np.float32:
    t = np.ascontiguousarray(terms, dtype=np.float32).ravel()
    if t.size == 0:
        return F(0.0)
    if mode == "seq_f32":
        return np.add.accumulate(t, dtype=np.float32)[-1]
    if mode == "f64":
        return F(t.astype(np.float64).sum())
    raise ValueError(mode)


def gray_of(rgb: np.ndarray) -> np.ndarray:
    """image_heuristics.rs:84-88: (0.299 r + 0.587 g) + 0.114 b in f32; rgb is [h, w, 3] uint8."""
    r, g, b = (rgb[..., c].astype(np.float32) for c in range(3))
    return (F(0.299) * r + F(0.587) * g) + F(0.114) * b


def block_variances(gray: np.ndarray) -> np.ndarray:
    """Each whole 8x8 block's variance (image_heuristics.rs:111-131), blocks in row-major order: the 64 terms of a block
    added sequentially in f32 in row-major order, then / 64."""
    h, w = gray.shape
    by, bx = h // 8, w // 8
    if by == 0 or bx == 0:
        return np.zeros(0, np.float32)
    blk = gray[: by * 8, : bx * 8].reshape(by, 8, bx, 8).transpose(0, 2, 1, 3).reshape(by * bx, 64)
    s = np.zeros(by * bx, np.float32)
    for k in range(64):
        s = s + blk[:, k]
    mean = s / F(64.0)
    q = np.zeros(by * bx, np.float32)
    for k in range(64):
        d = blk[:, k] - mean
        q = q + d * d
    return q / F(64.0)


def edge_strengths(gray: np.ndarray) -> np.ndarray:
    gx = gray[1:-1, 2:] - gray[1:-1, :-2]
    gy = gray[2:, 1:-1] - gray[:-2, 1:-1]
    return np.sqrt(gx * gx + gy * gy)


def local_contrasts(gray: np.ndarray) -> np.ndarray:
    h, w = gray.shape
    hi = lo = gray[1:-1, 1:-1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v = gray[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
            hi, lo = np.maximum(hi, v), np.minimum(lo, v)
    return hi - lo


def adjacent_diffs(gray: np.ndarray) -> np.ndarray:
    return np.abs(gray[:, 1:] - gray[:, :-1])


def compute(rgb, width: int, height: int, mode: str = "f64") -> dict:
    """compute_heuristics of a packed RGB8 image (at least 3 x 3) -> {field: value}; f32 fields as np.float32."""
    if width < 3 or height < 3:
        raise ValueError("the reference needs at least 3 x 3 pixels")
    a = np.asarray(rgb, np.uint8).reshape(height, width, 3)
    pixels = width * height
    fpix = F(pixels)
    gray = gray_of(a)
    o = {"width": width, "height": height, "pixels": pixels}

    o["mean_luminance"] = _sum(gray, mode) / fpix
    d = gray - o["mean_luminance"]
    o["luminance_variance"] = _sum(d * d, mode) / fpix
    o["luminance_std"] = np.sqrt(o["luminance_variance"])

    es = edge_strengths(gray)
    n_es = F(max(es.size, 1))
    o["edge_strength_mean"] = _sum(es, mode) / n_es
    o["edge_strength_max"] = F(es.max()) if es.size else F(0.0)
    o["edge_density"] = F(int(np.count_nonzero(es > F(30.0)))) / n_es

    bv = block_variances(gray)
    nb = F(max(bv.size, 1))
    pct = lambda m: F(100.0) * F(int(np.count_nonzero(m))) / nb  # noqa: E731
    o["flat_block_pct"] = pct(bv < F(100.0))
    o["low_var_block_pct"] = pct(bv < F(500.0))
    o["mid_var_block_pct"] = pct((bv >= F(500.0)) & (bv < F(2000.0)))
    o["high_var_block_pct"] = pct((bv >= F(2000.0)) & (bv < F(5000.0)))
    o["detail_block_pct"] = pct(bv >= F(5000.0))
    o["block_variance_mean"] = _sum(bv, mode) / nb
    d = bv - o["block_variance_mean"]
    o["block_variance_std"] = np.sqrt(_sum(d * d, mode) / nb)

    var = []
    for c in range(3):
        ch = a[..., c].astype(np.float32)
        m = _sum(ch, mode) / fpix
        d = ch - m
        var.append(_sum(d * d, mode) / fpix)
    o["color_variance"] = (var[0] + var[1] + var[2]) / F(3.0)

    mx = a.max(axis=2).astype(np.float32)
    mn = a.min(axis=2).astype(np.float32)
    sat = np.zeros_like(mx)
    np.divide(mx - mn, mx, out=sat, where=mx > F(0.0))
    o["saturation_mean"] = _sum(sat, mode) / fpix
    d = sat - o["saturation_mean"]
    o["saturation_std"] = np.sqrt(_sum(d * d, mode) / fpix)

    diff = adjacent_diffs(gray)
    # the reference counts in f32 (`+= 1.0`), which stops at 2^24
    low = F(min(int(np.count_nonzero(diff < F(10.0))), 1 << 24))
    high = F(min(int(np.count_nonzero(diff > F(30.0))), 1 << 24))
    transitions = F((width - 1) * height)
    o["low_freq_energy"] = low / transitions
    o["high_freq_energy"] = high / transitions
    o["freq_ratio"] = o["high_freq_energy"] / o["low_freq_energy"] if o["low_freq_energy"] > F(0.0) else o["high_freq_energy"]

    lc = local_contrasts(gray)
    n_lc = F(max(lc.size, 1))
    o["local_contrast_mean"] = _sum(lc, mode) / n_lc
    d = lc - o["local_contrast_mean"]
    o["local_contrast_std"] = np.sqrt(_sum(d * d, mode) / n_lc)

    n = F((width - 2) * (height - 2))
    o["horizontal_complexity"] = _sum(np.abs(gray[1:-1, 2:] - gray[1:-1, :-2]), mode) / n
    o["vertical_complexity"] = _sum(np.abs(gray[2:, 1:-1] - gray[:-2, 1:-1]), mode) / n
    o["diagonal_complexity"] = _sum(np.abs(gray[2:, 2:] - gray[:-2, :-2]), mode) / n

    # analyze-image (analyze_image.rs:94-96), over num_blocks.max(1) as above
    o["analyze_detail_block_pct"] = pct(bv > F(1000.0))
    return o


def ulp_distance(a, b) -> int:
    """Distance in f32 units in the last place between two finite f32 values of the same sign."""
    ia = int(np.asarray(a, np.float32).view(np.int32))
    ib = int(np.asarray(b, np.float32).view(np.int32))
    return abs(ia - ib)
