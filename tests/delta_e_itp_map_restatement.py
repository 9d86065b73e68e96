"""The Delta E ITP maps (include/ce_metrics.h: ce_batch_delta_e_itp_map, ce_eval_pair_delta_e_itp_map)
restated in numpy on top of tests/hdr_fidelity_restatement.py: every pixel's k of pixel_q20 saturated to 32 bits, the maxima of
B x B cells with the edge cells clipped to the image, and how many pixels exceed a threshold.  A helper, not a test."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_fidelity_cases as K  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402

U32_MAX = (1 << 32) - 1
THRESHOLDS = (0, 1 << 20, 5 << 20, U32_MAX)  # above nothing, above 1 and 5 just noticeable differences, what nothing exceeds


def full_map(ref, test, depth: int, white_nits: float) -> np.ndarray:
    """[h, w, 3] float32 pair -> uint32 [h, w]: m = min(k, 2^32 - 1)."""
    ref, test = np.asarray(ref, np.float32), np.asarray(test, np.float32)
    assert ref.shape == test.shape and ref.ndim == 3 and ref.shape[2] == 3
    _, k = F.pixel_q20(ref, test, depth, white_nits)
    assert k.min() >= 0
    return np.minimum(k, U32_MAX).astype(np.uint32)


def block_max(m, block: int) -> np.ndarray:
    """uint32 [h, w] -> the maximum of every block x block cell, [ceil(h / block), ceil(w / block)]: the map padded to whole
    cells with zeros, which no maximum of unsigned values notices, and folded."""
    m = np.asarray(m)
    h, w = m.shape
    ch, cw = -(-h // block), -(-w // block)
    padded = np.zeros((ch * block, cw * block), m.dtype)
    padded[:h, :w] = m
    return padded.reshape(ch, block, cw, block).max(axis=(1, 3))


def over(m, thresholds) -> np.ndarray:
    """uint64 [n]: the pixels of the full map above each threshold."""
    m = np.asarray(m).astype(np.int64)
    return np.array([int((m > int(t)).sum()) for t in thresholds], np.uint64)


def saturating_pixels(white_nits: float):
    """The pair of imaginary colours whose k needs 33 bits: with Mi = the f64 inverse of f64(B) f64(A) and p = 1.01 * 10000 /
    white, ref = f32(Mi [p, 0, p]) and test = f32(Mi [0, p, 0]) - L and S at PQ's peak against M there - both inside +-1024."""
    a, b = F.matrices()
    mi = np.linalg.inv(b.astype(np.float64) @ a.astype(np.float64))
    p = 1.01 * 10000.0 / float(np.float32(white_nits))
    ref, test = (mi @ np.array([p, 0.0, p])).astype(np.float32), (mi @ np.array([0.0, p, 0.0])).astype(np.float32)
    assert max(np.abs(ref).max(), np.abs(test).max()) <= 1024.0
    return ref, test


@functools.lru_cache(maxsize=None)
def expected_maps(shape_index: int, depth: int, white: float):
    """The restated full maps of every pair of hdr_fidelity_cases.shape_cases()[shape_index], computed once and shared; pairs
    made of the same arrays share one map.  Read-only."""
    _, _, _, pairs = K.shape_cases()[shape_index]
    memo, out = {}, []
    for _, ref, test in pairs:
        key = (id(ref), id(test))
        if key not in memo:
            memo[key] = full_map(ref, test, depth, white)
            memo[key].setflags(write=False)
        out.append(memo[key])
    return out
