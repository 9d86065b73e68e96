"""The SSIM / MS-SSIM maps as include/ce_metrics.h defines them (ce_batch_msssim_map), restated in numpy on
top of tests/msssim_restatement.py: its filter, its pooling and its quantisation, float64 element-wise operations in the
header's order, then integers.  The device equals this on every element."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msssim_restatement import Q, filt, levels_of, pool  # noqa: E402

U32_MAX = (1 << 32) - 1
Q32 = 1 << 32
WHAT = {"ssim": 0, "cs": 1}


def position_q(x, y, L):
    """one level of one channel (float64 planes) -> qs, qc: int64 [h - 10, w - 10], the integers level_sums adds up"""
    c1, c2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    cs = (2.0 * sxy + c2) / ((sxx + syy) + c2)
    lum = (2.0 * (mx * my) + c1) / ((mx * mx + my * my) + c1)
    s = lum * cs
    return np.rint(s * Q).astype(np.int64), np.rint(cs * Q).astype(np.int64)


def level_q(ref, test, depth, levels, level):
    """ref, test: (h, w, 3) integer samples of `depth` bits -> int64 [2 (qs, qc), 3, vh, vw] at `level` of `levels`"""
    h, w, _ = ref.shape
    assert levels_of(w, h, levels) is not None and 0 <= level < levels
    L = float((1 << depth) - 1)
    out = []
    for c in range(3):
        x, y = ref[:, :, c].astype(np.float64), test[:, :, c].astype(np.float64)
        for _ in range(level):
            x, y = pool(x), pool(y)
        out.append(position_q(x, y, L))
    return np.stack([np.stack([o[k] for o in out]) for k in range(2)])


def value(q):
    """the map value of q: 2^32 - q saturated to [0, 2^32 - 1], uint32"""
    return np.clip(Q32 - q.astype(np.int64), 0, U32_MAX).astype(np.uint32)


def full_map(ref, test, depth, levels=5, level=0, what="ssim"):
    """-> uint32 [3, vh, vw]: the block-1 map of one pair"""
    return value(level_q(ref, test, depth, levels, level)[WHAT[what]])


def cells(m, block):
    """the maximum of m [..., vh, vw] over block x block cells, edge cells clipped: [..., ceil(vh / block), ceil(vw / block)]"""
    if block == 1:
        return m.copy()
    vh, vw = m.shape[-2:]
    ch, cw = -(-vh // block), -(-vw // block)
    p = np.zeros(m.shape[:-2] + (ch * block, cw * block), m.dtype)  # 0 is the least value: padding cannot raise a maximum
    p[..., :vh, :vw] = m
    return p.reshape(m.shape[:-2] + (ch, block, cw, block)).max(axis=(-3, -1))


def over(m, thresholds):
    """m: the block-1 map [3, vh, vw] -> uint64 [3, n]: positions with d > thresholds[j], per channel"""
    return np.array([[int((m[c] > np.uint32(t)).sum()) for t in thresholds] for c in range(m.shape[0])], np.uint64)
