"""The plane-domain scores as include/ce_metrics.h defines them (ce_yuv_plane_fidelity), restated in numpy.
The filter, the pooling, a level's sums, the weights and the quantum are tests/msssim_restatement.py's, imported, not copied;
here are the plane geometry, the sample rule, the squared error as Python integers, the level rule of a chroma plane and the
finishing.  The device equals this on every integer."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from msssim_restatement import Q, WT, filt, level_sums, levels_of, pool  # noqa: E402,F401

SUB_444, SUB_422, SUB_420, SUB_400 = 0, 1, 2, 3


def plane_sizes(w, h, sub):
    """-> [(w_p, h_p)] of the planes the subsampling has"""
    if sub == SUB_400:
        return [(w, h)]
    cw = w if sub == SUB_444 else (w + 1) // 2
    ch = (h + 1) // 2 if sub == SUB_420 else h
    return [(w, h), (cw, ch), (cw, ch)]


def sample(stored, depth, msb_aligned=False):
    """stored values -> the samples scored: min(v >> shift, 2^d - 1)"""
    v = np.asarray(stored).astype(np.int64) >> ((16 - depth) if msb_aligned else 0)
    return np.minimum(v, (1 << depth) - 1)


def n_levels_of(w, h, sub, levels):
    """-> the levels every plane runs, or None where the call is refused"""
    if levels not in (0, 1, 5) or w == 0 or h == 0 or (levels and levels_of(w, h, levels) is None):
        return None
    out = []
    for p, (pw, ph) in enumerate(plane_sizes(w, h, sub)):
        if p == 0 or (levels and levels_of(pw, ph, levels) is not None):
            out.append(levels)
        else:
            out.append(1 if levels >= 1 and min(pw, ph) >= 11 else 0)
    return out + [0] * (3 - len(out))


def psnr(sse, n, L):
    mse = float(sse) / float(n)
    return math.inf if mse == 0.0 else 10.0 * math.log10(L * L / mse)


def plane_fidelity(ref, test, depth, sub, levels=5):
    """ref, test: the planes' SAMPLES (sample() already applied), [(h_p, w_p) integer arrays] -> ce_plane_scores as a dict"""
    h, w = ref[0].shape
    n_levels = n_levels_of(w, h, sub, levels)
    assert n_levels is not None and [p.shape[::-1] for p in ref] == plane_sizes(w, h, sub) == [p.shape[::-1] for p in test]
    L = float((1 << depth) - 1)
    n_planes = len(ref)
    out = {"n_planes": n_planes, "n_levels": n_levels, "sse": [0] * 3, "n": [0] * 3, "psnr": [math.nan] * 3, "ssim": [math.nan] * 3,
           "ms_ssim": [math.nan] * 3, "ssim_q": [[0] * 5 for _ in range(3)], "cs_q": [[0] * 5 for _ in range(3)],
           "n_pos": [[0] * 5 for _ in range(3)]}
    for p in range(n_planes):
        d = ref[p].astype(np.int64) - test[p].astype(np.int64)
        out["sse"][p] = sum(int(v) for v in (d * d).sum(axis=1))
        out["n"][p] = d.size
        out["psnr"][p] = psnr(out["sse"][p], out["n"][p], L)
        x, y = ref[p].astype(np.float64), test[p].astype(np.float64)
        ms, mc = [], []
        for l in range(n_levels[p]):
            out["ssim_q"][p][l], out["cs_q"][p][l], out["n_pos"][p][l] = level_sums(x, y, L)
            ms.append((float(out["ssim_q"][p][l]) / Q) / out["n_pos"][p][l])
            mc.append((float(out["cs_q"][p][l]) / Q) / out["n_pos"][p][l])
            x, y = pool(x), pool(y)
        if n_levels[p] >= 1:
            out["ssim"][p] = ms[0]
        if n_levels[p] == 5:
            v = math.pow(max(mc[0], 0.0), WT[0])
            for l in range(1, 4):
                v = v * math.pow(max(mc[l], 0.0), WT[l])
            out["ms_ssim"][p] = v * math.pow(max(ms[4], 0.0), WT[4])
    out["psnr_weighted"] = ((6.0 * out["psnr"][0] + out["psnr"][1]) + out["psnr"][2]) / 8.0
    out["psnr_overall"] = psnr(sum(out["sse"]), sum(out["n"]), L)
    return out
