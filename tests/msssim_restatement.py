"""SSIM / MS-SSIM as include/ce_metrics.h defines them (ce_batch_msssim), restated in numpy: float64
element-wise operations in the header's order - numpy neither fuses nor reorders them - and Python integers for the sums.  The
device equals this on every integer."""
import math

import numpy as np

G6 = [0.00102838008447911, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002, 0.2130055377112537, 0.26601172486179436]
G = np.array(G6 + G6[4::-1], np.float64)
WT = [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]
Q = 4294967296.0


def levels_of(w, h, levels):
    """-> [(w_l, h_l)]; None where the header refuses"""
    if levels not in (1, 5) or (min(w, h) < 11 if levels == 1 else min(w, h) <= 160):
        return None
    out = []
    for _ in range(levels):
        out.append((w, h))
        w, h = (w + (w & 1)) // 2, (h + (h & 1)) // 2
    return out


def filt(p):
    h, w = p.shape
    v = np.zeros((h - 10, w), np.float64)
    for i in range(11):
        v = v + G[i] * p[i:i + h - 10, :]
    o = np.zeros((h - 10, w - 10), np.float64)
    for i in range(11):
        o = o + G[i] * v[:, i:i + w - 10]
    return o


def pool(p):
    h, w = p.shape
    q = np.zeros((h + (h & 1), w + (w & 1)), np.float64)
    q[h & 1:, w & 1:] = p
    return ((q[0::2, 0::2] + q[0::2, 1::2]) + (q[1::2, 0::2] + q[1::2, 1::2])) * 0.25


def level_sums(x, y, L):
    """one level of one channel (float64 planes) -> ssim_q, cs_q, n"""
    c1, c2 = (0.01 * L) * (0.01 * L), (0.03 * L) * (0.03 * L)
    mx, my = filt(x), filt(y)
    sxx, syy, sxy = filt(x * x) - mx * mx, filt(y * y) - my * my, filt(x * y) - mx * my
    cs = (2.0 * sxy + c2) / ((sxx + syy) + c2)
    lum = (2.0 * (mx * my) + c1) / ((mx * mx + my * my) + c1)
    s = lum * cs
    qs, qc = np.rint(s * Q).astype(np.int64), np.rint(cs * Q).astype(np.int64)
    return sum(int(v) for v in qs.sum(axis=1)), sum(int(v) for v in qc.sum(axis=1)), qs.size


def msssim(ref, test, depth, levels=5):
    """ref, test: (h, w, 3) integer samples of `depth` bits -> ce_msssim_scores as a dict"""
    h, w, _ = ref.shape
    assert levels_of(w, h, levels) is not None
    L = float((1 << depth) - 1)
    ssim_q, cs_q = [[0] * 3 for _ in range(5)], [[0] * 3 for _ in range(5)]
    n = [0] * 5
    for c in range(3):
        x, y = ref[:, :, c].astype(np.float64), test[:, :, c].astype(np.float64)
        for l in range(levels):
            ssim_q[l][c], cs_q[l][c], n[l] = level_sums(x, y, L)
            x, y = pool(x), pool(y)
    out = {"ssim_q": ssim_q, "cs_q": cs_q, "n": n, "n_levels": levels}
    ms = [[(float(ssim_q[l][c]) / Q) / n[l] for c in range(3)] for l in range(levels)]
    mc = [[(float(cs_q[l][c]) / Q) / n[l] for c in range(3)] for l in range(levels)]
    out["ssim_rgb"] = ms[0]
    out["ms_ssim_rgb"] = [math.nan] * 3
    if levels == 5:
        for c in range(3):
            p = math.pow(max(mc[0][c], 0.0), WT[0])
            for l in range(1, 4):
                p = p * math.pow(max(mc[l][c], 0.0), WT[l])
            out["ms_ssim_rgb"][c] = p * math.pow(max(ms[4][c], 0.0), WT[4])
    out["ssim"] = ((out["ssim_rgb"][0] + out["ssim_rgb"][1]) + out["ssim_rgb"][2]) / 3.0
    out["ms_ssim"] = ((out["ms_ssim_rgb"][0] + out["ms_ssim_rgb"][1]) + out["ms_ssim_rgb"][2]) / 3.0
    return out
