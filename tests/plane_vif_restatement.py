"""Pixel-domain VIF (VIFp, Sheikh & Bovik's vifp_mscale) of a decoder's planes as include/ce_metrics.h defines it
(ce_yuv_plane_vif), restated in numpy operation by operation: the four windows, the "valid" filter first
down the columns and then along the rows with explicit tap loops in the stated order, the filter-and-decimate pyramid in f64,
the per-position text with its four exceptional branches, the fixed-sequence logarithm on the bit patterns, the quantisation to
2^-24 nat and the finishing.  Every f64 operation below is one numpy operation, so it is rounded where the header rounds it;
the sums are Python integers.  Neither np.convolve nor np.log is used.  The planes, their sizes and the sample rule are
tests/plane_fidelity_restatement.py's, imported, not copied.  The device equals this on every integer."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plane_fidelity_restatement import SUB_400, SUB_420, SUB_422, SUB_444, plane_sizes, sample  # noqa: E402,F401

TAPS = (17, 9, 5, 3)  # scale 1 .. 4
MIN_SIDE = 41         # the smallest side that leaves scale 4 a position
EPS = 1e-10
BRANCHES = ("s1_small", "s2_small", "g_negative", "sv_small")


def window(n):
    """g[i] = exp(-(i - c)^2 / (2 sd^2)) over their sum, c = (n - 1) / 2, sd = n / 5: the numbers the library holds as literals"""
    i = np.arange(n, dtype=np.float64)
    c, sd = (n - 1) / 2, n / 5
    g = np.exp(-(i - c) ** 2 / (2 * sd ** 2))
    return g / g.sum()


def filt(p, g):
    """'valid' filtering of p [h, w] f64 with the taps g: down the columns, then along the rows; each pass ((g0 p0 + g1 p1) +
    g2 p2) + ..., products separately rounded, sums left to right"""
    n, (h, w) = len(g), p.shape
    oh, ow = h - n + 1, w - n + 1
    v = g[0] * p[0:oh] + g[1] * p[1:oh + 1]
    for i in range(2, n):
        v = v + g[i] * p[i:oh + i]
    o = g[0] * v[:, 0:ow] + g[1] * v[:, 1:ow + 1]
    for i in range(2, n):
        o = o + g[i] * v[:, i:ow + i]
    return o


def scale_sizes(pw, ph):
    """-> [(w_s, h_s)] of the four scales of a pw x ph plane, or [] if it does not run"""
    if pw < MIN_SIDE or ph < MIN_SIDE:
        return []
    out = [(pw, ph)]
    for n in TAPS[1:]:
        w, h = out[-1]
        out.append(((w - n + 2) // 2, (h - n + 2) // 2))
    return out


def ln_fixed(x):
    """ln x for normal x >= 1, on the bit patterns: the first half of hlg_pixel.h's hlg_pow, operation for operation"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)).view(np.float64)
    big = m >= 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    p = np.full(x.shape, 1.0 / 21.0)
    for k in (19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
        p = p * t2 + 1.0 / k
    p = p * t2 + 1.0
    return (2.0 * t) * p + e.astype(np.float64) * 0.6931471805599453


def position_terms(X, Y, n):
    """X, Y: the two sides at one scale, f64 [h, w]; n taps -> the per-position values: a, b, qa, qb (int64) and how many
    positions took each exceptional branch"""
    g_ = window(n)
    mu1, mu2 = filt(X, g_), filt(Y, g_)
    s1 = filt(X * X, g_) - mu1 * mu1
    s2 = filt(Y * Y, g_) - mu2 * mu2
    s12 = filt(X * Y, g_) - mu1 * mu2
    s1 = np.where(s1 < 0.0, 0.0, s1)
    s2 = np.where(s2 < 0.0, 0.0, s2)
    g = s12 / (s1 + EPS)
    sv = s2 - g * s12
    k1 = s1 < EPS
    g, sv, s1 = np.where(k1, 0.0, g), np.where(k1, s2, sv), np.where(k1, 0.0, s1)
    k2 = s2 < EPS
    g, sv = np.where(k2, 0.0, g), np.where(k2, 0.0, sv)
    k3 = g < 0.0
    sv, g = np.where(k3, s2, sv), np.where(k3, 0.0, g)
    k4 = sv <= EPS
    sv = np.where(k4, EPS, sv)
    a = 1.0 + ((g * g) * s1) / (sv + 2.0)
    b = 1.0 + s1 / 2.0
    qa = np.rint(ln_fixed(a) * 16777216.0).astype(np.int64)
    qb = np.rint(ln_fixed(b) * 16777216.0).astype(np.int64)
    return {"a": a, "b": b, "qa": qa, "qb": qb, "branches": dict(zip(BRANCHES, (int(k.sum()) for k in (k1, k2, k3, k4))))}


def plane_scales(x, y, depth):
    """x, y: one plane's SAMPLES on the two sides -> [position_terms(...)] of the four scales"""
    unit = 1.0 / float(1 << (depth - 8))
    X, Y = np.asarray(x).astype(np.float64) * unit, np.asarray(y).astype(np.float64) * unit
    out = []
    for s, n in enumerate(TAPS):
        if s:
            g = window(n)
            X, Y = filt(X, g)[0::2, 0::2], filt(Y, g)[0::2, 0::2]
        out.append(position_terms(X, Y, n))
    return out


def ratio(num, den):
    return 1.0 if den == 0 else float(num) / float(den)


def plane_vif(ref, test, depth, sub):
    """ref, test: the planes' SAMPLES (sample() already applied), [(h_p, w_p) integer arrays] -> ce_plane_vif_scores as a dict,
    with "branches"[p][s] = {branch: positions} beside it"""
    h, w = ref[0].shape
    assert w >= MIN_SIDE and h >= MIN_SIDE
    assert [p.shape[::-1] for p in ref] == plane_sizes(w, h, sub) == [p.shape[::-1] for p in test]
    out = {"n_planes": len(ref), "ran": [0] * 3, "num_q": [[0] * 4 for _ in range(3)], "den_q": [[0] * 4 for _ in range(3)],
           "n_pos": [[0] * 4 for _ in range(3)], "vif_scale": [[math.nan] * 4 for _ in range(3)], "vifp": [math.nan] * 3,
           "branches": [None] * 3}
    for p in range(len(ref)):
        ph, pw = ref[p].shape
        sizes = scale_sizes(pw, ph)
        if not sizes:
            continue
        out["ran"][p] = 1
        scales = plane_scales(ref[p], test[p], depth)
        out["branches"][p] = [t["branches"] for t in scales]
        for s, t in enumerate(scales):
            n = (sizes[s][0] - TAPS[s] + 1) * (sizes[s][1] - TAPS[s] + 1)
            assert t["qa"].size == n and t["qa"].min() >= 0 and t["qb"].min() >= 0 and max(t["qa"].max(), t["qb"].max()) < 1 << 28
            num, den = sum(int(v) for v in t["qa"].reshape(-1)), sum(int(v) for v in t["qb"].reshape(-1))
            out["num_q"][p][s], out["den_q"][p][s], out["n_pos"][p][s] = num, den, n
            out["vif_scale"][p][s] = ratio(num, den)
        out["vifp"][p] = ratio(sum(out["num_q"][p]), sum(out["den_q"][p]))
    return out
