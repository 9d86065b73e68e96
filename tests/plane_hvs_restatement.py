"""PSNR-HVS and PSNR-HVS-M of a decoder's planes as include/ce_metrics.h defines them (ce_yuv_plane_hvs),
restated in numpy operation by operation: the two tables from JPEG Annex K's luminance table, the direct 8-point DCT with its
eight literals, the contrast mask of Ponomarenko et al., the quantisation of every coefficient's weighted squared difference and
the finishing.  Every f64 operation below is one numpy operation, so it is rounded where the header rounds it; the sums are
Python integers.  The planes, their sizes and the sample rule are tests/plane_fidelity_restatement.py's, imported, not copied.
The device equals this on every integer."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plane_fidelity_restatement import SUB_400, SUB_420, SUB_422, SUB_444, plane_sizes, sample  # noqa: E402,F401

# JPEG (ITU-T T.81) Annex K, table K.1, in natural order
Q = np.array([[16, 11, 10, 16, 24, 40, 51, 61],
              [12, 12, 14, 19, 26, 58, 60, 55],
              [14, 13, 16, 24, 40, 57, 69, 56],
              [14, 17, 22, 29, 51, 87, 80, 62],
              [18, 22, 37, 56, 68, 109, 103, 77],
              [24, 35, 55, 64, 81, 104, 113, 92],
              [49, 64, 78, 87, 103, 121, 120, 101],
              [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.int64)
CSF = 25.73509 / Q.astype(np.float64)
MC = 100.0 / (Q * Q).astype(np.float64)

# g[0] = sqrt(1 / 8), g[m] = cos(m pi / 16) / 2: the nearest f64, the same text as plane_hvs_kernel.h's kHvsG
G_TEXT = ["0x1.6a09e667f3bcdp-2", "0x1.f6297cff75cb0p-2", "0x1.d906bcf328d46p-2", "0x1.a9b66290ea1a3p-2",
          "0x1.6a09e667f3bcdp-2", "0x1.1c73b39ae68c8p-2", "0x1.87de2a6aea963p-3", "0x1.8f8b83c69a60bp-4"]
G = [float.fromhex(t) for t in G_TEXT]


def dct_entry(k, j):
    """T[k][j] = sqrt(1/8) for k = 0, else cos((2j + 1) k pi / 16) / 2 as +-g[m]: a = (2j + 1) k mod 32 folded by cos(2 pi - x) =
    cos x and cos(pi - x) = -cos x into m in 1 .. 7 (a is never 0, 8, 16 or 24 for k in 1 .. 7)"""
    if k == 0:
        return G[0]
    a = ((2 * j + 1) * k) % 32
    if a > 16:
        a = 32 - a
    sign = 1.0
    if a > 8:
        a, sign = 16 - a, -1.0
    assert 1 <= a <= 7
    return sign * G[a]


T = np.array([[dct_entry(k, j) for j in range(8)] for k in range(8)])


def dct8(x):
    """x[..., 8] -> out[..., 8] along the last axis: products separately rounded, sums left to right"""
    out = np.empty(x.shape, np.float64)
    for k in range(8):
        s = T[k][0] * x[..., 0] + T[k][1] * x[..., 1]
        for j in range(2, 8):
            s = s + T[k][j] * x[..., j]
        out[..., k] = s
    return out


def dct2(z):
    """z[..., 8 rows, 8 columns] -> D[..., k, l]: along the rows of the block first, then down the columns"""
    rows = dct8(np.asarray(z, np.float64))
    return np.swapaxes(dct8(np.swapaxes(rows, -1, -2)), -1, -2)


def n_blocks_of(pw, ph, step):
    return 0 if pw < 8 or ph < 8 else ((pw - 8) // step + 1) * ((ph - 8) // step + 1)


def blocks_of(plane, step):
    """-> [n_blocks, 8, 8] int64, block rows first"""
    ph, pw = plane.shape
    p = np.asarray(plane).astype(np.int64)
    out = [p[y:y + 8, x:x + 8] for y in range(0, ph - 7, step) for x in range(0, pw - 7, step)] if pw >= 8 and ph >= 8 else []
    return np.stack(out) if out else np.zeros((0, 8, 8), np.int64)


def spread(z):
    """I(z) = N sum z^2 - (sum z)^2 over the last two axes, exact"""
    n = z.shape[-1] * z.shape[-2]
    s = z.sum(axis=(-1, -2))
    return n * (z * z).sum(axis=(-1, -2)) - s * s


def masks(z, D):
    """z [n, 8, 8] int64, D its DCT -> mask [n]"""
    t = (D * D) * MC
    cols = []
    for l in range(8):
        c = t[:, 1, 0] if l == 0 else t[:, 0, l]
        for k in range(2 if l == 0 else 1, 8):
            c = c + t[:, k, l]
        cols.append(c)
    m = ((cols[0] + cols[1]) + (cols[2] + cols[3])) + ((cols[4] + cols[5]) + (cols[6] + cols[7]))
    whole = spread(z)
    quads = (spread(z[:, :4, :4]) + spread(z[:, :4, 4:])) + (spread(z[:, 4:, :4]) + spread(z[:, 4:, 4:]))
    pop = np.zeros(len(z), np.float64)
    nz = whole != 0
    pop[nz] = (63.0 * quads[nz].astype(np.float64)) / (15.0 * whole[nz].astype(np.float64))
    return np.sqrt(m * pop) / 32.0


def plane_blocks(x, y, depth, step):
    """x, y: one plane's SAMPLES on the two sides -> per-block results: q_hvs, q_hvsm [n, 8, 8] int64, the masks, and how
    often each branch of the threshold ran"""
    za, zb = blocks_of(x, step), blocks_of(y, step)
    DA, DB = dct2(za), dct2(zb)
    ma, mb = masks(za, DA), masks(zb, DB)
    M = np.maximum(ma, mb)
    u = np.abs(DA - DB)
    t = M[:, None, None] / MC
    below = u < t
    um = np.where(below, 0.0, u - t)
    um[:, 0, 0] = u[:, 0, 0]
    unit = float(1 << (36 - 2 * depth))

    def quantise(v):
        w = v * CSF
        return np.rint((w * w) * unit).astype(np.int64)

    ac = np.ones((8, 8), bool)
    ac[0, 0] = False
    return {"q_hvs": quantise(u), "q_hvsm": quantise(um), "mask_a": ma, "mask_b": mb, "M": M, "D_a": DA, "D_b": DB,
            "n_below": int(below[:, ac].sum()), "n_at_or_above": int((~below)[:, ac].sum()), "n_unmasked": int((M == 0).sum())}


def finish(total, n_blocks, depth):
    """the exact sum -> the score, from the two 32-bit-split accumulators as the host forms it"""
    if n_blocks == 0:
        return math.nan
    if total == 0:
        return math.inf
    L = float((1 << depth) - 1)
    lo, hi = total & 0xffffffff, total >> 32
    S = ((float(hi) * 4294967296.0 + float(lo)) / float(1 << (36 - 2 * depth))) / (64.0 * n_blocks)
    return 10.0 * math.log10(L * L / S)


def plane_hvs(ref, test, depth, sub, step=8):
    """ref, test: the planes' SAMPLES (sample() already applied), [(h_p, w_p) integer arrays] -> ce_plane_hvs_scores as a dict:
    hvs_q[p] and hvsm_q[p] are [sum mod 2^32, sum >> 32]"""
    h, w = ref[0].shape
    assert 1 <= step <= 8 and w >= 8 and h >= 8
    assert [p.shape[::-1] for p in ref] == plane_sizes(w, h, sub) == [p.shape[::-1] for p in test]
    out = {"n_planes": len(ref), "step": step, "hvs_q": [[0, 0] for _ in range(3)], "hvsm_q": [[0, 0] for _ in range(3)],
           "n_blocks": [0] * 3, "psnr_hvs": [math.nan] * 3, "psnr_hvsm": [math.nan] * 3}
    for p in range(len(ref)):
        ph, pw = ref[p].shape
        n = out["n_blocks"][p] = n_blocks_of(pw, ph, step)
        if n == 0:
            continue
        b = plane_blocks(ref[p], test[p], depth, step)
        assert len(b["M"]) == n
        for name, key in (("hvs", "q_hvs"), ("hvsm", "q_hvsm")):
            total = sum(int(v) for v in b[key].reshape(n, 64).sum(axis=1))
            out[name + "_q"][p] = [total & 0xffffffff, total >> 32]
            out["psnr_" + name][p] = finish(total, n, depth)
    return out
