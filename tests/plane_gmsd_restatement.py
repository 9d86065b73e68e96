"""GMSD of a decoder's planes as include/ce_metrics.h defines it (ce_yuv_plane_gmsd), restated in numpy
operation by operation: the 2 x 2 sums, the Prewitt sums and the squared gradient magnitude in int64, the five f64 operations
of a position each one numpy operation, so that each is rounded where the header rounds it, and the sums, the variance and the
finishing in Python integers.  The planes, their sizes and the sample rule are tests/plane_fidelity_restatement.py's,
imported, not copied.  The device equals this on every integer."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plane_fidelity_restatement import SUB_400, SUB_420, SUB_422, SUB_444, plane_sizes, sample  # noqa: E402,F401

TWO32 = 1 << 32


def k_of(depth):
    """K = 24480 * 4^(d - 8): 144 * 170 at the depth's scale"""
    return 24480 * 4 ** (depth - 8)


def sums_2x2(v):
    """v[ph][pw] samples -> S[H2][W2] int64, a sample outside the plane counting 0"""
    v = np.asarray(v).astype(np.int64)
    ph, pw = v.shape
    padded = np.zeros((2 * ((ph + 1) // 2), 2 * ((pw + 1) // 2)), np.int64)
    padded[:ph, :pw] = v
    return padded[0::2, 0::2] + padded[0::2, 1::2] + padded[1::2, 0::2] + padded[1::2, 1::2]


def magnitude2(v):
    """v -> A[H2][W2] int64 = Gx * Gx + Gy * Gy, S outside the grid counting 0"""
    s = sums_2x2(v)
    h2, w2 = s.shape
    e = np.zeros((h2 + 2, w2 + 2), np.int64)
    e[1:-1, 1:-1] = s
    left = e[0:h2, 0:w2] + e[1:h2 + 1, 0:w2] + e[2:h2 + 2, 0:w2]
    right = e[0:h2, 2:w2 + 2] + e[1:h2 + 1, 2:w2 + 2] + e[2:h2 + 2, 2:w2 + 2]
    up = e[0:h2, 0:w2] + e[0:h2, 1:w2 + 1] + e[0:h2, 2:w2 + 2]
    down = e[2:h2 + 2, 0:w2] + e[2:h2 + 2, 1:w2 + 1] + e[2:h2 + 2, 2:w2 + 2]
    gx, gy = left - right, up - down
    return gx * gx + gy * gy


def similarity(ref, test, depth):
    """the planes' samples -> (g float64 [H2][W2], q int64 [H2][W2] as Python-sized integers fit: q <= 2^32)"""
    k = k_of(depth)
    a_ref, a_test = magnitude2(ref), magnitude2(test)
    m_ref, m_test = np.sqrt(a_ref.astype(np.float64)), np.sqrt(a_test.astype(np.float64))
    prod = m_ref * m_test
    num = (2.0 * prod) + float(k)
    den = (a_ref + a_test + k).astype(np.float64)  # under 2^35: exact
    g = num / den
    q = np.rint(g * 4294967296.0).astype(np.int64)
    return g, q


def finish(sum_q, sum_q2, n_pos):
    """-> (gmsd, gmsm) from the exact integers"""
    v = n_pos * sum_q2 - sum_q * sum_q
    assert v >= 0
    scale = float(n_pos) * 4294967296.0
    return math.sqrt(float(v)) / scale, float(sum_q) / scale  # float(int) is the nearest double, ties to even


def plane_gmsd(ref, test, depth, sub):
    """ref, test: the planes' SAMPLES (sample() already applied), [(h_p, w_p) integer arrays] -> ce_plane_gmsd_scores as a dict;
    sum_q2 as [low 64 bits, high 64 bits] and as one integer in sum_q2_int"""
    h, w = ref[0].shape
    assert [p.shape[::-1] for p in ref] == plane_sizes(w, h, sub) == [p.shape[::-1] for p in test]
    out = {"n_planes": len(ref), "sum_q": [0] * 3, "sum_q2": [[0, 0] for _ in range(3)], "sum_q2_int": [0] * 3, "n_pos": [0] * 3,
           "gmsd": [math.nan] * 3, "gmsm": [math.nan] * 3, "max_dis": [0] * 3}
    for p in range(len(ref)):
        _, q = similarity(ref[p], test[p], depth)
        qs = [int(x) for x in q.reshape(-1)]
        assert all(1 <= x <= TWO32 for x in qs)
        n, s, s2 = len(qs), sum(qs), sum(x * x for x in qs)
        out["n_pos"][p], out["sum_q"][p], out["sum_q2_int"][p] = n, s, s2
        out["sum_q2"][p] = [s2 & ((1 << 64) - 1), s2 >> 64]
        out["max_dis"][p] = TWO32 - min(qs)
        out["gmsd"][p], out["gmsm"][p] = finish(s, s2, n)
    return out
