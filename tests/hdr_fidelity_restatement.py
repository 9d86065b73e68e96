"""HDR fidelity of linear batches (include/ce_metrics.h: ce_batch_hdr_fidelity, ce_eval_pair_hdr_fidelity, ce_pq_code_thresholds,
ce_hdr_fidelity_matrices) restated in numpy: PSNR in the PQ domain and the Delta E ITP of Rec. ITU-R
BT.2124 of a pair of linear-light images with sRGB primaries.  A helper, not a test.

The thresholds and the two matrices are built in Python floats (IEEE f64, the host libm's pow - what the library's host code
calls) and rounded once to float32; the per-pixel part is numpy float32 whose products and sums are each rounded separately,
integer work in int64, and the per-pixel Delta E in numpy float64 with a correctly rounded sqrt.  Everything that is summed
is an integer, so the device equals this bit for bit whatever order it adds in."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402

DEPTHS = (10, 12, 16)
WHITES = (80.0, 203.0, 10000.0)
# BT.2100: LMS <- BT.2020 RGB, times 4096 (every entry / 4096 is exact in float32)
LMS_4096 = ((1688, 2146, 262), (683, 2951, 462), (99, 309, 3688))
Q20 = float(1 << 20)


@functools.lru_cache(maxsize=None)
def _thresholds(depth: int, white_nits: float) -> np.ndarray:
    maxv = (1 << depth) - 1
    white = float(np.float32(white_nits))  # the ABI carries it as a float
    out = np.array([R.pq_nits((c - 0.5) / maxv) / white for c in range(1, maxv + 1)], np.float64).astype(np.float32)
    out.setflags(write=False)
    return out


def thresholds(depth: int, white_nits: float) -> np.ndarray:
    """T[1 .. maxv] at indices 0 .. maxv - 1: T[c] = f32(PQ_EOTF((c - 0.5) / maxv) / white_nits)."""
    return _thresholds(int(depth), float(white_nits))


def matrices():
    """A = the inverse of ce_colour_matrix(9) - of the float32 matrix the ingest multiplies by, so that A undoes it as well as
    float32 can - taken in f64 by the adjugate and rounded once to float32; B = BT.2100's LMS <- RGB."""
    a = np.array(R._inv3([float(v) for v in R.colour_matrix(9).reshape(-1)]), np.float64).astype(np.float32).reshape(3, 3)
    b = (np.array(LMS_4096, np.float64) / 4096.0).astype(np.float32)
    return a, b


def code(x, depth: int, white_nits: float) -> np.ndarray:
    """The number of thresholds <= x: negatives, zero and NaN give 0, anything at or above the last one maxv."""
    x = np.asarray(x, np.float32)
    c = np.searchsorted(thresholds(depth, white_nits), x, side="right").astype(np.int64)
    return np.where(np.isnan(x), 0, c)  # numpy sorts NaN behind everything


def _mat3(m, v):
    r, g, b = v[..., 0], v[..., 1], v[..., 2]
    out = np.stack([(m[i, 0] * r + m[i, 1] * g) + m[i, 2] * b for i in range(3)], axis=-1)
    assert out.dtype == np.float32
    return out


def codes(rgb, depth: int, white_nits: float):
    """[..., 3] float32 linear light, sRGB primaries -> (Rc Gc Bc, Lc Mc Sc), int64 [..., 3] each."""
    a, b = matrices()
    q = _mat3(a, np.asarray(rgb, np.float32))
    lms = _mat3(b, q)
    return code(q, depth, white_nits), code(lms, depth, white_nits)


def ictcp(lms_codes):
    """BT.2100's ICtCp of PQ codes, times 4096 * maxv, exactly: int64 (i, ct, cp)."""
    lc, mc, sc = (lms_codes[..., k] for k in range(3))
    return 2048 * (lc + mc), 6610 * lc - 13613 * mc + 7003 * sc, 17933 * lc - 17390 * mc - 543 * sc


def pixel_q20(ref, test, depth: int, white_nits: float):
    """Per pixel: the squared PQ code differences summed over R, G, B (int64) and Delta E ITP in units of 2^-20 (int64)."""
    maxv = (1 << depth) - 1
    (rq, rl), (tq, tl) = codes(ref, depth, white_nits), codes(test, depth, white_nits)
    d = rq - tq
    sq = (d * d).sum(axis=-1)
    di, dct, dcp = (a - b for a, b in zip(ictcp(rl), ictcp(tl)))
    fi, fct, fcp = di.astype(np.float64), dct.astype(np.float64), dcp.astype(np.float64)
    s = (fi * fi + 0.25 * (fct * fct)) + fcp * fcp
    e = 720.0 * np.sqrt(s) / float(4096 * maxv)
    return sq, np.rint(e * Q20).astype(np.int64)


def finish(pq_sse: int, itp_sum: int, itp_max: int, n_pixels: int, depth: int):
    """The host's finish in f64: (pq_psnr, delta_e_itp_mean, delta_e_itp_max)."""
    maxv = float((1 << depth) - 1)
    mse = float(pq_sse) / float(n_pixels * 3)
    psnr = math.inf if mse == 0.0 else 10.0 * math.log10(maxv * maxv / mse)
    return psnr, float(itp_sum) / Q20 / float(n_pixels), float(itp_max) / Q20


def fidelity(ref, test, depth: int, white_nits: float) -> dict:
    ref, test = np.asarray(ref, np.float32).reshape(-1, 3), np.asarray(test, np.float32).reshape(-1, 3)
    assert ref.shape == test.shape
    sq, k = pixel_q20(ref, test, depth, white_nits)
    pq_sse, itp_sum, itp_max = int(sq.sum()), int(k.sum()), int(k.max())
    psnr, mean, mx = finish(pq_sse, itp_sum, itp_max, ref.shape[0], depth)
    return dict(pq_sse=pq_sse, itp_sum_q20=itp_sum, itp_max_q20=itp_max, pq_psnr=psnr, delta_e_itp_mean=mean, delta_e_itp_max=mx)
