"""What the PSNR-HVS / PSNR-HVS-M tests share (ce_yuv_plane_hvs): the shapes, each one way for the kernel
to go wrong; the content - tests/plane_fidelity_cases.py's smooth pattern plus noise with a flat patch laid into both sides
where a plane has room for one, so that blocks under the mask's threshold, over it and without a mask all occur; the
restatement's result for a pair, computed once per process and handed out unchanged (tests/plane_hvs_restatement.py); and the
comparison."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_hvs_restatement as H  # noqa: E402

PLANAR, SEMIPLANAR = K.PLANAR, K.SEMIPLANAR

# (w, h, subsampling, depth, step, the test image's layout, msb_aligned)
SHAPES = [
    (8, 8, H.SUB_400, 8, 8, PLANAR, False),        # one block
    (8, 8, H.SUB_420, 8, 8, SEMIPLANAR, False),    # chroma has no block
    (16, 16, H.SUB_420, 8, 8, SEMIPLANAR, False),  # chroma exactly one
    (9, 8, H.SUB_444, 8, 8, PLANAR, False),        # a leftover on one side
    (15, 15, H.SUB_422, 8, 8, SEMIPLANAR, False),  # and on both
    (15, 16, H.SUB_444, 8, 7, PLANAR, False),      # two overlapping blocks
    (12, 10, H.SUB_444, 8, 1, SEMIPLANAR, False),  # 15 blocks, every overlap
    (93, 67, H.SUB_420, 8, 8, SEMIPLANAR, False),  # 88 blocks: a last thread block a quarter empty, ragged edges, odd chroma
    (93, 67, H.SUB_420, 8, 7, PLANAR, False),
    (93, 67, H.SUB_420, 8, 4, SEMIPLANAR, False),
    (264, 8, H.SUB_400, 8, 8, PLANAR, False),      # 33 blocks: one past a thread block, a single block row
    (93, 67, H.SUB_420, 10, 8, SEMIPLANAR, True),  # the shift
    (93, 67, H.SUB_420, 12, 7, PLANAR, False),     # the clamp's range
]
PATCH = (8, 24, 8, 32)  # rows 8 .. 23, columns 8 .. 31: holds a whole block at every step


@functools.lru_cache(maxsize=None)
def planes(w, h, sub, depth, seed=0):
    """-> (ref, test): K.planes with the flat patch, 100 / 255 of L on the reference and 3 / 255 of L more on the test"""
    L = (1 << depth) - 1
    out = []
    for side, planes_ in enumerate(K.planes(w, h, sub, depth, seed)):
        mine = []
        for p in planes_:
            q = p.copy()
            if q.shape[0] >= PATCH[1] and q.shape[1] >= PATCH[3]:
                q[PATCH[0]:PATCH[1], PATCH[2]:PATCH[3]] = (100 + 3 * side) * L // 255
            q.setflags(write=False)
            mine.append(q)
        out.append(tuple(mine))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(w, h, sub, depth, step, seed=0, ref_seed=None):
    """the restatement on planes(..., seed)'s test against planes(..., ref_seed or seed)'s reference"""
    ref = planes(w, h, sub, depth, seed if ref_seed is None else ref_seed)[0]
    return H.plane_hvs(list(ref), list(planes(w, h, sub, depth, seed)[1]), depth, sub, step)


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= 1e-14 * abs(b)


def check(got, want, where=""):
    """got: a PlaneHvsScores (codec_eval_amd), want: the restatement's dict: every integer equal, the doubles within 1e-14
    relative (libm's log10 is the unpinned operation), NaN matching NaN and infinity infinity"""
    assert got.n_planes == want["n_planes"] and got.step == want["step"], (where, got.n_planes, got.step)
    assert list(got.n_blocks) == want["n_blocks"], (where, got.n_blocks, want["n_blocks"])
    for p in range(3):
        assert list(got.hvs_q[p]) == want["hvs_q"][p], (where, "hvs_q", p, got.hvs_q[p], want["hvs_q"][p])
        assert list(got.hvsm_q[p]) == want["hvsm_q"][p], (where, "hvsm_q", p, got.hvsm_q[p], want["hvsm_q"][p])
        assert same(got.psnr_hvs[p], want["psnr_hvs"][p]), (where, "psnr_hvs", p, got.psnr_hvs[p], want["psnr_hvs"][p])
        assert same(got.psnr_hvsm[p], want["psnr_hvsm"][p]), (where, "psnr_hvsm", p, got.psnr_hvsm[p], want["psnr_hvsm"][p])
