"""What the SSIM / MS-SSIM map tests share: msssim_cases' content, the shapes - each chosen for one way the map kernel can go
wrong - and the restatement's map for a pair, computed once per process and handed out read-only
(tests/msssim_map_restatement.py)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as K  # noqa: E402
import msssim_map_restatement as R  # noqa: E402

BLOCKS = [1, 2, 4, 8, 16, 32, 64]
U32_MAX = R.U32_MAX
# thresholds in units of 2^-32: an SSIM under 1, 0.99, 0.95, 0.9, 0.8, 0.7, 0.5, and the one nothing exceeds
THR8 = [0, R.Q32 // 100, R.Q32 // 20, R.Q32 // 10, R.Q32 // 5, 3 * (R.Q32 // 10), R.Q32 // 2, U32_MAX]

# (w, h, depth, levels, [level, ...])
ONE_LEVEL = [(w, h, 8, 1, [0]) for w, h in K.ONE_LEVEL]  # one position, one row, one column of positions
ODD_ROWS = [(43, 27, 8, 1, [0]),  # vw = 33 is odd: map rows are misaligned for the 8-byte store; two tiles each way
            (44, 27, 8, 1, [0])]  # vw = 34: the last lane pair has one valid output
TILE_EDGES = [(w, h, 8, 5, [0]) for w, h in K.TILE_EDGES]  # the valid region one under, at, one over a multiple of the tile
FIVE = [(176, 163, 8, 5, [0, 1, 2, 3, 4])]  # every level; level 4 is a single position
DEEP = [(192, 256, 10, 5, [0, 2]), (12, 11, 16, 1, [0])]
SHAPES = ONE_LEVEL + ODD_ROWS + TILE_EDGES + FIVE + DEEP


@functools.lru_cache(maxsize=None)
def level_q(w, h, depth, levels, level, seed=0, ref_seed=None):
    """int64 [2, 3, vh, vw] of pair(w, h, depth, seed)'s test against pair(w, h, depth, ref_seed or seed)'s reference"""
    ref = K.pair(w, h, depth, seed if ref_seed is None else ref_seed)[0]
    q = R.level_q(ref, K.pair(w, h, depth, seed)[1], depth, levels, level)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def expected(w, h, depth, levels, level, what="ssim", block=1, seed=0, ref_seed=None):
    """uint32 [3, ch, cw]: the restatement's map of that pair"""
    m = R.cells(R.value(level_q(w, h, depth, levels, level, seed, ref_seed)[R.WHAT[what]]), block)
    m.setflags(write=False)
    return m


def expected_over(w, h, depth, levels, level, what, thresholds, seed=0, ref_seed=None):
    return R.over(expected(w, h, depth, levels, level, what, 1, seed, ref_seed), thresholds)


def patched(w, h, x0, y0, side=6):
    """pair(w, h, 8)'s reference, and the same with a side x side patch at (x0, y0) inverted"""
    ref = K.pair(w, h, 8)[0]
    test = ref.copy()
    test[y0:y0 + side, x0:x0 + side] = 255 - test[y0:y0 + side, x0:x0 + side]
    return ref, test
