"""What the tests of the fused Y'CbCr + CICP ingest share (include/ce_metrics.h: ce_batch_set_*_yuv_cicp, ce_yuv_to_linear;
DESIGN.md section 16): the composed restatement - tests/yuv_restatement.py's yuv_to_rgb at D = c.depth, then
tests/cicp_restatement.py's to_linear - and one deterministic list of cases that covers every shape in every slot and every
pair of the options."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import yuv_restatement as Y  # noqa: E402

WHITE = 203.0
# every crop and alignment branch: one pixel, one block, cropped groups of 1, 7 and 4 pixels, widths under 8 (the per-sample
# luma route), odd heights (a last row pair of one row), w * h odd (slots 1 and 2 start 4, 8 or 12 bytes off a 16-byte
# boundary), rows whose start walks through the residues (w = 9, 17, 97, 301), more than one block, a single block row pair
SHAPES = ((1, 1), (2, 2), (7, 3), (8, 2), (9, 3), (16, 4), (17, 5), (100, 76), (97, 131), (301, 9), (9, 301))
SLOTS = (0, 1, 2)
OPTIONS = {
    "sub": (Y.SUB_444, Y.SUB_422, Y.SUB_420, Y.SUB_400),
    "layout": (Y.PLANAR, Y.SEMIPLANAR),
    "sample": ((8, False), (10, False), (10, True), (12, False), (12, True)),  # depth, MSB-aligned (P010 / P012)
    "mode": (Y.NEAREST, Y.TRIANGLE),
    "range": (Y.FULL, Y.LIMITED),
    "matrix": (Y.BT601, Y.BT709, Y.BT2020),
    "prim": R.PRIMARIES,
    "tr": R.TRANSFERS,
    "grid16": (False, True),  # c.depth: the samples' own depth, or 16
    "pad": (0, 1, 64),        # pitch beyond the row, in samples: 8-bit planes get an odd byte pitch from 1
    "device": (False, True),  # CE_MEM_DEVICE planes (the GPU test; the host build has no such thing)
}


def _pairs(case):
    keys = sorted(case)
    return {(a, case[a], b, case[b]) for a, b in itertools.combinations(keys, 2)}


def cases():
    """Two cases per (shape, slot), the first for the reference slab and the second for the test slab, their options chosen
    greedily (best of 40 seeded draws) for the pairs not met yet; every pair of option values is asserted covered."""
    rng = np.random.default_rng(20250916)
    names = list(OPTIONS)
    seen, out = set(), []
    for (w, h), slot, slab in itertools.product(SHAPES, SLOTS, (0, 1)):
        best, best_new = None, -1
        for _ in range(40):
            c = {k: OPTIONS[k][int(rng.integers(len(OPTIONS[k])))] for k in names}
            c.update(shape=(w, h), slot=slot)
            new = len(_pairs(c) - seen)
            if new > best_new:
                best, best_new = c, new
        seen |= _pairs(best)
        best.update(slab=slab, seed=1000 + len(out))
        out.append(best)
    for a, b in itertools.combinations(sorted(names), 2):
        for va, vb in itertools.product(OPTIONS[a], OPTIONS[b]):
            assert (a, va, b, vb) in seen, (a, va, b, vb)
    for shape in SHAPES:
        for sub in OPTIONS["sub"]:
            assert ("shape", shape, "sub", sub) in seen, (shape, sub)
    return out


def c_depth(case):
    return 16 if case["grid16"] else case["sample"][0]


def planes_of(case):
    """random planes of the case: low-aligned deep samples include values above 2^d - 1, which ingest clamps"""
    (w, h), (d, msb) = case["shape"], case["sample"]
    return Y.random_planes(np.random.default_rng(case["seed"]), w, h, case["sub"], d, msb, over=True)


def composed(y, cb, cr, w, h, sub, matrix, range_, mode, d, msb, prim, tr, D, white=WHITE):
    """the definition: integer RGB of depth D by the Y'CbCr restatement, then linear light by the CICP restatement"""
    rgb = Y.yuv_to_rgb(y, cb, cr, w, h, sub, matrix, range_, mode, d, D, msb)
    return R.to_linear(rgb, prim, tr, D, white)


def want_of(case, planes=None):
    (w, h), (d, msb) = case["shape"], case["sample"]
    y, cb, cr = planes if planes is not None else planes_of(case)
    return composed(y, cb, cr, w, h, case["sub"], case["matrix"], case["range"], case["mode"], d, msb, case["prim"], case["tr"], c_depth(case))
