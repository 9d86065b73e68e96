"""What the tests of the fused Y'CbCr + ICC ingest share (include/ce_metrics.h: ce_batch_set_*_yuv_icc, ce_yuv_icc_to_*;
DESIGN.md section 25): the composed restatement - tests/yuv_restatement.py's yuv_to_rgb at D = rgb_depth, then
tests/icc_restatement.py's or tests/icc_lut_restatement.py's to_linear / to_srgb - and one deterministic list of cases that
covers every shape in slots 0 to 2 of both slabs and every pair of the options."""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_lut_restatement as LR  # noqa: E402
import icc_restatement as R  # noqa: E402
import yuv_linear_cases as L  # noqa: E402
import yuv_restatement as Y  # noqa: E402

SHAPES = L.SHAPES
SLOTS = (0, 1, 2)  # every crop, store-width and multi-block branch of the frame (a slot's start moves the rows' residues)
# name -> (flavour, fixture, interpolation): two matrix/TRC profiles - M = I, and a matrix with a `para` curve - and two LUT-based
# ones, one per interpolation - an mAB with a 5^3 CLUT, power M curves and a matrix into PCS XYZ, and an mft2 with a 9^3 CLUT and
# sampled output tables into legacy Lab
PROFILES = {
    "srgb_para": ("matrix", "srgb_para", None),
    "p3": ("matrix", "p3", None),
    "mab_xyz_tet": ("lut", "mab_xyz", LR.TETRAHEDRAL),
    "mft2_lab_tri": ("lut", "mft2_lab", LR.TRILINEAR),
}
# the destination: (slot kind, the slot's depth): a linear batch, an RGB8 batch, deep sides of 10, 12 and 16
DESTS = (("lin", 0), ("u8", 8), ("u16", 10), ("u16", 12), ("u16", 16))
OPTIONS = {k: L.OPTIONS[k] for k in ("sub", "layout", "sample", "mode", "range", "matrix", "pad", "device")}
OPTIONS.update(profile=tuple(PROFILES), grid16=(False, True), dest=DESTS)


def profile_bytes(name: str) -> bytes:
    flavour, fixture, _ = PROFILES[name]
    return (R.fixtures() if flavour == "matrix" else LR.fixtures())[fixture]


def _pairs(case):
    keys = sorted(case)
    return {(a, case[a], b, case[b]) for a, b in itertools.combinations(keys, 2)}


def cases():
    """Two cases per (shape, slot), the first for the reference slab and the second for the test slab, their options chosen
    greedily (best of 60 seeded draws) for the pairs not met yet.  Asserted: every pair of option values is covered, every
    shape meets every subsampling, every shape meets both profile flavours."""
    rng = np.random.default_rng(20261019)
    names = list(OPTIONS)
    seen, out = set(), []
    for (w, h), slot, slab in itertools.product(SHAPES, SLOTS, (0, 1)):
        best, best_new = None, -1
        for _ in range(60):
            c = {k: OPTIONS[k][int(rng.integers(len(OPTIONS[k])))] for k in names}
            c.update(shape=(w, h), slot=slot)
            new = len(_pairs(c) - seen)
            if new > best_new:
                best, best_new = c, new
        seen |= _pairs(best)
        best.update(slab=slab, seed=3000 + len(out))
        out.append(best)
    for a, b in itertools.combinations(sorted(names), 2):
        for va, vb in itertools.product(OPTIONS[a], OPTIONS[b]):
            assert (a, va, b, vb) in seen, (a, va, b, vb)
    for shape in SHAPES:
        for sub in OPTIONS["sub"]:
            assert ("shape", shape, "sub", sub) in seen, (shape, sub)
        met = {PROFILES[c["profile"]][0] for c in out if c["shape"] == shape}
        assert met == {"matrix", "lut"}, (shape, met)
    return out


def rgb_depth(case):
    return 16 if case["grid16"] else case["sample"][0]


def planes_of(case):
    """random planes of the case: low-aligned deep samples include values above 2^d - 1, which ingest clamps"""
    (w, h), (d, msb) = case["shape"], case["sample"]
    return Y.random_planes(np.random.default_rng(case["seed"]), w, h, case["sub"], d, msb, over=True)


def apply_profile(rgb, profile: str, D: int, dest):
    """integer RGB of depth D [h, w, 3] -> what the slot `dest` = (kind, depth) stores, by the ICC restatement of the profile's flavour"""
    flavour, _, interpolation = PROFILES[profile]
    p = profile_bytes(profile)
    kind, depth_out = dest
    if flavour == "matrix":
        return R.to_linear(rgb, p, D) if kind == "lin" else R.to_srgb(rgb, p, D, depth_out, out16=kind == "u16")
    if kind == "lin":
        return LR.to_linear(rgb, p, D, interpolation)
    return LR.to_srgb(rgb, p, D, depth_out, out16=kind == "u16", interpolation=interpolation)


def composed(y, cb, cr, w, h, sub, matrix, range_, mode, d, msb, profile: str, D: int, dest):
    """the definition: integer RGB of depth D by the Y'CbCr restatement, then the profile by the ICC restatement"""
    rgb = Y.yuv_to_rgb(y, cb, cr, w, h, sub, matrix, range_, mode, d, D, msb)
    return apply_profile(rgb, profile, D, dest)


def want_of(case, planes=None):
    (w, h), (d, msb) = case["shape"], case["sample"]
    y, cb, cr = planes if planes is not None else planes_of(case)
    return composed(y, cb, cr, w, h, case["sub"], case["matrix"], case["range"], case["mode"], d, msb, case["profile"], rgb_depth(case), case["dest"])
