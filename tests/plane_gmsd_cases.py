"""What the GMSD tests share (ce_yuv_plane_gmsd): the shapes, each one way for the kernel to go wrong; the
content - tests/plane_hvs_cases.py's smooth pattern plus noise with its flat patch, so that positions with q = 2^32 occur, and
as a second kind the reference's pattern against a flat test, which drives q low; the restatement's result for a pair,
computed once per process and handed out unchanged (tests/plane_gmsd_restatement.py); and the comparison."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_gmsd_restatement as G  # noqa: E402
import plane_hvs_cases as HK  # noqa: E402

PLANAR, SEMIPLANAR = K.PLANAR, K.SEMIPLANAR
TW, TH = 64, 16  # plane_gmsd_kernel.h's kGmsdTileW, kGmsdTileH: positions a thread block (tests/test_plane_gmsd_cpu.py reads the header)
NOISY, FLAT_TEST = 0, 1

# (w, h, subsampling, depth, the test image's layout, msb_aligned)
SHAPES = [
    (1, 1, G.SUB_400, 8, PLANAR, False),                    # the smallest plane
    (2, 2, G.SUB_420, 8, SEMIPLANAR, False),                # chroma is 1 x 1
    (3, 3, G.SUB_444, 8, PLANAR, False),                    # odd both ways: the half sums
    (5, 1, G.SUB_400, 8, PLANAR, False),                    # a single row of positions: every neighbour above and below is outside
    (1, 5, G.SUB_400, 8, PLANAR, False),                    # a single column
    (2 * TW, 2 * TH, G.SUB_400, 8, PLANAR, False),          # exactly one tile
    (2 * TW - 1, 2 * TH - 1, G.SUB_444, 8, SEMIPLANAR, False),  # one tile, odd
    (2 * TW + 1, 2 * TH + 1, G.SUB_420, 8, PLANAR, False),  # one position into the next tile both ways, and that position is a half sum
    (4 * TW + 2, 2, G.SUB_400, 8, PLANAR, False),           # a single row of positions over three tiles
    (93, 67, G.SUB_420, 8, SEMIPLANAR, False),              # ragged edges, odd chroma
    (93, 67, G.SUB_420, 10, SEMIPLANAR, True),              # the shift
    (93, 67, G.SUB_422, 12, PLANAR, False),                 # the clamp's range
]


@functools.lru_cache(maxsize=None)
def planes(w, h, sub, depth, seed=0, kind=NOISY):
    """-> (ref, test).  NOISY: HK.planes.  FLAT_TEST: its reference against planes of L / 2 everywhere.  Read-only."""
    ref, test = HK.planes(w, h, sub, depth, seed)
    if kind == FLAT_TEST:
        flat = []
        for p in ref:
            q = np.full_like(p, ((1 << depth) - 1) // 2)
            q.setflags(write=False)
            flat.append(q)
        test = tuple(flat)
    return ref, test


@functools.lru_cache(maxsize=None)
def expected(w, h, sub, depth, seed=0, ref_seed=None, kind=NOISY):
    """the restatement on planes(..., seed, kind)'s test against planes(..., ref_seed or seed)'s reference"""
    ref = planes(w, h, sub, depth, seed if ref_seed is None else ref_seed)[0]
    return G.plane_gmsd(list(ref), list(planes(w, h, sub, depth, seed, kind)[1]), depth, sub)


def stored_planes(samples, sub, depth, layout=PLANAR, msb_aligned=False, pad_of=lambda row: -row % 16, seed=0):
    """K.host_planes with each stored plane's padding chosen from its own row length, pad_of(row bytes) -> bytes; as given,
    rows lie 16 bytes apart, so that from an aligned base every row admits the wide path"""
    rng = np.random.default_rng(seed)
    s = K.stored(samples, depth, msb_aligned)
    planes_ = [s[0]] if sub == G.SUB_400 else [s[0], K.interleave(s[1], s[2])] if layout == SEMIPLANAR else list(s)
    out = []
    for p in planes_:
        row = np.ascontiguousarray(p).view(np.uint8).reshape(p.shape[0], -1).shape[1]
        out.append(K.padded(p, pad_of(row), rng))
    return out


same = HK.same


def check(got, want, where=""):
    """got: a PlaneGmsdScores (codec_eval_amd), want: the restatement's dict: every integer equal, the doubles by
    plane_hvs_cases.same (they are finished from equal integers by correctly rounded operations: equal in practice), NaN
    matching NaN"""
    assert got.n_planes == want["n_planes"], (where, got.n_planes)
    assert list(got.n_pos) == want["n_pos"], (where, got.n_pos, want["n_pos"])
    assert list(got.sum_q) == want["sum_q"], (where, "sum_q", got.sum_q, want["sum_q"])
    assert [list(q) for q in got.sum_q2] == want["sum_q2"], (where, "sum_q2", got.sum_q2, want["sum_q2"])
    assert list(got.sum_q2_int) == want["sum_q2_int"], (where, "sum_q2_int")
    assert list(got.max_dis) == want["max_dis"], (where, "max_dis", got.max_dis, want["max_dis"])
    for p in range(3):
        assert same(got.gmsd[p], want["gmsd"][p]), (where, "gmsd", p, got.gmsd[p], want["gmsd"][p])
        assert same(got.gmsm[p], want["gmsm"][p]), (where, "gmsm", p, got.gmsm[p], want["gmsm"][p])
