"""What the VIFp tests share (ce_yuv_plane_vif): the shapes, each one way for the kernels to go wrong; the
content - tests/plane_fidelity_cases.py's smooth pattern plus noise with three patches laid in where a plane has room: one flat
on both sides at different levels (no reference variance, no test variance), one where the test is L - ref (a negative gain)
and one where the test equals the reference (no residual variance), so that the four exceptional branches of the definition
all occur; the restatement's result for a pair, computed once per process and handed out unchanged
(tests/plane_vif_restatement.py); and the comparison."""
import functools
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_vif_restatement as V  # noqa: E402

PLANAR, SEMIPLANAR = K.PLANAR, K.SEMIPLANAR
TILE_W, TILE_H = 32, 32  # the stats kernel's tile of positions (plane_vif_kernel.h: kVifTileW, kVifTileH)

# (w, h, subsampling, depth, the test image's layout, msb_aligned)
SHAPES = [
    (41, 41, V.SUB_400, 8, PLANAR, False),         # one position at scale 4
    (41, 41, V.SUB_420, 8, SEMIPLANAR, False),     # chroma does not run
    (82, 82, V.SUB_420, 8, SEMIPLANAR, False),     # chroma exactly admits
    (81, 83, V.SUB_422, 8, PLANAR, False),
    (42, 57, V.SUB_444, 8, SEMIPLANAR, False),     # even and odd lengths before each decimation
    (131, 99, V.SUB_420, 8, SEMIPLANAR, False),    # several ragged tiles, chroma running
    (41, 600, V.SUB_400, 8, PLANAR, False),        # long and thin
    (600, 41, V.SUB_400, 8, PLANAR, False),
    (131, 99, V.SUB_420, 10, SEMIPLANAR, True),    # the shift
    (131, 99, V.SUB_420, 12, PLANAR, False),       # the clamp's range
    (TILE_W + 17, TILE_H + 17, V.SUB_400, 8, PLANAR, False),  # scale 1 has one position more than a tile each way
    (TILE_W + 16, TILE_H + 16, V.SUB_400, 8, PLANAR, False),  # ... and exactly a tile
]
# rows r0 .. r1 - 1, columns c0 .. c1 - 1: each holds a 17 x 17 window
FLAT, INVERTED, EQUAL = (4, 24, 4, 28), (4, 24, 32, 56), (28, 48, 4, 28)


@functools.lru_cache(maxsize=None)
def planes(w, h, sub, depth, seed=0):
    """-> (ref, test): K.planes with the patches; the flat one is 100 / 255 of L on the reference and 103 / 255 of L on the test"""
    L = (1 << depth) - 1
    ref, test = ([p.copy() for p in side] for side in K.planes(w, h, sub, depth, seed))
    for r, t in zip(ref, test):
        fits = lambda q: r.shape[0] >= q[1] and r.shape[1] >= q[3]  # noqa: E731
        if fits(FLAT):
            r[FLAT[0]:FLAT[1], FLAT[2]:FLAT[3]] = 100 * L // 255
            t[FLAT[0]:FLAT[1], FLAT[2]:FLAT[3]] = 103 * L // 255
        if fits(INVERTED):
            t[INVERTED[0]:INVERTED[1], INVERTED[2]:INVERTED[3]] = L - r[INVERTED[0]:INVERTED[1], INVERTED[2]:INVERTED[3]]
        if fits(EQUAL):
            t[EQUAL[0]:EQUAL[1], EQUAL[2]:EQUAL[3]] = r[EQUAL[0]:EQUAL[1], EQUAL[2]:EQUAL[3]]
        r.setflags(write=False), t.setflags(write=False)
    return tuple(ref), tuple(test)


@functools.lru_cache(maxsize=None)
def expected(w, h, sub, depth, seed=0, ref_seed=None):
    """the restatement on planes(..., seed)'s test against planes(..., ref_seed or seed)'s reference"""
    ref = planes(w, h, sub, depth, seed if ref_seed is None else ref_seed)[0]
    return V.plane_vif(list(ref), list(planes(w, h, sub, depth, seed)[1]), depth, sub)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def check(got, want, where=""):
    """got: a PlaneVifScores (codec_eval_amd), want: the restatement's dict: every integer equal, and every double - a pure f64
    quotient of the integers - bit for bit, NaN where a plane did not run"""
    assert got.n_planes == want["n_planes"] and list(got.ran) == want["ran"], (where, got.n_planes, got.ran)
    for p in range(3):
        for k in ("num_q", "den_q", "n_pos"):
            assert list(getattr(got, k)[p]) == want[k][p], (where, k, p, getattr(got, k)[p], want[k][p])
        assert [bits(v) for v in got.vif_scale[p]] == [bits(v) for v in want["vif_scale"][p]], (where, "vif_scale", p, got.vif_scale[p], want["vif_scale"][p])
        assert bits(got.vifp[p]) == bits(want["vifp"][p]), (where, "vifp", p, got.vifp[p], want["vifp"][p])
