"""What the plane-domain tests share (ce_yuv_plane_fidelity): planes for every subsampling, layout, depth,
alignment and pitch - section 27's smooth pattern plus noise of 4 % of L, per plane, seeded - the restatement's result for a
pair, computed once per process and handed out unchanged (tests/plane_fidelity_restatement.py), and the comparison."""
import ctypes as C
import dataclasses
import functools
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_restatement as P  # noqa: E402

PLANAR, SEMIPLANAR = 0, 1
SUBS = (P.SUB_444, P.SUB_422, P.SUB_420, P.SUB_400)
SSE_SHAPES = [(1, 1), (2, 2), (3, 5), (15, 7), (16, 16), (17, 9), (33, 31), (100, 76)]
# (w, h, sub, layout, depth, msb_aligned) of the five-level cases
FIVE_LEVELS = [(161, 161, P.SUB_420, PLANAR, 8, False),      # chroma 81 x 81: one level
               (321, 321, P.SUB_420, PLANAR, 8, False),      # chroma 161 x 161: all three planes run five
               (322, 341, P.SUB_422, SEMIPLANAR, 10, True),
               (192, 256, P.SUB_444, PLANAR, 12, False)]
# the level kernel's 32 x 16 tile: a valid region of 159, 160, 161 = one under, at and one over 5 tiles across and 10 down, on
# luma (4:4:4) and on the chroma planes of a luma of 337, 339, 341 (4:2:0)
TILE_EDGES = [(n, n, P.SUB_444, PLANAR, 8, False) for n in (169, 170, 171)] + [(n, n, P.SUB_420, PLANAR, 8, False) for n in (337, 339, 341)]
assert [P.plane_sizes(n, n, P.SUB_420)[1] for n in (337, 339, 341)] == [(169, 169), (170, 170), (171, 171)]
ONE_LEVEL = [(21, 22, P.SUB_420), (20, 20, P.SUB_420), (12, 11, P.SUB_444), (11, 75, P.SUB_400)]


@functools.lru_cache(maxsize=None)
def planes(w, h, sub, depth, seed=0):
    """-> (ref, test): the planes' samples, [(h_p, w_p)] uint8 at depth 8 and uint16 above.  Read-only."""
    L = (1 << depth) - 1
    rng = np.random.default_rng(1000 * depth + 7 * w + h + 31 * sub + 100003 * seed)
    dt = np.uint8 if depth == 8 else np.uint16
    ref, test = [], []
    for c, (pw, ph) in enumerate(P.plane_sizes(w, h, sub)):
        yy, xx = np.mgrid[0:ph, 0:pw].astype(np.float64)
        smooth = 0.5 + 0.35 * np.sin(xx / (9.0 + 3 * c) + rng.random() * 6.0) * np.cos(yy / (7.0 + 2 * c)) + 0.1 * np.sin((xx + yy) / 31.0)
        r = np.clip(np.rint(smooth * L), 0, L).astype(dt)
        t = np.clip(np.rint(smooth * L + (rng.random(smooth.shape) * 2.0 - 1.0) * 0.04 * L), 0, L).astype(dt)
        r.setflags(write=False), t.setflags(write=False)
        ref.append(r), test.append(t)
    return tuple(ref), tuple(test)


@functools.lru_cache(maxsize=None)
def expected(w, h, sub, depth, levels=5, seed=0, ref_seed=None):
    """the restatement on planes(..., seed)'s test against planes(..., ref_seed or seed)'s reference"""
    ref = planes(w, h, sub, depth, seed if ref_seed is None else ref_seed)[0]
    return P.plane_fidelity(list(ref), list(planes(w, h, sub, depth, seed)[1]), depth, sub, levels)


def stored(samples, depth, msb_aligned):
    """samples -> the values a decoder stores: in the top bits of the u16 when MSB-aligned"""
    return [(np.asarray(p).astype(np.uint16) << (16 - depth)) if msb_aligned else np.asarray(p) for p in samples]


def interleave(cb, cr):
    out = np.empty((cb.shape[0], 2 * cb.shape[1]), cb.dtype)
    out[:, 0::2], out[:, 1::2] = cb, cr
    return out


def padded(plane, pad, rng):
    """the plane's bytes as rows of a wider buffer whose padding holds junk: a (rows, row bytes) uint8 view, pitch = + pad"""
    raw = np.ascontiguousarray(plane).view(np.uint8).reshape(plane.shape[0], -1)
    if pad == 0:
        return raw
    buf = rng.integers(0, 256, (raw.shape[0], raw.shape[1] + pad), dtype=np.uint8)
    buf[:, :raw.shape[1]] = raw
    return buf[:, :raw.shape[1]]


def host_planes(samples, sub, depth, layout=PLANAR, msb_aligned=False, pad=0, seed=0):
    """samples -> the planes as the layout stores them, [(rows, row bytes) uint8 views whose row stride is the pitch]"""
    rng = np.random.default_rng(seed)
    s = stored(samples, depth, msb_aligned)
    if sub == P.SUB_400:
        return [padded(s[0], pad, rng)]
    if layout == SEMIPLANAR:
        return [padded(s[0], pad, rng), padded(interleave(s[1], s[2]), pad, rng)]
    return [padded(p, pad, rng) for p in s]


def pitch_of(p):
    return p.strides[0] if p.shape[0] > 1 else p.shape[1]


def image(ce, samples, sub, depth, layout=PLANAR, msb_aligned=False, pad=0, **kw):
    """samples -> a YuvImage on the host"""
    pl = host_planes(samples, sub, depth, layout, msb_aligned, pad)
    return ce.YuvImage(pl, subsampling=sub, layout=layout, depth=depth, msb_aligned=msb_aligned, pitches=[pitch_of(p) for p in pl], **kw)


class HipBuffer:
    """device memory from the HIP runtime the library itself is linked against (no second runtime in the process), freed
    with the object"""
    def __init__(self, lib, data):
        self.lib, self.ptr, self.nbytes = lib, C.c_void_p(), data.nbytes
        assert lib.hipMalloc(C.byref(self.ptr), C.c_size_t(max(data.nbytes, 1))) == 0 and self.ptr.value % 256 == 0
        assert lib.hipMemcpy(self.ptr, C.c_void_p(data.ctypes.data), C.c_size_t(data.nbytes), 1) == 0

    def read(self):
        out = np.empty(self.nbytes, np.uint8)
        assert self.lib.hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(self.nbytes), 2) == 0
        return out

    def __del__(self):
        self.lib.hipFree(self.ptr)


def on_device(ce, img, offset=0):
    """the same planes in device memory, `offset` bytes into their 256-byte aligned allocations, passed by address, junk in
    the pitch padding; returns (YuvImage, the buffers to keep)"""
    keep, ptrs, pitches = [], [], []
    for p in img.planes:
        pitch = pitch_of(p)
        full = np.full(offset + p.shape[0] * pitch, 0xA5, np.uint8)
        rows = full[offset:].reshape(p.shape[0], pitch)
        rows[:, :p.shape[1]] = p
        buf = HipBuffer(ce.lib(), full)
        keep.append(buf)
        ptrs.append(buf.ptr.value + offset)
        pitches.append(pitch)
    dev = ce.YuvImage(ptrs, img.subsampling, img.layout, img.matrix, img.range, img.upsample, img.depth, img.msb_aligned, ce.MEM_DEVICE, pitches)
    return dev, keep


def checkerboard(w, h, sub, cell=3, L=255, dtype=np.uint8):
    """per plane a `cell`-sample checkerboard of 0 and L, and its inverse"""
    a, b = [], []
    for pw, ph in P.plane_sizes(w, h, sub):
        yy, xx = np.mgrid[0:ph, 0:pw]
        v = ((((yy // cell) + (xx // cell)) & 1) * L).astype(dtype)
        a.append(v), b.append((L - v).astype(dtype))
    return a, b


def key(scores):
    """a PlaneScores, or a list of them, with every double as its bit pattern: NaN fields compare equal"""
    if isinstance(scores, list):
        return [key(s) for s in scores]
    bits = lambda v: struct.unpack("<Q", struct.pack("<d", v))[0] if isinstance(v, float) else tuple(bits(x) for x in v) if isinstance(v, tuple) else v  # noqa: E731
    return tuple(bits(v) for v in dataclasses.astuple(scores))


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= 1e-14 * abs(b)


def check_integers(got, want, where=""):
    """got: a PlaneScores (codec_eval_amd), want: the restatement's dict: every integer equal, the doubles within 1e-14 relative
    (libm's log10 and pow are the unpinned operations), NaN matching NaN and infinity infinity"""
    assert got.n_planes == want["n_planes"] and list(got.n_levels) == want["n_levels"], (where, got.n_planes, got.n_levels)
    assert list(got.sse) == want["sse"] and list(got.n) == want["n"], (where, "sse", got.sse, want["sse"], got.n, want["n"])
    for p in range(3):
        assert list(got.ssim_q[p]) == want["ssim_q"][p], (where, "ssim_q", p, got.ssim_q[p], want["ssim_q"][p])
        assert list(got.cs_q[p]) == want["cs_q"][p], (where, "cs_q", p, got.cs_q[p], want["cs_q"][p])
        assert list(got.n_pos[p]) == want["n_pos"][p], (where, "n_pos", p)
        for k in ("psnr", "ssim", "ms_ssim"):
            assert same(getattr(got, k)[p], want[k][p]), (where, k, p, getattr(got, k)[p], want[k][p])
    assert same(got.psnr_weighted, want["psnr_weighted"]) and same(got.psnr_overall, want["psnr_overall"]), (where, got, want)
