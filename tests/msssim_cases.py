"""What the SSIM / MS-SSIM tests share: the content (a smooth pattern plus noise of 4 % of L), the shapes, and the restatement's
result for a pair, computed once per process and handed out unchanged (tests/msssim_restatement.py)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_restatement as M  # noqa: E402

TILE_W, TILE_H = 32, 16  # the level kernel's output tile (msssim_kernel.h: kMssTileW, kMssTileH)

# (w, h, depth) of the five-level cases; depth 8 is scored in an RGB8 batch
SHAPES_8 = [(161, 161), (176, 163), (163, 176), (161, 200)]
DEEP = [(192, 256, 10), (192, 256, 12), (192, 256, 16)]
# level 0's valid region (w - 10) x (h - 10) one under, at and one over a multiple of the tile, both ways: 159 = 5 * 32 - 1 = 10 * 16 - 1
TILE_EDGES = [(169, 169), (170, 170), (171, 171)]
assert all((w - 10 - d) % TILE_W == 0 and (h - 10 - d) % TILE_H == 0 for d, (w, h) in zip((-1, 0, 1), TILE_EDGES))
ONE_LEVEL = [(11, 11), (12, 11), (11, 75)]


@functools.lru_cache(maxsize=None)
def pair(w, h, depth, seed=0):
    """-> (ref, test), (h, w, 3) uint8 at depth 8 and uint16 above: a smooth pattern, and the same with noise of 4 % of L
    (uniform in +-4 % of L), clipped to [0, L].  Read-only."""
    L = (1 << depth) - 1
    rng = np.random.default_rng(1000 * depth + 7 * w + h + 100003 * seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.random(3) * 6.0
    smooth = np.stack([0.5 + 0.35 * np.sin(xx / (9.0 + 3 * c) + ph[c]) * np.cos(yy / (7.0 + 2 * c)) + 0.1 * np.sin((xx + yy) / 31.0)
                       for c in range(3)], axis=-1)
    dt = np.uint8 if depth == 8 else np.uint16
    ref = np.clip(np.rint(smooth * L), 0, L).astype(dt)
    test = np.clip(np.rint(smooth * L + (rng.random(smooth.shape) * 2.0 - 1.0) * 0.04 * L), 0, L).astype(dt)
    ref.setflags(write=False), test.setflags(write=False)
    return ref, test


@functools.lru_cache(maxsize=None)
def expected(w, h, depth, levels=5, seed=0, ref_seed=None):
    """the restatement on pair(w, h, depth, seed)'s test against pair(w, h, depth, ref_seed or seed)'s reference"""
    ref = pair(w, h, depth, seed if ref_seed is None else ref_seed)[0]
    return M.msssim(ref, pair(w, h, depth, seed)[1], depth, levels)


def checkerboard(w, h, cell=3, L=255, dtype=np.uint8):
    """a `cell`-pixel checkerboard of 0 and L on all channels, and its inverse"""
    yy, xx = np.mgrid[0:h, 0:w]
    a = (((yy // cell) + (xx // cell)) & 1) * L
    a = np.repeat(a[:, :, None], 3, axis=2)
    return a.astype(dtype), (L - a).astype(dtype)


def check_integers(got, want, where=""):
    """got: an MsSsim (codec_eval_amd), want: the restatement's dict: every integer equal, the doubles within 1e-14 relative
    (only libm's pow may differ)"""
    lv = want["n_levels"]
    assert got.n_levels == lv, where
    for l in range(5):
        assert list(got.ssim_q[l]) == want["ssim_q"][l], (where, "ssim_q", l, got.ssim_q[l], want["ssim_q"][l])
        assert list(got.cs_q[l]) == want["cs_q"][l], (where, "cs_q", l, got.cs_q[l], want["cs_q"][l])
        assert got.n[l] == want["n"][l], (where, "n", l)
    close = lambda a, b: (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-14 * abs(b)  # noqa: E731
    assert close(got.ssim, want["ssim"]) and close(got.ms_ssim, want["ms_ssim"]), (where, got.ssim, want["ssim"], got.ms_ssim, want["ms_ssim"])
    for c in range(3):
        assert close(got.ssim_rgb[c], want["ssim_rgb"][c]) and close(got.ms_ssim_rgb[c], want["ms_ssim_rgb"][c]), (where, c)
