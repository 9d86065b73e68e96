"""The batches the CIEDE2000 tests score (tests/test_ciede2000_kernel_host_cpu.py on the host build of the kernel,
tests/test_gpu_ciede2000.py on the device): per shape and kind of batch two references and five tests bound through a pair
table that is no identity, with the launcher's geometry restated so that the tests can say which path a shape takes and
whether its grid-stride loop goes round.  Content: anchor pairs in turn - black and white, greys, primaries against their
complements and hue pairs chosen so that every branch of the hue difference and of the mean hue runs - then noise; an image
against itself; noise of +-3 codes; unrelated noise.  A helper, not a test."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_restatement as R  # noqa: E402

DEPTHS = (8, 10, 12, 16)
# what a batch holds: (0, 0) an RGB8 batch (uint8 slabs, read at depth 8), else a deep batch's (reference depth, test depth)
KINDS = [(0, 0), (10, 10), (12, 12), (16, 16), (8, 16)]
SHAPES = [(1, 1), (3, 1), (4, 1), (5, 3), (16, 8), (333, 251)]
# 512 x 520 pixels with 16 pairs: a pair gets 64 blocks, whose lanes hold 262144 pixels of an RGB8 image and 131072 of a deep one
BIG, BIG_PAIRS = (512, 520), 16
BINDING = [1, 0, 0, 1, 0]  # pair -> reference slot
THRESHOLDS = [0, 1, 1 << 20, 2 << 20, 5 << 20, 50 << 20, 100 << 20, (1 << 32) - 1]

TABLES = {}


def use(ce):
    """The library's sRGB tables (ce_srgb_table(depth, 0)): what the restatement reads the samples through."""
    for d in DEPTHS:
        if d not in TABLES:
            TABLES[d] = ce.srgb_table(d, 0)


# the launcher's geometry (codec-eval_amd/csrc/ciede2000_kernel.h: cie_unit, cie_wide, cie_blocks)
THREADS = 256


def unit(deep):
    return 8 if deep else 16


def wide(n_pixels, deep):
    return n_pixels % unit(deep) == 0


def blocks(n_pixels, n_pairs, deep):
    work = n_pixels // unit(deep) if wide(n_pixels, deep) else n_pixels
    want, cap = (work + THREADS - 1) // THREADS, max(1024 // n_pairs, 64)
    return max(min(want, cap), 1)


def goes_round(n_pixels, n_pairs, deep):
    """More units of work than the launch has lanes: the grid-stride loop takes a second turn."""
    per_lane = unit(deep) if wide(n_pixels, deep) else 1
    return n_pixels > blocks(n_pixels, n_pairs, deep) * THREADS * per_lane


W, K0 = (255, 255, 255), (0, 0, 0)
RED, GREEN, BLUE, CYAN, MAGENTA, YELLOW = (255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0)
# (reference, test) in 8-bit terms
ANCHORS = [(K0, W), (W, K0), (K0, K0), (W, W), (K0, RED), (BLUE, K0), (W, (254, 255, 255)),
           ((128, 128, 128), (129, 128, 128)), ((17, 17, 17), (200, 200, 200)), ((64, 64, 64), (64, 64, 63)), ((1, 1, 1), (2, 2, 2)),
           (RED, CYAN), (GREEN, MAGENTA), (BLUE, YELLOW), (CYAN, RED), (MAGENTA, GREEN), (YELLOW, BLUE),
           ((255, 0, 100), (0, 200, 255)), ((0, 200, 255), (255, 0, 100)), ((255, 0, 40), (0, 140, 255)), ((0, 140, 255), (255, 0, 40)),
           ((255, 10, 0), (255, 0, 60)), ((255, 0, 60), (255, 10, 0)), ((10, 3, 2), (9, 3, 3)), ((3, 2, 1), (2, 2, 2))]


def to_depth(v8, depth):
    """8-bit terms -> the nearest code of `depth` bits (257 v at 16 bits)."""
    maxv = (1 << depth) - 1
    return (np.asarray(v8, np.int64) * maxv + 127) // 255


@functools.lru_cache(maxsize=None)
def images(w, h, kind):
    """-> (refs, tests): two reference and five test images [h, w, 3], uint8 for the RGB8 kind and else uint16 at the kind's
    depths.  Pair p is tests[p] against refs[BINDING[p]]:
      0 against noise: the noise moved by up to +-3 codes;   1 against the anchors' reference colours: their test colours;
      2 against the anchors image: itself (at 8 / 16, 257 v for v);   3 against noise: other noise;
      4 against the anchors image: its greys and near-greys tinted by one code."""
    dr, dt = (8, 8) if kind == (0, 0) else kind
    n = w * h
    rng = np.random.default_rng(1000 * w + h + dr + dt)
    a = np.array(ANCHORS, np.int64)  # [k, 2, 3]
    idx = np.arange(n) % len(a)
    tail = np.arange(n) >= 4 * len(a)  # beyond four rounds of anchors: noise with its own test colours
    base_r, base_t = a[idx, 0], a[idx, 1]
    fill = min(n, 4096)  # few distinct pairs, so that restating a large image stays cheap
    nr, nt = rng.integers(0, 256, (fill, 3)), rng.integers(0, 256, (fill, 3))
    pick = rng.integers(0, fill, n)
    base_r = np.where(tail[:, None], nr[pick], base_r)
    base_t = np.where(tail[:, None], nt[pick], base_t)
    ref0, t1 = to_depth(base_r, dr), to_depth(base_t, dt)
    t2 = to_depth(base_r, dt)
    maxr, maxt = (1 << dr) - 1, (1 << dt) - 1
    noise_r = rng.integers(0, maxr + 1, (fill, 3))[pick]
    ref1 = noise_r
    t0 = np.clip(noise_r * maxt // maxr + rng.integers(-3, 4, (fill, 3))[rng.integers(0, fill, n)], 0, maxt)
    t3 = rng.integers(0, maxt + 1, (fill, 3))[pick[::-1]]
    t4 = np.clip(to_depth(base_r, dt) + np.array([1, 0, -1]) * (idx[:, None] % 3 - 1), 0, maxt)
    dtype = np.uint8 if kind == (0, 0) else np.uint16
    shape = lambda x: np.ascontiguousarray(x.reshape(h, w, 3).astype(dtype))  # noqa: E731
    return [shape(ref0), shape(ref1)], [shape(t0), shape(t1), shape(t2), shape(t3), shape(t4)]


def q_of(ref, test, kind):
    """The pixels' q of one pair by the restatement, through the distinct (reference, test) colour pairs of the images."""
    dr, dt = (8, 8) if kind == (0, 0) else kind
    both = np.concatenate([ref.reshape(-1, 3), test.reshape(-1, 3)], axis=1).astype(np.int64)
    uniq, inverse = np.unique(both, axis=0, return_inverse=True)
    q = R.q20(uniq[:, :3], dr, TABLES[dr], uniq[:, 3:], dt, TABLES[dt])
    return q[inverse.reshape(-1)]


@functools.lru_cache(maxsize=None)
def pair_q(w, h, kind, p):
    refs, tests = images(w, h, kind)
    return q_of(refs[BINDING[p]], tests[p], kind)


@functools.lru_cache(maxsize=None)
def expected(w, h, kind, with_thresholds=True):
    """-> the five pairs' scores (R.scores) with THRESHOLDS or with none; use(ce) first."""
    return [R.scores(pair_q(w, h, kind, p), THRESHOLDS if with_thresholds else ()) for p in range(5)]


def check(got, want, what):
    """A Ciede2000 of the binding against R.scores' dict: integers with ==, doubles within 1e-14 relative."""
    assert (got.sum_q20, got.max_q20, got.n, list(got.n_above)) == (want["sum_q20"], want["max_q20"], want["n"], want["n_above"]), what
    for name in ("mean", "max", "ciede2000_db"):
        g, w_ = getattr(got, name), want[name]
        assert g == w_ or abs(g - w_) <= 1e-14 * abs(w_), (what, name, g, w_)
