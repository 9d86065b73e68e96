"""The definition of the alpha compositor (include/ce_metrics.h: ce_batch_set_*_over, ce_composite_rgba*) restated in numpy,
in exact integers at every depth: straight alpha, source-over onto an opaque solid colour, on the encoded sample values,

    out = (c * a + bg * (m - a) + (m >> 1)) // m,    m = 2^d - 1,    c and a clamped to m first.

uint64 holds m * m + (m >> 1) < 2^32 with room to spare, so nothing here can wrap; test_alpha_composite_cpu.py checks it
against Python's own integers and, for m = 255, against Pillow's Image.alpha_composite on all 2^24 (c, a, bg) triples."""
import numpy as np

DEPTHS = (8, 10, 12, 16)


def composite(rgba, bg, depth=8):
    """rgba: (..., 4) unsigned integer samples; bg: three samples <= 2^depth - 1.  Returns (..., 3), uint8 for a uint8
    input and uint16 otherwise."""
    a = np.asarray(rgba)
    assert a.shape[-1] == 4 and a.dtype.kind == "u"
    m = (1 << depth) - 1
    bg = np.asarray(bg, np.uint64)
    assert bg.shape == (3,) and int(bg.max()) <= m
    v = np.minimum(a.astype(np.uint64), np.uint64(m))
    c, al = v[..., :3], v[..., 3:4]
    out = (c * al + bg * (np.uint64(m) - al) + np.uint64(m >> 1)) // np.uint64(m)
    return out.astype(np.uint8 if a.dtype == np.uint8 else np.uint16)


def composite_int(c, a, bg, m):
    """one sample in Python integers"""
    c, a = min(int(c), m), min(int(a), m)
    return (c * a + int(bg) * (m - a) + (m >> 1)) // m


def scale_background(rgb8, depth):
    """an 8-bit background colour at `depth` bits"""
    m = (1 << depth) - 1
    return tuple((int(v) * m + 127) // 255 for v in rgb8)


def random_rgba(rng, w, h, depth=8, dtype=None, over=False):
    """(h, w, 4) samples of `depth` bits with alpha = 0 and alpha = m well represented; over: some u16 samples above m"""
    m = (1 << depth) - 1
    dt = dtype or (np.uint8 if depth == 8 else np.uint16)
    px = rng.integers(0, m + 1, (h, w, 4))
    sel = rng.integers(0, 4, (h, w))
    px[..., 3] = np.where(sel == 0, 0, np.where(sel == 1, m, px[..., 3]))
    if over and np.dtype(dt).itemsize == 2 and depth < 16:
        px = np.where(rng.integers(0, 16, px.shape) == 0, rng.integers(m + 1, 65536, px.shape), px)
    return px.astype(dt)
