"""The resampler of include/ce_metrics.h (enum ce_resample_filter) restated in numpy: the separable
fixed-point convolution Pillow's Image.resize runs on 8-bit images.  Plain and slow on purpose - this is what the device
kernels (codec-eval_amd/csrc/resample.hip) and the host tables (ce_tables.cpp) are compared with, byte for byte.

Per axis, `n_in` -> `n_out` samples, filter of support S:
    scale = n_in / n_out; fs = max(scale, 1); support = S * fs
    output xx: center = (xx + 0.5) * scale
               xmin = max(0, int(center - support + 0.5)); xmax = min(n_in, int(center + support + 0.5))
               w_x = f((x + xmin - center + 0.5) / fs), x in [0, xmax - xmin), divided by their left-to-right f64 sum
               k_x = int(0.5 + w_x * 2^22)  (int(-0.5 + ...) for a negative weight)
               out = clip_0_255((2^21 + sum k_x * sample[xmin + x]) >> 22), int32 accumulator, arithmetic shift
The horizontal pass runs first and writes u8; the vertical pass runs on that; a pass whose size does not change is skipped.
"""
import math

import numpy as np

BOX, BILINEAR, BICUBIC, LANCZOS3 = 0, 1, 2, 3
FILTERS = (BOX, BILINEAR, BICUBIC, LANCZOS3)
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0, LANCZOS3: 3.0}
PRECISION_BITS = 22


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def weight(filt, x):
    if filt == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if filt == BILINEAR:
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if filt == BICUBIC:
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if filt == LANCZOS3:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(f"unknown filter {filt}")


def taps(n_in, n_out, filt):
    """[(xmin, [k_0 .. k_{n-1}])] per output sample, the weights as 22-bit integers."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        ws = [weight(filt, (x + xmin - center + 0.5) / fs) for x in range(xmax - xmin)]
        ww = 0.0
        for w in ws:
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        ks = [int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS)) for w in ws]
        out.append((xmin, ks))
    return out


def _pass(img, n_out, filt, max_acc):
    """Resample axis 0 of an (n_in, ...) uint8 array."""
    n_in = img.shape[0]
    src = img.astype(np.int64)
    out = np.empty((n_out,) + img.shape[1:], np.uint8)
    for xx, (xmin, ks) in enumerate(taps(n_in, n_out, filt)):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for i, k in enumerate(ks):
            acc += k * src[xmin + i]
            if max_acc is not None:
                max_acc[0] = max(max_acc[0], int(np.abs(acc).max(initial=0)))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resample(img, out_w, out_h, filt=LANCZOS3, max_acc=None):
    """(h, w, 3) uint8 -> (out_h, out_w, 3) uint8.  max_acc: a one-element list that collects the largest |accumulator|."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    h, w = img.shape[:2]
    if out_w != w:
        img = np.ascontiguousarray(_pass(np.ascontiguousarray(img.transpose(1, 0, 2)), out_w, filt, max_acc).transpose(1, 0, 2))
    if out_h != h:
        img = _pass(img, out_h, filt, max_acc)
    return np.ascontiguousarray(img)


# the issue's cases: shapes (w, h) x ratios; a ratio r turns n into max(1, round-half-away(n * r))
CASE_SHAPES = ((768, 512), (257, 129), (100, 76), (9, 301), (64, 64), (8, 8))
CASE_RATIOS = ((1, 3), (1, 2), (2, 3), (3, 4), (1, 1), (3, 2), (2, 1), (3, 1))


def scaled(n, num, den):
    return max(1, (2 * n * num + den) // (2 * den))


def content(w, h, kind, seed=0):
    """'noise': uniform random bytes; 'pattern': gradients, a checkerboard and hard 0/255 edges."""
    if kind == "noise":
        return np.random.default_rng(1000 + seed + w * 7 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    r = (x * 255 // max(w - 1, 1)).astype(np.uint8)
    g = (((x // 3 + y // 2) & 1) * 255).astype(np.uint8)
    b = np.where((x > w // 2) ^ (y > h // 3), 255, 0).astype(np.uint8)
    return np.ascontiguousarray(np.stack([r, g, b], axis=2))
