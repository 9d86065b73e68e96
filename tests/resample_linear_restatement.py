"""The float resampler of include/ce_metrics.h (ce_resample_linear) restated in numpy: the separable
convolution Pillow's Image.resize runs on mode "F" images.  Plain and slow on purpose - this is what the device kernels
(codec-eval_amd/csrc/resample_f32.hip) and the host table (ce_tables.cpp: ce_build_resample_table_f64) are compared with, bit
for bit, and what test_resample_linear_cpu.py pins to Pillow itself.

Per axis, `n_in` -> `n_out` samples, filter of support S (weight, SUPPORT: resample_restatement.py):
    scale = n_in / n_out; fs = max(scale, 1); support = S * fs; ss = 1.0 / fs
    output xx: center = (xx + 0.5) * scale
               xmin = max(0, int(center - support + 0.5)); xmax = min(n_in, int(center + support + 0.5))
               w_x = f((x + xmin - center + 0.5) * ss), x in [0, xmax - xmin); divided by their left-to-right f64 sum unless it is 0
               acc = 0.0; acc = acc + float64(sample[xmin + x]) * w_x for x ascending, product and sum each rounded (no fma)
               out = float32(acc)
The reciprocal is Pillow's: with `/ fs` in its place (reciprocal=False) some bilinear downscales differ in their last bits.
The horizontal pass runs first and writes f32; the vertical pass runs on that; a pass whose size does not change is skipped;
the last pass that runs clamps to [-LINEAR_MAX, LINEAR_MAX] (clamp=False: Pillow, which has no such bound); equal sizes
return the input's bits.
"""
import numpy as np

from resample_restatement import BICUBIC, BILINEAR, BOX, CASE_RATIOS, FILTERS, LANCZOS3, SUPPORT, scaled, weight  # noqa: F401

LINEAR_MAX = 1024.0  # CE_LINEAR_MAX


def taps(n_in, n_out, filt, reciprocal=True):
    """[(xmin, [w_0 .. w_{n-1}])] per output sample, the weights as normalised Python floats (f64)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        if reciprocal:
            ws = [weight(filt, (x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        else:
            ws = [weight(filt, (x + xmin - center + 0.5) / fs) for x in range(xmax - xmin)]
        ww = 0.0
        for w in ws:
            ww += w
        if ww != 0.0:
            ws = [w / ww for w in ws]
        out.append((xmin, ws))
    return out


def _pass(img, n_out, filt, reciprocal):
    """Resample axis 0 of an (n_in, ...) float32 array."""
    src = img.astype(np.float64)
    out = np.empty((n_out,) + img.shape[1:], np.float32)
    for xx, (xmin, ws) in enumerate(taps(img.shape[0], n_out, filt, reciprocal)):
        acc = np.zeros(img.shape[1:], np.float64)
        for i, w in enumerate(ws):
            acc = acc + src[xmin + i] * np.float64(w)  # an elementwise product, then an elementwise sum: two roundings
        out[xx] = acc.astype(np.float32)
    return out


def resample(img, out_w, out_h, filt=LANCZOS3, clamp=True, reciprocal=True):
    """(h, w, 3) float32 -> (out_h, out_w, 3) float32."""
    img = np.asarray(img)
    assert img.dtype == np.float32 and img.ndim == 3
    h, w = img.shape[:2]
    if (out_w, out_h) == (w, h):
        return np.ascontiguousarray(img).copy()
    if out_w != w:
        img = np.ascontiguousarray(_pass(np.ascontiguousarray(img.transpose(1, 0, 2)), out_w, filt, reciprocal).transpose(1, 0, 2))
    if out_h != h:
        img = _pass(img, out_h, filt, reciprocal)
    if clamp:
        img = np.clip(img, np.float32(-LINEAR_MAX), np.float32(LINEAR_MAX))
    return np.ascontiguousarray(img, np.float32)


# the issue's cases against Pillow: 5 shapes (w, h) x CASE_RATIOS x the four filters
PILLOW_SHAPES = ((257, 129), (100, 76), (9, 301), (64, 64), (8, 8))


def content(w, h, seed=0, negatives=False):
    """Gaussian noise x 3 with 2 % of the samples set to 125.0 (PQ's 10 000 nits at an 80-nit white); negatives: another 1 %
    set to -60.0, far outside the gamut."""
    rng = np.random.default_rng(4000 + seed + w * 7 + h)
    a = (rng.standard_normal((h, w, 3)) * 3.0).astype(np.float32)
    a[rng.random((h, w, 3)) < 0.02] = np.float32(125.0)
    if negatives:
        a[rng.random((h, w, 3)) < 0.01] = np.float32(-60.0)
    return np.ascontiguousarray(a)
