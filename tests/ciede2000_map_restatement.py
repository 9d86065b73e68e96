"""The CIEDE2000 maps (include/ce_metrics.h: ce_batch_ciede2000_map, ce_eval_pair_ciede2000_map{,_deep}, ce_ciede2000_pixel_terms;
DESIGN.md section 34) restated in numpy.  terms_of_lab states the whole pixel itself - every f64 operation of
tests/ciede2000_restatement.py's delta_e, in its order and with its parentheses, on that file's elementary sequences - up to the
lightness, chroma and hue terms tl, tc, th and the rotation factor R_T, and forms the four values a map can hold: q = rint(dE
2^20), which tests/test_ciede2000_map_cpu.py holds to ciede2000_restatement.q20 with ==, and rint(|term| 2^20) of the three
terms.  Then the maxima of B x B cells with the edge cells clipped to the image, and how many pixels exceed a threshold.  A
helper, not a test."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_cases as K  # noqa: E402
import ciede2000_restatement as R  # noqa: E402

DE, DL, DC, DH = 0, 1, 2, 3  # CE_CIEDE2000_MAP_DE, _DL, _DC, _DH
WHATS = (DE, DL, DC, DH)
NAMES = ("de", "dl", "dc", "dh")
BLOCKS = (2, 4, 8, 16, 32, 64)
F = np.float64


def _q(x):
    """rint(x 2^20) of a non-negative f64 array as uint32."""
    return np.rint(x * 1048576.0).astype(np.uint64).astype(np.uint32)


def terms_of_lab(l1, a1, b1, l2, a2, b2):
    """Lab arrays (f64) of the reference (1) and the test (2) -> uint32 [..., 4]: DE, DL, DC, DH."""
    hue, sc, ex = R.hue_deg, R.sincos_deg, R.exp_fixed
    l1, a1, b1, l2, a2, b2 = [np.asarray(v, F) for v in (l1, a1, b1, l2, a2, b2)]
    c1 = np.sqrt(a1 * a1 + b1 * b1)
    c2 = np.sqrt(a2 * a2 + b2 * b2)
    cb = 0.5 * (c1 + c2)
    cb7 = R.pow7(cb)
    g = 0.5 * (1.0 - np.sqrt(cb7 / (cb7 + R.POW25_7)))
    ap1 = (1.0 + g) * a1
    ap2 = (1.0 + g) * a2
    cp1 = np.sqrt(ap1 * ap1 + b1 * b1)
    cp2 = np.sqrt(ap2 * ap2 + b2 * b2)
    h1 = hue(b1, ap1)
    h2 = hue(b2, ap2)
    dl = l2 - l1
    dc = cp2 - cp1
    cc = cp1 * cp2
    nz = cc != 0.0
    dh = h2 - h1
    dh = np.where(dh > 180.0, dh - 360.0, np.where(dh < -180.0, dh + 360.0, dh))
    dh = np.where(nz, dh, 0.0)
    dH = (2.0 * np.sqrt(cc)) * sc(0.5 * dh)[0]
    hs = h1 + h2
    hb = np.where(~nz, hs, np.where(np.abs(h1 - h2) <= 180.0, 0.5 * hs, np.where(hs < 360.0, 0.5 * (hs + 360.0), 0.5 * (hs - 360.0))))
    lb = 0.5 * (l1 + l2)
    cpb = 0.5 * (cp1 + cp2)
    t = (((1.0 - 0.17 * sc(hb - 30.0)[1]) + 0.24 * sc(2.0 * hb)[1]) + 0.32 * sc(3.0 * hb + 6.0)[1]) - 0.20 * sc(4.0 * hb - 63.0)[1]
    z = (hb - 275.0) / 25.0
    dth = 30.0 * ex(-(z * z))
    cpb7 = R.pow7(cpb)
    rc = 2.0 * np.sqrt(cpb7 / (cpb7 + R.POW25_7))
    l50 = lb - 50.0
    l50 = l50 * l50
    sl = 1.0 + (0.015 * l50) / np.sqrt(20.0 + l50)
    s_c = 1.0 + 0.045 * cpb
    sh = 1.0 + (0.015 * cpb) * t
    rt = (-sc(2.0 * dth)[0]) * rc
    tl, tc, th = dl / sl, dc / s_c, dH / sh
    s = ((tl * tl + tc * tc) + th * th) + rt * (tc * th)
    de = np.sqrt(np.maximum(s, 0.0))
    # |x| clears the sign bit: np.abs of a float does, and -0 gives 0
    return np.stack([_q(de), _q(np.abs(tl)), _q(np.abs(tc)), _q(np.abs(th))], axis=-1)


def terms(ref, ref_depth, ref_table, test, test_depth, test_table):
    """[..., 3] integer samples a side -> uint32 [..., 4]: the four values of every pixel."""
    return terms_of_lab(*R.lab(ref, ref_depth, ref_table), *R.lab(test, test_depth, test_table))


def block_max(m, block: int) -> np.ndarray:
    """uint32 [h, w] -> the maximum of every block x block cell, [ceil(h / block), ceil(w / block)]: the map padded to whole
    cells with zeros, which no maximum of unsigned values notices, and folded."""
    m = np.asarray(m)
    h, w = m.shape
    ch, cw = -(-h // block), -(-w // block)
    padded = np.zeros((ch * block, cw * block), m.dtype)
    padded[:h, :w] = m
    return padded.reshape(ch, block, cw, block).max(axis=(1, 3))


def over(m, thresholds) -> np.ndarray:
    """uint64 [n]: the pixels of the full map above each threshold."""
    m = np.asarray(m).astype(np.int64)
    return np.array([int((m > int(t)).sum()) for t in thresholds], np.uint64)


def terms_of_images(ref, test, kind):
    """One pair of [h, w, 3] images of ciede2000_cases' `kind` -> uint32 [h, w, 4], through the distinct (reference, test) colour
    pairs of the images, as ciede2000_cases.q_of; ciede2000_cases.use(ce) first."""
    dr, dt = (8, 8) if kind == (0, 0) else kind
    both = np.concatenate([ref.reshape(-1, 3), test.reshape(-1, 3)], axis=1).astype(np.int64)
    uniq, inverse = np.unique(both, axis=0, return_inverse=True)
    v = terms(uniq[:, :3], dr, K.TABLES[dr], uniq[:, 3:], dt, K.TABLES[dt])
    return v[inverse.reshape(-1)].reshape(ref.shape[0], ref.shape[1], 4)


@functools.lru_cache(maxsize=None)
def expected(w, h, kind):
    """The restated values of the five pairs of ciede2000_cases.images(w, h, kind): uint32 [5, h, w, 4], computed once and
    shared.  Read-only."""
    refs, tests = K.images(w, h, kind)
    out = np.stack([terms_of_images(refs[K.BINDING[p]], tests[p], kind) for p in range(5)])
    out.setflags(write=False)
    return out
