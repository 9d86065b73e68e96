"""The Y'CbCr ingest definition of include/ce_metrics.h restated in numpy: the chroma upsampling
of libjpeg-turbo's decoder (h2v2 / h2v1 "fancy" triangle filters, or replication), then jdcolor.c's fixed-point colour
conversion with the coefficients generalised to other matrices, ranges and depths.  Everything after the coefficients
is int64.  The tests compare the device with this, and this with libjpeg-turbo through tests/golden/yuv_pillow.npz."""
import numpy as np

SUB_444, SUB_422, SUB_420, SUB_400 = 0, 1, 2, 3
PLANAR, SEMIPLANAR = 0, 1
BT601, BT709, BT2020 = 0, 1, 2
FULL, LIMITED = 0, 1
NEAREST, TRIANGLE = 0, 1


def matrix_constants(matrix):
    """a (Cr -> R), b (Cb -> G), c (Cr -> G), e (Cb -> B)"""
    if matrix == BT601:
        return 1.40200, 0.34414, 0.71414, 1.77200  # libjpeg's literals
    kr, kb = {BT709: (0.2126, 0.0722), BT2020: (0.2627, 0.0593)}[matrix]
    kg = 1.0 - kr - kb
    a, e = 2.0 * (1.0 - kr), 2.0 * (1.0 - kb)
    return a, kb * e / kg, kr * a / kg, e


def range_constants(range_, d, D):
    """y0, c0, sy, sc"""
    m, u = float((1 << D) - 1), float(1 << (d - 8))
    if range_ == FULL:
        s = m / float((1 << d) - 1)
        return 0, 1 << (d - 1), s, s
    return 16 << (d - 8), 128 << (d - 8), m / (219.0 * u), m / (224.0 * u)


def coefficients(matrix, range_, d, D):
    """(KY, KRV, KGU, KGV, KBU, y0, c0): f64 products rounded once"""
    a, b, c, e = matrix_constants(matrix)
    y0, c0, sy, sc = range_constants(range_, d, D)
    return (int(np.rint(sy * 65536.0)), int(np.rint(sc * a * 65536.0)), int(np.rint(sc * b * 65536.0)),
            int(np.rint(sc * c * 65536.0)), int(np.rint(sc * e * 65536.0)), y0, c0)


def chroma_size(w, h, sub):
    """(cw, ch) of a chroma plane"""
    return (w if sub == SUB_444 else (w + 1) // 2), ((h + 1) // 2 if sub == SUB_420 else h)


def samples(plane, d, msb_aligned=False):
    """a plane's values: MSB-aligned u16 shifted down, low-aligned values clamped to 2^d - 1"""
    v = np.asarray(plane).astype(np.int64)
    if msb_aligned:
        v = v >> (16 - d)
    return np.minimum(v, (1 << d) - 1)


def _triangle_h(t, add_even, add_odd, shift):
    left = np.concatenate([t[:, :1], t[:, :-1]], axis=1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int64)
    out[:, 0::2] = (3 * t + left + add_even) >> shift
    out[:, 1::2] = (3 * t + right + add_odd) >> shift
    return out


def upsample(c, sub, mode, w, h):
    """one chroma plane (ch, cw) of int64 values -> (h, w)"""
    c = np.asarray(c, np.int64)
    if sub == SUB_444:
        return c[:h, :w]
    if mode == NEAREST:
        full = np.repeat(c, 2, axis=1)
        if sub == SUB_420:
            full = np.repeat(full, 2, axis=0)
    elif sub == SUB_422:
        full = _triangle_h(c, 1, 2, 2)
    else:
        above = np.concatenate([c[:1], c[:-1]], axis=0)
        below = np.concatenate([c[1:], c[-1:]], axis=0)
        t = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
        t[0::2] = 3 * c + above
        t[1::2] = 3 * c + below
        full = _triangle_h(t, 8, 7, 4)
    return full[:h, :w]


def convert(y, cb, cr, k, D):
    """full-resolution int64 planes -> (h, w, 3) of depth D"""
    ky, krv, kgu, kgv, kbu, y0, c0 = k
    m = (1 << D) - 1
    yy = ky * (y - y0) + (1 << 15)
    u, v = cb - c0, cr - c0
    r = (yy + krv * v) >> 16
    g = (yy - kgu * u - kgv * v) >> 16
    b = (yy + kbu * u) >> 16
    return np.clip(np.stack([r, g, b], -1), 0, m).astype(np.uint8 if D == 8 else np.uint16)


def yuv_to_rgb(y, cb, cr, w, h, sub, matrix=BT601, range_=FULL, mode=TRIANGLE, d=8, D=8, msb_aligned=False):
    """planes as a decoder hands them over (2-D arrays; cb / cr ignored for 4:0:0) -> (h, w, 3) u8 (D = 8) or u16"""
    k = coefficients(matrix, range_, d, D)
    yv = samples(y, d, msb_aligned)[:h, :w]
    if sub == SUB_400:
        c = np.full((h, w), k[6], np.int64)
        return convert(yv, c, c, k, D)
    cbf = upsample(samples(cb, d, msb_aligned), sub, mode, w, h)
    crf = upsample(samples(cr, d, msb_aligned), sub, mode, w, h)
    return convert(yv, cbf, crf, k, D)


def convert_f64(y, cb, cr, matrix, range_, d=8, D=8):
    """round-half-up of the f64 definition the fixed point approximates (full-resolution planes)"""
    a, b, c, e = matrix_constants(matrix)
    y0, c0, sy, sc = range_constants(range_, d, D)
    m = (1 << D) - 1
    yy = sy * (np.asarray(y, np.float64) - y0)
    u, v = sc * (np.asarray(cb, np.float64) - c0), sc * (np.asarray(cr, np.float64) - c0)
    rgb = np.stack([yy + a * v, yy - b * u - c * v, yy + e * u], -1)
    return np.clip(np.floor(rgb + 0.5), 0, m).astype(np.int64)


def interleave(cb, cr):
    """planar Cb, Cr -> the CbCr plane of the semiplanar layouts (NV12 / NV16 / P010)"""
    return np.ascontiguousarray(np.stack([cb, cr], -1).reshape(cb.shape[0], -1))


def random_planes(rng, w, h, sub, d=8, msb_aligned=False, over=False):
    """random planes of depth d (over: some low-aligned values above 2^d - 1, which ingest clamps)"""
    cw, ch = chroma_size(w, h, sub)
    dt = np.uint8 if d == 8 else np.uint16
    hi = (1 << d) + (64 if over and d > 8 and not msb_aligned else 0)

    def one(r, c):
        v = rng.integers(0, hi, (r, c)).astype(dt)
        return (v << (16 - d)).astype(dt) if msb_aligned else v
    return one(h, w), one(ch, cw), one(ch, cw)


def smooth_planes(rng, w, h, sub, d=8):
    """a gradient with noise: neighbouring samples differ a little, as a photograph's do"""
    cw, ch = chroma_size(w, h, sub)
    m = (1 << d) - 1

    def one(r, c, fx, fy):
        yy, xx = np.mgrid[0:r, 0:c]
        v = m * (0.5 + 0.5 * np.sin(fx * xx / max(c, 1) + fy * yy / max(r, 1))) + rng.normal(0, m / 40.0, (r, c))
        return np.clip(np.rint(v), 0, m).astype(np.uint8 if d == 8 else np.uint16)
    return one(h, w, 5.0, 3.0), one(ch, cw, 2.0, 4.0), one(ch, cw, 3.0, 1.5)
