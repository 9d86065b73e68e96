"""CIEDE2000 of two integer RGB images as include/ce_metrics.h defines ce_batch_ciede2000, restated in numpy operation by
operation: every f64 addition, subtraction, product, quotient, square root and rint below is one separately rounded IEEE
operation, in the order and with the parentheses of codec-eval_amd/csrc/ciede2000_pixel.h, so the device, the host function
ce_ciede2000_pixels and this file give the same integer q for every pixel.  No libm function is called on the path to q: the
cube root, the hue angle, the sines and cosines of degrees and the exponential are the fixed sequences cbrt_fixed, hue_deg,
sincos_deg and exp_fixed.  libm_q20 states the same formula with numpy's own cbrt / arctan2 / sin / cos / exp, for comparison.

The sRGB -> linear table is the library's (ce_srgb_table(depth, 0)); callers hand it in, so this file imports nothing of the
library."""
import numpy as np

F = np.float64
M = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
XN, ZN = 0.950456, 1.088754
EPS, KAPPA = 216.0 / 24389.0, 24389.0 / 27.0
POW25_7 = 6103515625.0
DEG, RAD = 57.29577951308232, 0.017453292519943295  # 180 / pi, pi / 180
TAN_PI_8 = 0.41421356237309503
CBRT2, CBRT4 = 1.2599210498948732, 1.5874010519681994
LN2 = 0.6931471805599453
MAX_THRESHOLDS = 8


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.int64)


def _from_bits(b):
    return np.ascontiguousarray(b, np.int64).view(F)


def cbrt_fixed(t):
    """cbrt of a normal t > 0: t = m 2^e, m in [1, 2); e = 3 k + r; y0 = 0.7401 + 0.2599 m; three Halley steps
    y = y (y^3 + 2 m) / (2 y^3 + m); times cbrt(2)^r; times 2^k built from bits."""
    t = np.asarray(t, F)
    bits = _bits(t)
    e = ((bits >> 52) & 0x7FF) - 1023
    m = _from_bits((bits & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000)
    e3 = e + 3072
    k3 = e3 // 3
    r = e3 - 3 * k3
    k = k3 - 1024
    y = F(0.7401) + F(0.2599) * m
    m2 = m + m
    for _ in range(3):
        y3 = (y * y) * y
        y = (y * (y3 + m2)) / ((y3 + y3) + m)
    c = np.where(r == 0, F(1.0), np.where(r == 1, F(CBRT2), F(CBRT4)))
    scale = _from_bits((k + 1023) << 52)
    return (y * c) * scale


ATAN_C = [F((-1.0) ** k) / F(2 * k + 1) for k in range(25)]  # 1, -1/3, ... 1/49: quotients of literals, correctly rounded


def hue_deg(b, a):
    """atan2(b, a) in degrees in [0, 360), 0 at a = b = 0."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ax, ay = np.abs(a), np.abs(b)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    zero = mx == 0.0
    with np.errstate(all="ignore"):
        t = mn / np.where(zero, F(1.0), mx)
        big = t > TAN_PI_8
        u = np.where(big, (t - 1.0) / (t + 1.0), t)
        u2 = u * u
        p = ATAN_C[24]
        for k in range(23, -1, -1):
            p = p * u2 + ATAN_C[k]
        d = (u * p) * F(DEG)
        d = np.where(big, d + 45.0, d)
        d = np.where(ay > ax, 90.0 - d, d)
        d = np.where(a < 0.0, 180.0 - d, d)
        d = np.where(b < 0.0, 360.0 - d, d)
        d = np.where(d >= 360.0, d - 360.0, d)
    return np.where(zero, F(0.0), d)


SIN_C = [F(s) / F(f) for s, f in ((1.0, 1.0), (-1.0, 6.0), (1.0, 120.0), (-1.0, 5040.0), (1.0, 362880.0), (-1.0, 39916800.0),
                                   (1.0, 6227020800.0), (-1.0, 1307674368000.0), (1.0, 355687428096000.0))]  # to r^17
COS_C = [F(s) / F(f) for s, f in ((1.0, 1.0), (-1.0, 2.0), (1.0, 24.0), (-1.0, 720.0), (1.0, 40320.0), (-1.0, 3628800.0),
                                   (1.0, 479001600.0), (-1.0, 87178291200.0), (1.0, 20922789888000.0),
                                   (-1.0, 6402373705728000.0))]  # to r^18


def sincos_deg(x):
    """(sin, cos) of x degrees: n = rint(x / 90), r = x - 90 n (exact), rr = r (pi / 180), Taylor in Horner form."""
    x = np.asarray(x, F)
    n = np.rint(x / 90.0)
    r = x - 90.0 * n
    rr = r * F(RAD)
    r2 = rr * rr
    s = SIN_C[8]
    for k in range(7, -1, -1):
        s = s * r2 + SIN_C[k]
    s = rr * s
    c = COS_C[9]
    for k in range(8, -1, -1):
        c = c * r2 + COS_C[k]
    q = n.astype(np.int64) & 3
    sn = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    cs = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    return sn, cs


EXP_C = [F(1.0) / F(f) for f in (87178291200.0, 6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0,
                                  720.0, 120.0, 24.0, 6.0, 2.0, 1.0, 1.0)]


def exp_fixed(y):
    """exp y for y in [-700, 0]: n = rint(y / ln2), f = y - n ln2, hlg_pixel.h's exp_times_pow2(f, n)."""
    y = np.asarray(y, F)
    n = np.rint(y / F(LN2))
    f = y - n * F(LN2)
    q = EXP_C[0]
    for c in EXP_C[1:]:
        q = q * f + c
    return q * _from_bits((n.astype(np.int64) + 1023) << 52)


def pow7(c):
    c3 = (c * c) * c
    return (c3 * c3) * c


def lab(rgb, depth, table):
    """[..., 3] integer samples of `depth` bits -> L, a, b (f64); table = ce_srgb_table(depth, 0), f32."""
    maxv = (1 << depth) - 1
    v = np.minimum(np.asarray(rgb).astype(np.int64), maxv)
    e = np.asarray(table, np.float32)[v].astype(F)
    er, eg, eb = e[..., 0], e[..., 1], e[..., 2]
    x, y, z = [(F(m[0]) * er + F(m[1]) * eg) + F(m[2]) * eb for m in M]
    x, z = x / F(XN), z / F(ZN)

    def f(t):
        big = t > EPS
        return np.where(big, cbrt_fixed(np.where(big, t, F(1.0))), (F(KAPPA) * t + 16.0) / 116.0)

    fx, fy, fz = f(x), f(y), f(z)
    return 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)


def delta_e(l1, a1, b1, l2, a2, b2, fixed=True):
    """CIEDE2000 (kL = kC = kH = 1) of Lab arrays, f64.  fixed: the library's sequences; else numpy's libm."""
    if fixed:
        hue, sc, ex = hue_deg, sincos_deg, exp_fixed
    else:
        def hue(b, a):
            h = np.degrees(np.arctan2(b, a))
            h = np.where(h < 0.0, h + 360.0, h)
            return np.where((a == 0.0) & (b == 0.0), 0.0, h)

        def sc(x):
            return np.sin(np.radians(x)), np.cos(np.radians(x))

        ex = np.exp
    l1, a1, b1, l2, a2, b2 = [np.asarray(v, F) for v in (l1, a1, b1, l2, a2, b2)]
    c1 = np.sqrt(a1 * a1 + b1 * b1)
    c2 = np.sqrt(a2 * a2 + b2 * b2)
    cb = 0.5 * (c1 + c2)
    cb7 = pow7(cb)
    g = 0.5 * (1.0 - np.sqrt(cb7 / (cb7 + POW25_7)))
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
    cpb7 = pow7(cpb)
    rc = 2.0 * np.sqrt(cpb7 / (cpb7 + POW25_7))
    l50 = lb - 50.0
    l50 = l50 * l50
    sl = 1.0 + (0.015 * l50) / np.sqrt(20.0 + l50)
    s_c = 1.0 + 0.045 * cpb
    sh = 1.0 + (0.015 * cpb) * t
    rt = (-sc(2.0 * dth)[0]) * rc
    tl, tc, th = dl / sl, dc / s_c, dH / sh
    s = ((tl * tl + tc * tc) + th * th) + rt * (tc * th)
    return np.sqrt(np.maximum(s, 0.0))


def q20(ref, ref_depth, ref_table, test, test_depth, test_table):
    """-> uint32 array of the pixels' q = rint(dE 2^20); ref / test: [..., 3] integer samples."""
    de = delta_e(*lab(ref, ref_depth, ref_table), *lab(test, test_depth, test_table))
    return np.rint(de * 1048576.0).astype(np.uint64).astype(np.uint32)


def lab_libm(rgb, depth, table):
    maxv = (1 << depth) - 1
    e = np.asarray(table, np.float32)[np.minimum(np.asarray(rgb).astype(np.int64), maxv)].astype(F)
    xyz = [(F(m[0]) * e[..., 0] + F(m[1]) * e[..., 1]) + F(m[2]) * e[..., 2] for m in M]
    fx, fy, fz = [np.where(t > EPS, np.cbrt(t), (KAPPA * t + 16.0) / 116.0) for t in (xyz[0] / XN, xyz[1], xyz[2] / ZN)]
    return 116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)


def delta_e_libm(ref, ref_depth, ref_table, test, test_depth, test_table):
    """The same formula through numpy's cbrt, arctan2, sin, cos and exp: dE as f64."""
    return delta_e(*lab_libm(ref, ref_depth, ref_table), *lab_libm(test, test_depth, test_table), fixed=False)


def scores(q, thresholds=()):
    """What ce_batch_ciede2000 returns for one pair from its pixels' q (any shape)."""
    q = np.asarray(q, np.uint32).reshape(-1)
    s = int(q.astype(np.uint64).sum())
    mx = int(q.max())
    n = int(q.size)
    mean = (s / 1048576.0) / n
    return {"sum_q20": s, "max_q20": mx, "n": n, "n_above": [int((q > np.uint32(t)).sum()) for t in thresholds],
            "mean": mean, "max": mx / 1048576.0, "ciede2000_db": float("inf") if s == 0 else 45.0 - 20.0 * float(np.log10(mean))}
