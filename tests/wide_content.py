"""Wide content for linear batches: deterministic float32 pairs designed from the operand ranges of the metric kernels'
hand-expanded divisions ("Operand ranges"), shared by tests/test_wide_content_cpu.py and tests/test_gpu_wide_content.py.

A linear batch takes any float in [-CE_LINEAR_MAX, CE_LINEAR_MAX] = +-1024, negatives and subnormals included; the metric
kernels were written for 8-bit sRGB, where every linear sample is one of 256 values in [0, 1].  Every generator returns
(name, ref, test) as float32 [h, w, 3] that equal their own cicp_restatement.sanitise (asserted in the CPU test).
"""
import numpy as np

LINEAR_MAX = np.float32(1024.0)  # include/ce_metrics.h: CE_LINEAR_MAX
W, H = 96, 64  # two Malta tile columns (one partial), two DSSIM 60-column strips, two SSIMULACRA2 64-column strips, a 48 x 32 second Butteraugli level
ODD_W, ODD_H = 97, 35  # once per class: the mirrored and border paths at the same magnitudes
CROSS_W, CROSS_H = 512, 256  # lab_crossing
INTENSITIES = (80.0, 203.0, 10000.0)  # the stated domain of intensity_target for linear batches (include/ce_metrics.h)
LAB_EPSILON = 216.0 / 24389.0  # rgb_to_lab's select boundary (oracle/dssim.c)
SMALLEST_SUBNORMAL = np.float32(1.401298464324817e-45)  # 2^-149


def _clip(a):
    return np.clip(np.asarray(a, np.float32), -LINEAR_MAX, LINEAR_MAX).astype(np.float32)


def _rgb(plane):
    return np.ascontiguousarray(np.repeat(np.asarray(plane, np.float32)[..., None], 3, axis=-1))


def logramp_ref(w, h):
    """|v| = 2^e with e running from -149 (the smallest subnormal) to 10 (1024) along x; three row bands: every channel
    positive, every channel negative, and signs (+, -, +) / (-, +, -) on alternate rows."""
    e = -149.0 + 159.0 * np.arange(w, dtype=np.float64) / (w - 1)
    mag = np.exp2(e).astype(np.float32)
    assert mag[0] == SMALLEST_SUBNORMAL and mag[-1] == LINEAR_MAX
    out = np.empty((h, w, 3), np.float32)
    out[:] = mag[None, :, None]
    b0, b1 = h // 3, 2 * h // 3
    out[b0:b1] *= np.float32(-1.0)
    sign = np.array([1.0, -1.0, 1.0], np.float32)
    for y in range(b1, h):
        out[y] *= sign if (y - b1) % 2 == 0 else -sign
    return out


def logramp(w, h):
    ref = logramp_ref(w, h)
    rng = np.random.default_rng(101)
    noise = (rng.random(ref.shape, np.float32) - np.float32(0.5)) * np.float32(0.02)
    return [("logramp_x1.05", ref, _clip(ref * np.float32(1.05))), ("logramp_noise", ref, _clip(ref + noise))]


def checker_ref(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return _rgb(np.where((x + y) % 2 == 0, LINEAR_MAX, -LINEAR_MAX))


def checker(w, h):
    ref = checker_ref(w, h)
    test = ref.copy()
    test[2::5, 3::7] *= np.float32(0.9)  # a sparse lattice
    return [("checker", ref, test)]


def spikes(w, h):
    """1000 on a background of -0.05: the blurred opsin is clamped to 1e-4 next to (and under) a large unblurred value."""
    ref = np.full((h, w, 3), -0.05, np.float32)
    test = ref.copy()
    ref[4::9, 5::11] = np.float32(1000.0)
    test[4::9, 5::11] = np.float32(900.0)
    return [("spikes", ref, test)]


def neg_noise(w, h):
    rng = np.random.default_rng(102)
    ref = (rng.random((h, w, 3), np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    noise = (rng.random(ref.shape, np.float32) - np.float32(0.5)) * np.float32(0.1)
    return [("neg_noise", ref, _clip(ref + noise))]


def hdr_noise(w, h):
    rng = np.random.default_rng(103)
    ref = (rng.random((h, w, 3), np.float32) * np.float32(5.0)).astype(np.float32)
    noise = (rng.random(ref.shape, np.float32) - np.float32(0.5)) * np.float32(0.2)
    return [("hdr_noise", ref, _clip(ref + noise))]


def lab_threshold(w, h):
    """Ramps dense around 216/24389 - where rgb_to_lab selects between cbrt_poly and the linear segment - in grey and in
    one channel at a time (the others 0; the ramp is scaled so that the channel's own XYZ term crosses), and a ramp through
    0 from both sides with subnormals on either side of it."""
    t = np.linspace(-1.0, 1.0, w * (h // 5), dtype=np.float64).reshape(h // 5, w)
    around = LAB_EPSILON * (1.0 + 0.02 * t)
    out = np.zeros((h, w, 3), np.float32)
    band = h // 5
    out[0:band] = around[..., None]
    # fx = r * 0.4124 / 0.9505, fy = g * 0.7152, fz = b * 0.9505 / 1.089 with the other two channels at 0
    for c, k in enumerate((0.4124 / 0.9505, 0.7152, 0.9505 / 1.089)):
        out[(c + 1) * band:(c + 2) * band, :, c] = around / k
    rest = h - 4 * band
    z = np.linspace(-1.0, 1.0, w * rest, dtype=np.float64).reshape(rest, w)
    zero = np.sign(z) * np.exp2(-149.0 + 139.0 * np.abs(z))  # +-2^-149 (at z = +-0) .. +-2^-10
    out[4 * band:] = zero[..., None]
    ref = out
    rng = np.random.default_rng(104)
    noise = (rng.random(ref.shape, np.float32) - np.float32(0.5)) * np.float32(4e-4)
    return [("lab_threshold", ref, _clip(ref + noise))]


def saturated(w, h, identical=True):
    hi, lo, zero = (np.full((h, w, 3), v, np.float32) for v in (LINEAR_MAX, -LINEAR_MAX, 0.0))
    out = [("saturated_+1024_-1024", hi, lo), ("saturated_0_0", zero, zero.copy())]
    if identical:
        c = checker_ref(w, h)
        out.append(("saturated_identical_checker", c, c.copy()))  # must score exactly (100.0, 0.0, 0.0)
    return out


CLASSES = {"logramp": logramp, "checker": checker, "spikes": spikes, "neg_noise": neg_noise, "hdr_noise": hdr_noise,
           "lab_threshold": lab_threshold, "saturated": saturated}
IDENTICAL = "saturated_identical_checker"


def working_set():
    """Every class at the working shape."""
    return [case for gen in CLASSES.values() for case in gen(W, H)]


def odd_set():
    """One pair per class at 97 x 35."""
    return [gen(ODD_W, ODD_H)[0] for gen in CLASSES.values()]


def grid(cases):
    """-> refs, tests, pair_ref: the cases as the pairs of one batch; cases that share a reference array share a slot."""
    refs, tests, pair_ref = [], [], []
    for _, ref, test in cases:
        slot = next((i for i, r in enumerate(refs) if r is ref), None)
        if slot is None:
            slot = len(refs)
            refs.append(ref)
        tests.append(test)
        pair_ref.append(slot)
    return refs, tests, pair_ref


# ---- lab_crossing (DSSIM only) -------------------------------------------------------------------------------------
def _bits(x):
    return int(np.float32(x).view(np.uint32))


def _from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def crossing_bits(cbrt_den, step, lo=LAB_EPSILON * 1.001, hi=8.0, scan=4096):
    """The float32s (as bit patterns) at which the denominator of cbrt_poly's Halley step `step`, 2 y^3 + x, steps over zero,
    located with the probe `cbrt_den(x, step)` (linear_input_shim.Shim.cbrt_den): a coarse scan of [lo, hi] - above 8 the
    seed polynomial falls as -x^2 / 2 and both denominators stay negative - then bisection over bit patterns.  Sign changes
    through a pole (the second denominator where the first crosses: the values on either side are huge) are not zeros."""
    xs = np.exp(np.linspace(np.log(lo), np.log(hi), scan)).astype(np.float32)
    d = [cbrt_den(x, step) for x in xs]
    found = []
    for i in range(scan - 1):
        if d[i] * d[i + 1] < 0.0 and max(abs(d[i]), abs(d[i + 1])) < 1.0:
            a, b, up = _bits(xs[i]), _bits(xs[i + 1]), d[i] > 0.0
            while b - a > 1:
                m = (a + b) // 2
                if (cbrt_den(_from_bits(m), step) > 0.0) == up:
                    a = m
                else:
                    b = m
            found.append(b)
    return found


def _grey_window(centre):
    n = CROSS_W * CROSS_H
    return _rgb(_from_bits(np.arange(centre - n // 2, centre + n // 2, dtype=np.int64).astype(np.uint32)).reshape(CROSS_H, CROSS_W))


def lab_crossing(cbrt_den):
    """512 x 256, test = ref * 1.001.
    `grey`: every consecutive float32 of a window centred on the zero of cbrt_poly's FIRST denominator (x near 3.78, where
    the cube root has a pole), row-major, in all three channels (fx, fy and fz are the grey value to an ulp).
    `bands`: three row bands in which only R, only G or only B runs through consecutive floats - the other two channels at
    0.25 - placed so that fx, fy or fz alone crosses.
    `step2_*`: the same grey window around each zero of the SECOND denominator (x near 3.46 and 4.56)."""
    first = crossing_bits(cbrt_den, 1)
    assert len(first) == 1, first
    centre = first[0]
    x0 = float(_from_bits(centre))
    grey = _grey_window(centre)
    bands = np.full((CROSS_H, CROSS_W, 3), 0.25, np.float32)
    rows = [0, 85, 170, CROSS_H]
    # fx = (0.4124 r + 0.3576 g + 0.1805 b) / 0.9505, fy = 0.2126 r + 0.7152 g + 0.0722 b, fz = (0.0193 r + 0.1192 g + 0.9505 b) / 1.089
    solve = ((x0 * 0.9505 - 0.25 * (0.3576 + 0.1805)) / 0.4124, (x0 - 0.25 * (0.2126 + 0.0722)) / 0.7152,
             (x0 * 1.089 - 0.25 * (0.0193 + 0.1192)) / 0.9505)
    for c in range(3):
        m = (rows[c + 1] - rows[c]) * CROSS_W
        mid = _bits(solve[c])
        bands[rows[c]:rows[c + 1], :, c] = _from_bits(np.arange(mid - m // 2, mid - m // 2 + m, dtype=np.int64).astype(np.uint32)).reshape(-1, CROSS_W)
    k = np.float32(1.001)
    out = [("lab_crossing_grey", grey, (grey * k).astype(np.float32)), ("lab_crossing_bands", bands, (bands * k).astype(np.float32))]
    second = crossing_bits(cbrt_den, 2)
    assert len(second) == 2, second
    for i, c in enumerate(second):
        g = _grey_window(c)
        out.append((f"lab_crossing_step2_{i}", g, (g * k).astype(np.float32)))
    return out
