"""CIEDE2000 without a GPU (include/ce_metrics.h: ce_batch_ciede2000's definition, ce_ciede2000_pixels).
The numpy restatement (tests/ciede2000_restatement.py) against the published table of Sharma, Wu and Dalal
(tests/golden/ciede2000_sharma2005.txt), against the same formula through numpy's libm and against its anchors; then the
library's host function - the kernel's pixel text compiled for the host - against the restatement with == on every pixel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_cases as K  # noqa: E402
import ciede2000_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = np.loadtxt(os.path.join(ROOT, "tests", "golden", "ciede2000_sharma2005.txt"))
# the two pairs whose hues lie 180 degrees apart, on the formula's own discontinuity: either side of it is a right answer
KNIFE_EDGE = {(50.0, 2.49, -0.001, 50.0, -2.49, 0.001): (7.1792, 7.2195), (50.0, -0.001, 2.49, 50.0, 0.001, -2.49): (4.8045, 4.7461)}


@pytest.fixture(scope="module", autouse=True)
def tables(ce):
    K.use(ce)
    return K.TABLES


def test_published_table():
    assert TABLE.shape == (34, 7)
    for fixed in (True, False):
        for a, b in ((TABLE[:, :3], TABLE[:, 3:6]), (TABLE[:, 3:6], TABLE[:, :3])):  # and with the sides exchanged
            got = R.delta_e(*a.T, *b.T, fixed=fixed)
            for row, g in zip(TABLE, got):
                allowed = KNIFE_EDGE.get(tuple(row[:6]), KNIFE_EDGE.get(tuple(row[3:6]) + tuple(row[:3]), (row[6],)))
                assert row[6] in allowed
                assert min(abs(g - v) for v in allowed) <= 0.00005, (fixed, row, g)
    # plain libm gives every published value, the knife edges included
    assert np.abs(R.delta_e(*TABLE[:, :6].T, fixed=False) - TABLE[:, 6]).max() <= 0.00005


def fixed_seed_sets():
    rng = np.random.default_rng(2000)
    n = 400000
    r = rng.integers(0, 256, (n, 3))
    yield "random 8-bit pairs", r, rng.integers(0, 256, (n, 3))
    yield "pairs within +-3 codes", r, np.clip(r + rng.integers(-3, 4, (n, 3)), 0, 255)
    g = np.repeat(rng.integers(0, 256, (200000, 1)), 3, 1)
    yield "greys against near-greys", g, np.clip(g + rng.integers(-1, 2, (200000, 3)), 0, 255)
    yield "grey against grey", g, np.repeat(rng.integers(0, 256, (200000, 1)), 3, 1)


def test_fixed_sequences_agree_with_libm_within_half_a_quantum(tables):
    """2^-21 is half a unit of q, so q moves by at most one: the bound is that, whatever is measured."""
    t8 = tables[8]
    for name, r, t in fixed_seed_sets():
        fixed = R.delta_e(*R.lab(r, 8, t8), *R.lab(t, 8, t8))
        libm = R.delta_e_libm(r, 8, t8, t, 8, t8)
        worst = float(np.abs(fixed - libm).max())
        dq = int(np.abs(np.rint(fixed * 2.0 ** 20) - np.rint(libm * 2.0 ** 20)).max())
        print(f"{name}: largest |fixed - libm| {worst:.3g}, largest q difference {dq}, largest dE {float(fixed.max()):.4f}")
        assert worst <= 2.0 ** -21, name
        assert fixed.max() < 4096.0  # q fits 32 bits


def test_elementary_sequences_against_libm():
    rng = np.random.default_rng(2001)
    x = np.concatenate([rng.uniform(216.0 / 24389.0, 1.1, 200000), 2.0 ** rng.uniform(-300, 300, 50000)])
    assert np.abs(R.cbrt_fixed(x) / np.cbrt(x) - 1.0).max() < 1e-15
    assert R.cbrt_fixed(np.array([1.0, 8.0, 0.125])).tolist() == [1.0, 2.0, 0.5]
    a, b = rng.uniform(-130, 130, 200000), rng.uniform(-130, 130, 200000)
    h = np.degrees(np.arctan2(b, a))
    assert np.abs(R.hue_deg(b, a) - np.where(h < 0, h + 360.0, h)).max() < 2e-13
    axes = R.hue_deg(np.array([0.0, 1.0, 0.0, -1.0, 1.0, -1.0, -0.0, 0.0, -1e-300]), np.array([1.0, 0.0, -1.0, 0.0, 1.0, -1.0, 1.0, 0.0, 1.0]))
    assert axes.tolist() == [0.0, 90.0, 180.0, 270.0, 45.0, 225.0, 0.0, 0.0, 0.0]
    x = rng.uniform(-200, 1500, 200000)
    s, c = R.sincos_deg(x)
    assert np.abs(s - np.sin(np.radians(x))).max() < 1e-14 and np.abs(c - np.cos(np.radians(x))).max() < 1e-14
    s, c = R.sincos_deg(np.array([0.0, 90.0, 180.0, 270.0, 360.0, -90.0, 30.0]))
    assert s[:6].tolist() == [0.0, 1.0, 0.0, -1.0, 0.0, -1.0] and c[:6].tolist() == [1.0, 0.0, -1.0, 0.0, 1.0, 0.0] and abs(s[6] - 0.5) < 1e-15
    y = rng.uniform(-130, 0, 200000)
    assert np.abs(R.exp_fixed(y) / np.exp(y) - 1.0).max() < 1e-13 and R.exp_fixed(np.array([0.0]))[0] == 1.0


def test_anchors(tables):
    t8, t16 = tables[8], tables[16]
    one = lambda *v: np.array([v])  # noqa: E731
    red = [float(v[0]) for v in R.lab(one(255, 0, 0), 8, t8)]
    assert np.abs(np.array(red) - (53.2406, 80.0942, 67.2015)).max() <= 1e-4, red
    assert [float(v[0]) for v in R.lab(one(255, 255, 255), 8, t8)] == [100.0, 0.0, 0.0]
    assert [float(v[0]) for v in R.lab(one(0, 0, 0), 8, t8)] == [0.0, 0.0, 0.0]
    # black against white is L = 0 against L = 100 at zero chroma: S_L = 1 at Lbar = 50, so dE = 100 exactly
    assert R.q20(one(0, 0, 0), 8, t8, one(255, 255, 255), 8, t8)[0] == 100 << 20
    rng = np.random.default_rng(2002)
    a, b = rng.integers(0, 256, (50000, 3)), rng.integers(0, 256, (50000, 3))
    assert np.array_equal(R.q20(a, 8, t8, b, 8, t8), R.q20(b, 8, t8, a, 8, t8))  # symmetric
    assert not R.q20(a, 8, t8, a, 8, t8).any()  # identical gives 0
    assert np.array_equal(t8, t16[257 * np.arange(256)]) and not R.q20(a, 8, t8, 257 * a, 16, t16).any()  # 8-bit v against 16-bit 257 v
    for d in (10, 12, 16):
        deep = rng.integers(0, 1 << d, (20000, 3))
        assert not R.q20(deep, d, tables[d], deep, d, tables[d]).any()


def branch_codes(ref, test, dr, dt, tables):
    """Which way the hue difference wrapped (-1, 0, 1; 2: zero chroma) and which of the mean hue's four rules applied."""
    l1, a1, b1 = R.lab(ref, dr, tables[dr])
    l2, a2, b2 = R.lab(test, dt, tables[dt])
    cb7 = R.pow7(0.5 * (np.sqrt(a1 * a1 + b1 * b1) + np.sqrt(a2 * a2 + b2 * b2)))
    g = 0.5 * (1.0 - np.sqrt(cb7 / (cb7 + R.POW25_7)))
    ap1, ap2 = (1.0 + g) * a1, (1.0 + g) * a2
    h1, h2 = R.hue_deg(b1, ap1), R.hue_deg(b2, ap2)
    zero = np.sqrt(ap1 * ap1 + b1 * b1) * np.sqrt(ap2 * ap2 + b2 * b2) == 0.0
    dh = h2 - h1
    wrap = np.where(zero, 2, np.where(dh > 180.0, 1, np.where(dh < -180.0, -1, 0)))
    mean = np.where(zero, 0, np.where(np.abs(h1 - h2) <= 180.0, 1, np.where(h1 + h2 < 360.0, 2, 3)))
    return set(wrap.tolist()), set(mean.tolist())


def test_the_cases_reach_every_branch(tables):
    """The anchors of tests/ciede2000_cases.py: both wraps of the hue difference, all four rules of the mean hue, zero chroma
    on one side and on both, both pieces of f(t), and the maximum of the formula's range."""
    a = np.array(K.ANCHORS)
    assert branch_codes(a[:, 0], a[:, 1], 8, 8, tables) == ({-1, 0, 1, 2}, {0, 1, 2, 3})
    q = R.q20(a[:, 0], 8, tables[8], a[:, 1], 8, tables[8])
    assert q[0] == q[1] == 100 << 20 and q[2] == q[3] == 0 and (q[4:] > 0).all()
    for kind in K.KINDS:
        for w, h in K.SHAPES:
            got = K.expected(w, h, kind)
            assert got[2]["sum_q20"] == 0 and got[2]["ciede2000_db"] == float("inf") and got[2]["n_above"] == [0] * 8, (kind, w, h)
            assert all(g["sum_q20"] > 0 for i, g in enumerate(got) if i != 2 and (w * h > 3 or i in (1, 3))), (kind, w, h)
            assert all(g["n"] == w * h and g["n_above"][7] == 0 and g["n_above"][0] >= g["n_above"][1] for g in got)


def lattice():
    v = np.linspace(0, 255, 17).round().astype(np.int64)
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)


def host_inputs():
    """(name, reference [n, 3], depth, test [n, 3], depth)"""
    g = np.arange(256)
    gr, gt = np.meshgrid(g, g, indexing="ij")
    yield "all grey pairs", np.repeat(gr.reshape(-1, 1), 3, 1), 8, np.repeat(gt.reshape(-1, 1), 3, 1), 8
    lat = lattice()
    perm = np.random.default_rng(2003).permutation(len(lat))
    yield "17^3 lattice against a permutation of itself", lat, 8, lat[perm], 8
    yield "the lattice at 8 bits against itself at 16", lat, 8, 257 * lat[perm], 16
    # codes around t = 216 / 24389, where f changes pieces: Y reaches it at grey ~ 0.0089 linear, i.e. 8-bit code 23.5
    for d in K.DEPTHS:
        maxv = (1 << d) - 1
        centre = int(round(23.5 / 255 * maxv))
        v = np.arange(max(centre - 40, 0), centre + 40)
        a = np.stack(np.meshgrid(v[::3], v[::5], v[::7], indexing="ij"), -1).reshape(-1, 3)
        yield f"codes around the switch at {d} bits", a, d, a[::-1] + (np.arange(len(a)) % 3)[:, None], d
    rng = np.random.default_rng(2004)
    for dr, dt in ((8, 8), (10, 10), (12, 12), (16, 16), (8, 16), (16, 8), (10, 12), (12, 16)):
        yield f"noise at {dr} / {dt}", rng.integers(0, 1 << dr, (30000, 3)), dr, rng.integers(0, 1 << dt, (30000, 3)), dt
    yield "samples above an 8-bit side's range clamp", rng.integers(200, 400, (2000, 3)), 8, rng.integers(0, 1 << 10, (2000, 3)), 10


def test_host_function_equals_the_restatement_on_every_pixel(ce, tables):
    ys = []
    for name, r, dr, t, dt in host_inputs():
        got = ce.ciede2000_pixels(r, t, dr, dt)
        want = R.q20(r, dr, tables[dr], t, dt, tables[dt])
        assert got.dtype == np.uint32 and np.array_equal(got, want), (name, int(np.abs(got.astype(np.int64) - want).max()))
        if "switch" in name:
            ys.append(R.lab(r, dr, tables[dr])[0])
    # both pieces of f(t) ran on the luminance of those codes: L = 8 is the switch
    assert all(y.min() < 8.0 < y.max() for y in ys) and len(ys) == 4
    anchors = np.array(K.ANCHORS)
    assert np.array_equal(ce.ciede2000_pixels(anchors[:, 0], anchors[:, 1]), R.q20(anchors[:, 0], 8, tables[8], anchors[:, 1], 8, tables[8]))


def test_host_function_refusals(ce):
    L, rgb, out = ce.lib(), np.zeros(6, np.uint16), np.zeros(2, np.uint32)
    for dr, dt in ((9, 8), (8, 0), (16, 17)):
        assert L.ce_ciede2000_pixels(rgb.ctypes.data, dr, rgb.ctypes.data, dt, 2, out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ciede2000_pixels(None, 8, rgb.ctypes.data, 8, 2, out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ciede2000_pixels(rgb.ctypes.data, 8, None, 8, 2, out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ciede2000_pixels(rgb.ctypes.data, 8, rgb.ctypes.data, 8, 2, None) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ciede2000_pixels(rgb.ctypes.data, 8, rgb.ctypes.data, 8, 2, out.ctypes.data) == ce.CE_OK and not out.any()
    import ctypes
    assert ctypes.sizeof(ce.CeCiede2000Scores) == 120
