"""The alpha compositor's definition (tests/alpha_restatement.py) pinned without a device: against Pillow's
Image.alpha_composite on all 2^24 (c, a, bg) triples at 8 bits, against Python's integers at 10, 12 and 16 bits (with
c = a = bg = m, the largest intermediate), its properties, the 8-to-d background scaling, and the package's own host
composite (codec_eval_amd.composite_over, what the device-free multi-device sweep uses)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_restatement as A  # noqa: E402


def test_8bit_equals_pillow_alpha_composite_on_every_triple():
    Image = pytest.importorskip("PIL.Image")
    c, a = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))  # [a][c]
    mismatches = 0
    for bg in range(256):
        # R carries c, G the complement, B a constant: three channels of one image exercise three colour values per alpha
        src = np.stack([c, 255 - c, np.full_like(c, 77), a], -1)
        back = Image.new("RGBA", (256, 256), (bg, bg, bg, 255))
        got = np.asarray(Image.alpha_composite(back, Image.fromarray(src, "RGBA")))
        assert np.all(got[..., 3] == 255)
        want = A.composite(src, (bg, bg, bg))
        mismatches += int(np.count_nonzero(got[..., :3] != want))
    assert mismatches == 0


def test_hand_derived_cases():
    # (c, a, bg) -> out at m = 255: 200*128 + 50*127 + 127 = 32077, // 255 = 125
    for (c, a, bg), out in {(200, 128, 50): 125, (255, 255, 0): 255, (0, 255, 255): 0, (13, 0, 201): 201, (255, 1, 0): 1,
                            (0, 1, 255): 254, (255, 127, 0): 127, (255, 128, 255): 255, (1, 127, 0): 0, (1, 128, 0): 1,
                            (100, 254, 200): 100, (10, 51, 20): 18}.items():
        assert A.composite_int(c, a, bg, 255) == out, (c, a, bg)
        px = np.array([[c, c, c, a]], np.uint8)
        assert A.composite(px, (bg, bg, bg)).tolist() == [[out] * 3]
    # 10 bits: 1000*512 + 100*511 + 511 = 563611, // 1023 = 550
    assert A.composite_int(1000, 512, 100, 1023) == 550
    assert A.composite(np.array([[1000, 0, 1023, 512]], np.uint16), (100, 100, 100), 10).tolist() == [[550, 50, 562]]
    # samples above m are clamped first: c = 5000 -> 1023, a = 2000 -> 1023
    assert A.composite(np.array([[5000, 7, 1024, 2000]], np.uint16), (3, 3, 3), 10).tolist() == [[1023, 7, 1023]]


@pytest.mark.parametrize("depth", [10, 12, 16])
def test_deep_form_equals_python_integers(depth):
    m = (1 << depth) - 1
    rng = np.random.default_rng(depth)
    edge = np.array([0, 1, 2, m // 2, m // 2 + 1, m - 1, m], np.int64)
    vals = np.concatenate([edge, rng.integers(0, m + 1, 40)])
    c, a, bg = (x.reshape(-1) for x in np.meshgrid(vals, vals, vals, indexing="ij"))
    assert (c == m).any() and ((c == m) & (a == m) & (bg == m)).any()  # the largest intermediate: m * m + (m >> 1)
    assert m * m + (m >> 1) < 1 << 32
    want = np.array([A.composite_int(ci, ai, bi, m) for ci, ai, bi in zip(c.tolist(), a.tolist(), bg.tolist())])
    for b in np.unique(bg):
        sel = bg == b
        px = np.stack([c[sel], c[sel], c[sel], a[sel]], -1).astype(np.uint16)
        got = A.composite(px, (int(b),) * 3, depth)
        assert np.array_equal(got, np.repeat(want[sel][:, None], 3, 1))
    assert A.composite_int(m, m, m, m) == m


@pytest.mark.parametrize("depth", A.DEPTHS)
def test_properties(depth):
    m = (1 << depth) - 1
    rng = np.random.default_rng(100 + depth)
    dt = np.uint8 if depth == 8 else np.uint16
    px = A.random_rgba(rng, 64, 48, depth)
    bg = tuple(int(v) for v in rng.integers(0, m + 1, 3))
    opaque, clear = px.copy(), px.copy()
    opaque[..., 3], clear[..., 3] = m, 0
    assert np.array_equal(A.composite(opaque, bg, depth), px[..., :3])  # a = m gives c
    assert np.array_equal(A.composite(clear, bg, depth), np.broadcast_to(np.array(bg, dt), (48, 64, 3)))  # a = 0 gives bg
    # monotone in c for every alpha: all c of a coarse-to-fine ladder, a and bg sampled (8 bits: every a)
    cs = np.arange(m + 1, dtype=np.int64) if depth <= 12 else np.unique(np.concatenate([np.arange(0, m + 1, 17), [m - 1, m]]))
    alphas = np.arange(256) if depth == 8 else np.unique(np.concatenate([[0, 1, m // 2, m - 1, m], rng.integers(0, m + 1, 24)]))
    for b in (0, m // 3, m):
        ramp = np.zeros((len(alphas), len(cs), 4), dt)
        ramp[..., 0] = ramp[..., 1] = ramp[..., 2] = cs[None, :]
        ramp[..., 3] = alphas[:, None]
        out = A.composite(ramp, (b, b, b), depth).astype(np.int64)
        assert np.all(np.diff(out[..., 0], axis=1) >= 0)
        assert out.min() >= 0 and out.max() <= m


def test_background_scaling():
    assert A.scale_background((0, 128, 255), 8) == (0, 128, 255)
    assert A.scale_background((0, 128, 255), 10) == (0, (128 * 1023 + 127) // 255, 1023) == (0, 514, 1023)
    assert A.scale_background((1, 254, 255), 16) == (257, 65278, 65535)  # v * 257 exactly at 16 bits
    for d in A.DEPTHS:
        m = (1 << d) - 1
        s = [A.scale_background((v, v, v), d)[0] for v in range(256)]
        assert s[0] == 0 and s[255] == m and all(y > x for x, y in zip(s, s[1:]))
        assert all(abs(v * m / 255 - x) <= 0.5 for v, x in enumerate(s))


def test_package_host_composite_equals_the_restatement(ce):
    rng = np.random.default_rng(5)
    for depth in A.DEPTHS:
        m = (1 << depth) - 1
        for dt in ((np.uint8, np.uint16) if depth == 8 else (np.uint16,)):
            px = A.random_rgba(rng, 33, 21, depth, dt, over=True)
            for bg in ((0, 0, 0), (m, m, m), tuple(int(v) for v in rng.integers(0, m + 1, 3))):
                got = ce.composite_over(px, bg, depth)
                assert got.dtype == dt and np.array_equal(got, A.composite(px, bg, depth))
        assert ce.scale_background((0, 128, 255), depth) == A.scale_background((0, 128, 255), depth)
    assert ce.ALPHA_BLACK_WHITE == ((0, 0, 0), (255, 255, 255)) and ce.MAX_BACKGROUNDS == 8
    with pytest.raises(ValueError):
        ce.composite_over(np.zeros((1, 4), np.uint16), (1024, 0, 0), 10)
