"""Butteraugli's front end at the image's edges (k_ba_front: packed loads on every tile, the mirrored rim written into LDS once,
one blur form for every tile and sample type; codec-eval_amd/csrc/ba_front_geom.h) against the CPU oracle.

With the two switches of tests/test_gpu_butteraugli.py the oracle is the device's arithmetic exactly, so the scores are compared
with == and the 3-norms to f64 round-off: a wrong mirror source, a cell loaded twice or not at all, or a doubled odd edge taken
by the packed route moves the planes and with them the score.  The content is a ramp plus noise, so that every border pixel
differs from its neighbours and from its mirror image's neighbours.  Shapes: single-tile images; last tiles of 1, 2, 3 and 4
columns or rows; sizes around 64 / 65, whose half-resolution level is 32 or 33 wide; 8-wide and 8-high strips; the two
benchmark shapes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEVICE_SWITCHES = ("ba_malta_f32", "ba_l2_early")  # tests/test_gpu_butteraugli.py

SHAPES = [(8, 8), (31, 9), (32, 32),
          (33, 36), (34, 35), (35, 34), (36, 33),
          (64, 64), (65, 64), (64, 65), (65, 65), (63, 66), (66, 63),
          (8, 200), (200, 8),
          (512, 512), (768, 512)]


def pair(w, h, seed):
    """(h, w, 3) uint8 reference and distorted image: a ramp in both directions plus per-sample noise; the distorted image adds
    a smoother error and noise of its own."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    ramp = np.stack([(5 * x + 3 * y) % 200, (2 * x + 7 * y + 40) % 200, (255 - 3 * x - 2 * y) % 200], -1)
    ref = np.clip(ramp + rng.integers(0, 56, (h, w, 3)), 0, 255).astype(np.uint8)
    wave = 10.0 * np.sin(x / 3.0 + seed)[..., None] + 8.0 * np.cos(y / 2.5)[..., None]
    test = np.clip(ref.astype(np.float64) + wave + rng.integers(-6, 7, (h, w, 3)), 0, 255).astype(np.uint8)
    return ref, test


@pytest.fixture(scope="module")
def expected(oracle):
    """(score, 3-norm) of the oracle with the device's two switches on, computed once per pair and shared."""
    cache = {}

    def get(key, ref, test, w, h):
        if key not in cache:
            assert oracle.variants_all_default()
            for v in DEVICE_SWITCHES:
                oracle.set_variant(v, 1)
            try:
                cache[key] = oracle.butteraugli(ref, test, w, h)
            finally:
                for v in DEVICE_SWITCHES:
                    oracle.set_variant(v, 0)
            assert oracle.variants_all_default()
        return cache[key]
    return get


def check(got, got_p3, want, label):
    print(f"{label}: device {got!r} / {got_p3!r} oracle {want[0]!r} / {want[1]!r}")
    assert got == want[0], (label, got, want[0])
    assert abs(got_p3 - want[1]) <= 1e-13 * abs(want[1]), (label, got_p3, want[1])


def run_batch(ce, batch, refs, tests, pair_ref):
    for i, r in enumerate(refs):
        batch.set_reference(i, r)
    for p, t in enumerate(tests):
        batch.set_test(p, pair_ref[p], t)
    out = batch.run(len(tests), ce.MetricConfig(butteraugli=True))
    p3 = batch.butteraugli_pnorm3(len(tests))
    for s in out:
        assert s.status == 0 and s.valid == ce.METRIC_BUTTERAUGLI
    return [s.butteraugli for s in out], [float(v) for v in p3]


@pytest.mark.parametrize("w,h", SHAPES)
def test_u8_batch_is_the_oracle_bit_for_bit(gpu_ctx, ce, expected, w, h):
    ref, test = pair(w, h, 7 * w + h)
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        got, p3 = run_batch(ce, b, [ref], [test], [0])
    finally:
        b.close()
    check(got[0], p3[0], expected((w, h), ref, test, w, h), f"u8 {w}x{h}")


@pytest.mark.parametrize("w,h", [(33, 35), (65, 34)])
def test_deep_batch_runs_the_shared_stages(gpu_ctx, ce, expected, w, h):
    """16-bit samples v8 * 257 are the 8-bit image (tests/test_gpu_deep_input.py's second anchor): the same score, through
    k_ba_front<*, uint16_t>."""
    ref, test = pair(w, h, 7 * w + h)
    b = gpu_ctx.batch_deep(w, h, 1, 1, 16, 16)
    try:
        got, p3 = run_batch(ce, b, [ref.astype(np.uint16) * 257], [test.astype(np.uint16) * 257], [0])
    finally:
        b.close()
    check(got[0], p3[0], expected((w, h), ref, test, w, h), f"u16 {w}x{h}")


@pytest.mark.parametrize("w,h", [(33, 35), (65, 34)])
def test_linear_batch_runs_the_shared_stages(gpu_ctx, ce, expected, w, h):
    """The library's own table entries as floats are the 8-bit image (tests/test_gpu_linear_input.py's first anchor): the same
    score, through k_ba_front<*, float>."""
    ref, test = pair(w, h, 7 * w + h)
    t = ce.srgb_table(8, 0)
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        got, p3 = run_batch(ce, b, [t[ref]], [t[test]], [0])
    finally:
        b.close()
    check(got[0], p3[0], expected((w, h), ref, test, w, h), f"f32 {w}x{h}")


def test_one_pair_call(gpu_ctx, expected):
    w, h = 35, 33
    ref, test = pair(w, h, 7 * w + h)
    got = gpu_ctx.calculate_butteraugli(ref, test, w, h)
    want = expected((w, h), ref, test, w, h)
    print(f"one pair {w}x{h}: device {got!r} oracle {want[0]!r}")
    assert got == want[0]


def test_two_distorted_images_per_reference(gpu_ctx, ce, expected):
    """Two references with two distorted images each: the images are packed in their slabs, so at 66 x 35 (20790 bytes per
    image) the second image of a slab starts two bytes off a dword and its first and last packed windows are refused."""
    w, h = 66, 35
    refs, tests, pair_ref, keys = [], [], [], []
    for i in range(2):
        r, t0 = pair(w, h, 100 + i)
        r1, t1 = pair(w, h, 200 + i)  # another pair's error, put on this reference
        t1 = np.clip(r.astype(np.int16) + (t1.astype(np.int16) - r1.astype(np.int16)), 0, 255).astype(np.uint8)
        refs.append(r)
        for k, t in enumerate((t0, t1)):
            tests.append(t)
            pair_ref.append(i)
            keys.append(("grid", i, k))
    b = ce.Batch(gpu_ctx, w, h, 2, 4)
    try:
        got, p3 = run_batch(ce, b, refs, tests, pair_ref)
    finally:
        b.close()
    for p in range(4):
        check(got[p], p3[p], expected(keys[p], refs[pair_ref[p]], tests[p], w, h), f"grid pair {p}")
