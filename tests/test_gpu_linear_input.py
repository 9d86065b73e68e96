"""Linear batches and the CICP ingest on the device (ce_batch_create_linear, ce_batch_set_*_cicp),
through the C ABI.

The anchors are EXACT: a linear batch loaded with the library's own sRGB table entries hands the front ends the floats the
RGB8 batch's table lookup hands them, and everything behind is the same code, so every score and every map is compared with
== / array_equal.  The ingest equals tests/cicp_restatement.py byte for byte.  Content the 8-bit path cannot express (PQ
highlights, out-of-gamut P3, plain floats) is held against tests/linear_input_shim.py - the oracle's own stages from float
planes on - with tests/test_gpu_parity.py's bound.
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import cicp_restatement as R
import deep_input_shim as D
import linear_input_shim as LS
from test_gpu_deep_input import hip_runtime, run_everything, same

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4  # tests/test_gpu_parity.py
FLOORS = {"ssimulacra2": 1.0, "dssim": 1e-6, "butteraugli": 1e-3}  # that file's floors (Butteraugli: tests/test_gpu_butteraugli.py's)
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "inputs.npz"))


def golden(name):
    return GOLD[name + ".ref"], GOLD[name + ".test"]


def golden_grid(name):
    """-> refs, tests, pair_ref, w, h: one pair of a golden input, or the 3-reference / 9-pair grid of nat64."""
    if name != "nat64_grid":
        r, t = golden(name)
        return [r], [t], [0], r.shape[1], r.shape[0]
    (r0, t0), (r1, t1) = golden("nat64_q40"), golden("nat64_q85")
    refs = [r0, r1, np.ascontiguousarray(r0[::-1])]
    tests = [t0, t1, np.ascontiguousarray(t0[::-1]), t1, np.ascontiguousarray(t1[:, ::-1]), r0, r1, t0, np.ascontiguousarray(t1[::-1])]
    return refs, tests, [p % 3 for p in range(9)], 64, 64


GRIDS = ["min8x8_q50", "nat97x131_q75_420", "odd257x129_q30_420", "kodak768x512_q75", "nat64_grid"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory, oracle):
    return LS.Shim(tmp_path_factory.mktemp("linear_input_shim"))


@pytest.fixture(scope="module")
def rgb8_results(ce, gpu_ctx):
    """Every score and map of the RGB8 batch of each grid: computed once, shared by the anchors."""
    cache = {}

    def get(name):
        if name not in cache:
            refs, tests, pair_ref, w, h = golden_grid(name)
            b = ce.Batch(gpu_ctx, w, h, len(refs), len(tests))
            try:
                for i, r in enumerate(refs):
                    b.set_reference(i, r)
                for p, t in enumerate(tests):
                    b.set_test(p, pair_ref[p], t)
                cache[name] = run_everything(ce, b, len(tests), w, h)
            finally:
                b.close()
        return cache[name]
    return get


def only(result, which):
    """The part of run_everything's dict that `which` ('s2ba' or 'dssim') vouches for; PSNR and the others blanked."""
    out = {}
    for k, v in result.items():
        if k == "scores":
            out[k] = [((0.0, s[1], s[2], 0.0, s[4] & 6, s[5]) if which == "s2ba" else (s[0], 0.0, 0.0, 0.0, s[4] & 1, s[5])) for s in v]
        elif (k.startswith("ds_")) == (which == "dssim"):
            out[k] = v
    return out


@pytest.mark.parametrize("name", GRIDS)
def test_anchor_a_table_floats_equal_the_rgb8_batch(ce, gpu_ctx, rgb8_results, name):
    refs, tests, pair_ref, w, h = golden_grid(name)
    want = rgb8_results(name)
    lin = gpu_ctx.batch_linear(w, h, len(refs), len(tests))
    try:
        for rule, which in ((0, "s2ba"), (1, "dssim")):
            t = ce.srgb_table(8, rule)
            for i, r in enumerate(refs):
                lin.set_reference(i, t[r])
            for p, x in enumerate(tests):
                lin.set_test(p, pair_ref[p], t[x])
            got = run_everything(ce, lin, len(tests), w, h)
            assert all((s[4] & 8) == 0 and s[5] == 0 for s in got["scores"])  # no PSNR, the rest runs
            same(only(got, which), only(want, which))
            if len(refs) == 1:  # the same through the one-pair call
                leaf = gpu_ctx.eval_pair_linear(t[refs[0]], t[tests[0]], w, h, ce.MetricConfig.all())
                s = want["scores"][0]
                assert leaf.psnr is None
                if rule == 0:
                    assert (leaf.ssimulacra2, leaf.butteraugli) == (s[1], s[2])
                else:
                    assert leaf.dssim == s[0]
    finally:
        lin.close()


def read_slab(batch, which, n_floats):
    out = np.empty(n_floats, np.float32)
    batch.ctx.synchronize()
    assert hip_runtime().hipMemcpy(out.ctypes.data, batch.test_slab if which else batch.reference_slab, out.nbytes, 2) == 0
    return out


@pytest.mark.parametrize("name", GRIDS)
def test_anchor_b_cicp_srgb_upload_equals_anchor_a(ce, gpu_ctx, rgb8_results, name):
    refs, tests, pair_ref, w, h = golden_grid(name)
    want = rgb8_results(name)
    t0 = ce.srgb_table(8, 0)
    lin = gpu_ctx.batch_linear(w, h, len(refs), len(tests))
    try:
        for depth, scale, dt in ((8, 1, np.uint8), (16, 257, np.uint16)):
            colour = ce.ColourDescription(1, 13, depth)
            for i, r in enumerate(refs):
                lin.set_reference_cicp(i, (r.astype(dt) * dt(scale)), colour)
            for p, x in enumerate(tests):
                lin.set_test_cicp(p, pair_ref[p], (x.astype(dt) * dt(scale)), colour)
            lin.run(len(tests), ce.MetricConfig.ssimulacra2_only())  # orders the uploads before the read-back
            assert np.array_equal(read_slab(lin, 0, len(refs) * w * h * 3), np.concatenate([t0[r].reshape(-1) for r in refs]))
            assert np.array_equal(read_slab(lin, 1, len(tests) * w * h * 3), np.concatenate([t0[x].reshape(-1) for x in tests]))
            same(only(run_everything(ce, lin, len(tests), w, h), "s2ba"), only(want, "s2ba"))
    finally:
        lin.close()


def random_codes(rng, w, h, fmt_channels, dt, depth):
    maxv = (1 << depth) - 1
    px = rng.integers(0, maxv + 1, (h, w, fmt_channels)).astype(dt)
    if dt == np.uint16 and depth < 16:
        px[rng.random(px.shape) < 0.05] = dt(min(65535, maxv + 1 + int(rng.integers(0, 1000))))  # above maxv: clamped
    return px


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (17, 9), (100, 76), (768, 512)])
def test_ingest_equals_the_restatement_byte_for_byte(ce, gpu_ctx, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    combos = [(p, t, d, ch, dt) for p in R.PRIMARIES for t in R.TRANSFERS for ch in (3, 4)
              for d, dt in ((8, np.uint8), (8, np.uint16), (10, np.uint16), (12, np.uint16), (16, np.uint16))]
    if w * h > 100000:  # the large shape: every primaries x transfer and every format once, not their product
        combos = [c for i, c in enumerate(combos) if i % 7 == 0]
    for prim, tr, depth, ch, dt in combos:
        px = random_codes(rng, w, h, ch, dt, depth)
        got = gpu_ctx.cicp_to_linear(px, w, h, ce.ColourDescription(prim, tr, depth, 203.0))
        want = R.to_linear(px, prim, tr, depth, 203.0)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (prim, tr, depth, ch, dt)


@pytest.mark.parametrize("w,h", [(9, 11), (17, 9), (100, 76)])
def test_ingest_into_slots_leaves_neighbours_untouched(ce, gpu_ctx, w, h):
    """Non-zero ref_index / pair_index (slot k starts k * w * h * 12 bytes in: odd shapes change the store width per slot),
    the neighbours checked untouched, and one upload between a launch and its collect."""
    rng = np.random.default_rng(5)
    n = w * h * 3
    b = gpu_ctx.batch_linear(w, h, 3, 4)
    try:
        base_r = [rng.random((h, w, 3), np.float32) for _ in range(3)]
        base_t = [rng.random((h, w, 3), np.float32) for _ in range(4)]
        for i, r in enumerate(base_r):
            b.set_reference(i, r)
        for p, t in enumerate(base_t):
            b.set_test(p, p % 3, t)
        k = 0
        for prim in R.PRIMARIES:
            for tr, depth, dt in ((16, 10, np.uint16), (13, 8, np.uint8), (8, 16, np.uint16)):
                colour = ce.ColourDescription(prim, tr, depth, 100.0)
                ri, pi = 1 + k % 2, 1 + k % 3
                k += 1
                pr, pt = random_codes(rng, w, h, 3, dt, depth), random_codes(rng, w, h, 4, dt, depth)
                b.launch(4, ce.MetricConfig.ssimulacra2_only() if min(w, h) >= 8 else ce.MetricConfig(dssim=True, ssimulacra2=False, butteraugli=False, psnr=False))
                b.set_reference_cicp(ri, pr, colour)  # between a launch and its collect: waits for the launch on the device
                b.collect(4)
                b.set_test_cicp(pi, ri, pt, colour)
                base_r[ri] = R.to_linear(pr, prim, tr, depth, 100.0)
                base_t[pi] = R.to_linear(pt, prim, tr, depth, 100.0)
                b.run(4, ce.MetricConfig(dssim=True, ssimulacra2=False, butteraugli=False, psnr=False))
                assert b.pair_reference(pi) == ri
                assert np.array_equal(read_slab(b, 0, 3 * n).view(np.uint32), np.concatenate([x.reshape(-1) for x in base_r]).view(np.uint32))
                assert np.array_equal(read_slab(b, 1, 4 * n).view(np.uint32), np.concatenate([x.reshape(-1) for x in base_t]).view(np.uint32))
    finally:
        b.close()


def test_f32_upload_sanitisation(ce, gpu_ctx):
    w, h = 23, 11
    rng = np.random.default_rng(1)
    a = (rng.random((h, w, 3), np.float32) * 6 - 2).astype(np.float32)
    a.reshape(-1)[:16] = [np.nan, np.inf, -np.inf, 1e9, -1e9, 1024.0, -1024.0, 1024.5, -0.0, 0.0, 1e-42, -1e-42, 125.0, -3.5, 1.0, 1023.99]
    a.reshape(-1)[-3:] = [np.nan, -np.inf, 2e9]  # the tail that goes sample by sample
    b = gpu_ctx.batch_linear(w, h, 2, 2)
    try:
        for slot in (0, 1):
            b.set_reference(slot, a)
            b.set_test(slot, slot, a)
        b.run(2, ce.MetricConfig(dssim=True, ssimulacra2=False, butteraugli=False, psnr=False))
        want = R.sanitise(a).reshape(-1)
        assert want[0] == 0 and want[1] == 1024 and want[2] == -1024 and want[3] == 1024 and want[4] == -1024
        for which in (0, 1):
            got = read_slab(b, which, 2 * w * h * 3)
            assert np.array_equal(got.view(np.uint32), np.concatenate([want, want]).view(np.uint32))
    finally:
        b.close()


def pq_codes(nits, white=None):
    """The 10-bit PQ code of a luminance in nits (ST 2084's inverse EOTF, rounded)."""
    y = (np.asarray(nits, np.float64) / 10000.0) ** R.PQ_M1
    return np.round(((R.PQ_C1 + R.PQ_C2 * y) / (1.0 + R.PQ_C3 * y)) ** R.PQ_M2 * 1023.0).astype(np.uint16)


def hdr_pair(kind, w, h, seed):
    """(a) BT.2020 PQ 10-bit, highlights to ~1000 nits: deep_input_shim's generators mapped from [0, max] to [0.5, 1000] nits."""
    ref, test = {"gradient_noise": D.gradient_noise_pair, "blocky": D.blocky_pair}[kind](w, h, 16, 16, seed)
    top = float(ref.max())  # the reference's brightest sample lands on 1000 nits
    to_nits = lambda v: 0.5 * (2000.0 ** (v.astype(np.float64) / top))
    return pq_codes(to_nits(ref)), pq_codes(to_nits(test))


def p3_pair(kind, w, h, seed):
    """(b) saturated Display P3, 16-bit: one channel pushed to the gamut's edge so that the converted values go negative."""
    ref, test = {"gradient_noise": D.gradient_noise_pair, "blocky": D.blocky_pair}[kind](w, h, 16, 16, seed)
    for img in (ref, test):
        img[..., 1] = img[..., 1] // 16  # little green: saturated reds, blues and magentas
        img[: h // 2, :, 2] = img[: h // 2, :, 2] // 32
    return ref, test


worst = {}


def check_parity(ce, gpu_ctx, shim, label, ref, test, w, h, intensity):
    got = gpu_ctx.eval_pair_linear(ref, test, w, h, ce.MetricConfig.all(), intensity)
    want = {"ssimulacra2": shim.ssimulacra2(ref, test, w, h, 1), "dssim": shim.dssim(ref, test, w, h),
            "butteraugli": shim.butteraugli(ref, test, w, h, intensity)[0]}
    for key, floor in FLOORS.items():
        g = getattr(got, key)
        gap = abs(g - want[key]) / max(abs(want[key]), floor)
        worst[(label, key)] = max(worst.get((label, key), 0.0), gap)
        print(f"linear parity {label} {key}: device {g!r} shim {want[key]!r} gap {gap:.3e} (worst so far {worst[(label, key)]:.3e})")
    for key, floor in FLOORS.items():
        assert abs(getattr(got, key) - want[key]) <= REL_TOL * max(abs(want[key]), floor), (label, key)
    assert got.psnr is None


@pytest.mark.parametrize("kind", ["blocky", "gradient_noise"])
def test_parity_a_bt2020_pq_highlights(ce, gpu_ctx, shim, kind):
    w, h = 160, 120
    ref, test = hdr_pair(kind, w, h, 31)
    colour = ce.ColourDescription.BT2020_PQ
    lr, lt = gpu_ctx.cicp_to_linear(ref, w, h, colour), gpu_ctx.cicp_to_linear(test, w, h, colour)
    assert lr.max() > 3.0 and np.array_equal(lr, R.to_linear(ref, 9, 16, 10, 203.0))  # ~1000 nits at a 203-nit white
    check_parity(ce, gpu_ctx, shim, f"pq_{kind}", lr, lt, w, h, 203.0)


@pytest.mark.parametrize("kind", ["blocky", "gradient_noise"])
def test_parity_b_saturated_display_p3(ce, gpu_ctx, shim, kind):
    w, h = 160, 120
    ref, test = p3_pair(kind, w, h, 32)
    colour = ce.ColourDescription(12, 13, 16)
    lr, lt = gpu_ctx.cicp_to_linear(ref, w, h, colour), gpu_ctx.cicp_to_linear(test, w, h, colour)
    assert lr.min() < -0.01 and (lr < 0).mean() > 0.05
    check_parity(ce, gpu_ctx, shim, f"p3_{kind}", lr, lt, w, h, 80.0)


@pytest.mark.parametrize("kind", ["blocky", "gradient_noise"])
def test_parity_c_plain_floats(ce, gpu_ctx, shim, kind):
    w, h = 160, 120
    ref, test = {"gradient_noise": D.gradient_noise_pair, "blocky": D.blocky_pair}[kind](w, h, 16, 16, 33)
    lr, lt = (ref.astype(np.float32) / np.float32(65535.0)) ** 2, (test.astype(np.float32) / np.float32(65535.0)) ** 2
    assert lr.dtype == np.float32
    check_parity(ce, gpu_ctx, shim, f"f32_{kind}", lr, lt, w, h, 80.0)


def test_linear_batch_sees_what_a_clamp_to_sdr_hides(ce, gpu_ctx):
    """The point of the feature: a PQ pair that differs only where the reference is above 1.0."""
    w, h = 128, 96
    y, x = np.mgrid[0:h, 0:w]
    nits = 20.0 + 150.0 * (x / (w - 1.0))  # below the 203-nit white everywhere ...
    spot = (x - 90) ** 2 + (y - 40) ** 2 < 18 ** 2
    ref_n, test_n = nits.copy(), nits.copy()
    ref_n[spot], test_n[spot] = 900.0, 600.0  # ... but for a highlight, which the test renders dimmer
    ref = np.repeat(pq_codes(ref_n)[..., None], 3, axis=-1)
    test = np.repeat(pq_codes(test_n)[..., None], 3, axis=-1)
    colour = ce.ColourDescription(1, 16, 10, 203.0)
    lr, lt = gpu_ctx.cicp_to_linear(ref, w, h, colour), gpu_ctx.cicp_to_linear(test, w, h, colour)
    assert np.array_equal(lr != lt, np.repeat(spot[..., None], 3, axis=-1)) and lr[spot].min() > 1.0 and lt[spot].min() > 1.0
    cfg = ce.MetricConfig.all()
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        b.set_reference_cicp(0, ref, colour)
        b.set_test_cicp(0, 0, test, colour)
        s = b.run(1, cfg, 203.0)[0]
        print(f"highlight pair: ssimulacra2 {s.ssimulacra2!r} dssim {s.dssim!r} butteraugli {s.butteraugli!r}")
        assert s.status == 0 and s.valid == 7 and s.ssimulacra2 < 100.0 and s.butteraugli > 0.0 and s.dssim > 0.0
        b.set_reference(0, np.clip(lr, 0.0, 1.0))
        b.set_test(0, 0, np.clip(lt, 0.0, 1.0))
        s = b.run(1, cfg, 203.0)[0]
        assert (s.ssimulacra2, s.butteraugli, s.dssim) == (100.0, 0.0, 0.0)
    finally:
        b.close()


def test_p3_bytes_read_as_p3_score_differently_from_srgb(ce, gpu_ctx, workloads):
    w, h = 96, 64
    ref = np.asarray(workloads.make_reference(w, h, 5), np.uint8).reshape(h, w, 3)
    test = np.asarray(workloads.distort(ref, 40), np.uint8).reshape(h, w, 3)
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        out = []
        for colour in (ce.ColourDescription.DISPLAY_P3, ce.ColourDescription.SRGB):
            b.set_reference_cicp(0, ref, colour)
            b.set_test_cicp(0, 0, test, colour)
            s = b.run(1, ce.MetricConfig.all())[0]
            assert s.status == 0 and s.valid == 7
            out.append((s.ssimulacra2, s.butteraugli, s.dssim))
        plain = gpu_ctx.calculate_metrics(ref, test, w, h, ce.MetricConfig.all())
        assert out[1][:2] == (plain.ssimulacra2, plain.butteraugli)
        assert all(a != c for a, c in zip(out[0], out[1]))
    finally:
        b.close()


def test_refusals_leave_the_batch_usable(ce, gpu_ctx, workloads):
    w, h = 40, 24
    ref8 = np.asarray(workloads.make_reference(w, h, 3), np.uint8).reshape(h, w, 3)
    test8 = np.asarray(workloads.distort(ref8, 50), np.uint8).reshape(h, w, 3)
    cfg = ce.MetricConfig.all()
    L = ce.lib()
    t0 = ce.srgb_table(8, 0)
    lr, lt = t0[ref8], t0[test8]

    def refused(rc):
        assert rc == ce.CE_ERR_INVALID_ARG
        assert L.ce_last_error(gpu_ctx._h).decode() != ""

    b = gpu_ctx.batch_linear(w, h, 1, 1)
    plain = ce.Batch(gpu_ctx, w, h, 1, 1)
    deep = gpu_ctx.batch_deep(w, h, 1, 1, 16, 16)
    table = None
    try:
        b.set_reference(0, lr)
        b.set_test(0, 0, lt)
        want = b.run(1, cfg)[0]
        assert want.status == 0 and want.valid == 7
        s = (ce.CeScores * 1)()
        refused(L.ce_batch_run(b._h, 1, cfg.mask, ce.FLAG_XYB_ROUNDTRIP, 80.0, s))
        refused(L.ce_batch_image_heuristics(b._h, ce.BATCH_REFERENCES, 0, 1, (ce.CeImageHeuristics * 1)()))
        table = ce.ColorTable(gpu_ctx, ce.ColorTable.identity_cube())
        refused(L.ce_batch_set_test_lut(b._h, 0, 0, lt.ctypes.data, lt.nbytes, ce.PIXEL_RGB_F32, table._h))
        refused(L.ce_batch_set_reference_lut(b._h, 0, lr.ctypes.data, lr.nbytes, ce.PIXEL_RGB_F32, table._h))
        t16 = test8.astype(np.uint16)
        rgba8 = np.concatenate([test8, np.full((h, w, 1), 200, np.uint8)], axis=-1)
        for px, fmt in ((t16, ce.PIXEL_RGB16_10BIT), (np.concatenate([t16, t16[..., :1]], axis=-1), ce.PIXEL_RGBA16_10BIT), (test8, ce.PIXEL_RGB8),
                        (rgba8, ce.PIXEL_RGBA8), (t16, ce.PIXEL_RGB16)):
            px = np.ascontiguousarray(px)
            refused(L.ce_batch_set_test_fmt(b._h, 0, 0, px.ctypes.data, px.nbytes, fmt))
            refused(L.ce_batch_set_reference_fmt(b._h, 0, px.ctypes.data, px.nbytes, fmt))
        refused(L.ce_batch_set_test(b._h, 0, 0, test8.ctypes.data, test8.nbytes))
        refused(L.ce_batch_set_reference(b._h, 0, ref8.ctypes.data, ref8.nbytes))
        refused(L.ce_batch_resample(b._h, plain._h, ce.BATCH_TESTS, 0, 1, ce.RESAMPLE_LANCZOS3))
        refused(L.ce_batch_resample(plain._h, b._h, ce.BATCH_TESTS, 0, 1, ce.RESAMPLE_LANCZOS3))
        refused(L.ce_batch_resample_pairs(b._h, plain._h, 1, 1, ce.RESAMPLE_LANCZOS3))
        bg = np.zeros(3, np.uint16)
        refs = np.zeros(1, np.uint32)
        refused(L.ce_batch_set_reference_over(b._h, 0, rgba8.ctypes.data, rgba8.nbytes, ce.PIXEL_RGBA8, 1, bg.ctypes.data))
        refused(L.ce_batch_set_test_over(b._h, 0, refs.ctypes.data, rgba8.ctypes.data, rgba8.nbytes, ce.PIXEL_RGBA8, 1, bg.ctypes.data))
        yuv = ce.YuvImage([np.ascontiguousarray(test8[..., c]) for c in range(3)], ce.YUV_444, ce.YUV_PLANAR, ce.YUV_BT601, ce.YUV_FULL,
                          ce.CHROMA_NEAREST, 8, False, ce.MEM_HOST)
        cy, _keep = yuv._c()
        refused(L.ce_batch_set_reference_yuv(b._h, 0, C.byref(cy)))
        refused(L.ce_batch_set_test_yuv(b._h, 0, 0, C.byref(cy)))
        # CE_PIXEL_RGB_F32 and the CICP route on batches that are not linear
        for other in (plain, deep):
            refused(L.ce_batch_set_test_fmt(other._h, 0, 0, lt.ctypes.data, lt.nbytes, ce.PIXEL_RGB_F32))
            col = ce.ColourDescription.SRGB._c()
            refused(L.ce_batch_set_test_cicp(other._h, 0, 0, test8.ctypes.data, test8.nbytes, ce.PIXEL_RGB8, C.byref(col)))
            refused(L.ce_batch_set_reference_cicp(other._h, 0, test8.ctypes.data, test8.nbytes, ce.PIXEL_RGB8, C.byref(col)))
        # the CICP route's own argument checks
        for col, px, fmt in ((ce.CeColour(2, 13, 8, 0.0), test8, ce.PIXEL_RGB8), (ce.CeColour(1, 18, 10, 203.0), t16, ce.PIXEL_RGB16),
                             (ce.CeColour(1, 1, 10, 0.0), t16, ce.PIXEL_RGB16), (ce.CeColour(1, 13, 9, 0.0), t16, ce.PIXEL_RGB16),
                             (ce.CeColour(1, 13, 10, 0.0), test8, ce.PIXEL_RGB8), (ce.CeColour(9, 16, 10, 0.0), t16, ce.PIXEL_RGB16),
                             (ce.CeColour(9, 16, 10, -5.0), t16, ce.PIXEL_RGB16), (ce.CeColour(1, 13, 16, 0.0), t16, ce.PIXEL_RGB16_10BIT),
                             (ce.CeColour(1, 13, 8, 0.0), lt, ce.PIXEL_RGB_F32)):
            refused(L.ce_batch_set_test_cicp(b._h, 0, 0, px.ctypes.data, px.nbytes, fmt, C.byref(col)))
        col = ce.CeColour(1, 13, 8, 0.0)
        assert L.ce_batch_set_test_cicp(b._h, 0, 0, test8.ctypes.data, test8.nbytes - 3, ce.PIXEL_RGB8, C.byref(col)) == ce.CE_ERR_BAD_LENGTH
        refused(L.ce_eval_pair_linear(gpu_ctx._h, lr.ctypes.data, lr.nbytes, lt.ctypes.data, lt.nbytes, w, h, cfg.mask, ce.FLAG_XYB_ROUNDTRIP, 80.0, s))
        refused(L.ce_eval_pair_linear(gpu_ctx._h, lr.ctypes.data, lr.nbytes, lt.ctypes.data, lt.nbytes, w, h, cfg.mask, ce.FLAG_SSIMULACRA2_MAPS, 80.0, s))
        assert L.ce_eval_pair_linear(gpu_ctx._h, lr.ctypes.data, lr.nbytes, lt.ctypes.data, lt.nbytes - 12, w, h, cfg.mask, 0, 80.0, s) == ce.CE_ERR_DIM_MISMATCH
        assert L.ce_eval_pair_linear(gpu_ctx._h, lr.ctypes.data, lr.nbytes - 12, lt.ctypes.data, lt.nbytes - 12, w, h, cfg.mask, 0, 80.0, s) == ce.CE_ERR_BAD_LENGTH
        # a null table is no table; and after all of the above the batch still scores what it scored
        b.set_test_lut(0, 0, lt, ce.PIXEL_RGB_F32, None)
        again = b.run(1, cfg)[0]
        assert (again.dssim, again.ssimulacra2, again.butteraugli, again.valid, again.status) == \
               (want.dssim, want.ssimulacra2, want.butteraugli, want.valid, want.status)
    finally:
        if table is not None:
            table.close()
        for x in (b, plain, deep):
            x.close()


def test_session_scores_a_tagged_decode_through_a_linear_batch(ce, gpu_ctx, workloads, tmp_path):
    S = importlib.import_module("codec-eval_amd.session")
    w, h = 64, 48
    ref8 = np.asarray(workloads.make_reference(w, h, 4), np.uint8).reshape(h, w, 3)
    test8 = np.asarray(workloads.distort(ref8, 55), np.uint8).reshape(h, w, 3)
    rng = np.random.default_rng(2)
    decode10 = np.clip(test8.astype(np.int32) * 3 + rng.integers(0, 4, test8.shape), 0, 1023).astype(np.uint16)
    lin = (ce.srgb_table(8, 0)[test8] * np.float32(1.5)).astype(np.float32)
    cfg = S.EvalConfig.builder().report_dir(str(tmp_path)).metrics(ce.MetricConfig.all()).quality_levels([50.0]).build()
    sess = S.EvalSession(cfg, ctx=gpu_ctx)
    enc = lambda img, req: b"x"
    sess.add_codec_with_decode("pq", "1", enc, lambda data: S.ImageData.rgb16(decode10, w, h, 10, colour=ce.ColourDescription.BT2020_PQ))
    sess.add_codec_with_decode("f32", "1", enc, lambda data: S.ImageData.linear_f32(lin, w, h))
    sess.add_codec_with_decode("flat", "1", enc, lambda data: S.ImageData.rgb(test8, w, h))
    sess.add_codec_with_decode("srgb", "1", enc, lambda data: S.ImageData.rgb(test8, w, h, colour=ce.ColourDescription.SRGB))
    report = sess.evaluate_image("img", S.ImageData.rgb(ref8, w, h))
    rows = {r.codec_id: r for r in report.results}
    b = gpu_ctx.batch_linear(w, h, 1, 2)
    try:
        b.set_reference_cicp(0, ref8, ce.ColourDescription.SRGB)
        b.set_test_cicp(0, 0, decode10, ce.ColourDescription.BT2020_PQ)
        b.set_test(1, 0, lin)
        want = [ce.MetricResult.from_c(s) for s in b.run(2, ce.MetricConfig.all())]
    finally:
        b.close()
    for key, m in (("pq", want[0]), ("f32", want[1])):
        d = rows[key]
        assert (d.dssim, d.ssimulacra2, d.butteraugli, d.psnr) == (m.dssim, m.ssimulacra2, m.butteraugli, None)
    today = gpu_ctx.calculate_metrics(ref8, test8, w, h, ce.MetricConfig.all())
    for key in ("flat", "srgb"):  # untagged, or tagged as what it always was: every path and score as before
        f = rows[key]
        assert (f.dssim, f.ssimulacra2, f.butteraugli, f.psnr) == (today.dssim, today.ssimulacra2, today.butteraugli, today.psnr)
    # a colour description together with an ICC profile, or with alpha under alpha_backgrounds: refused
    tagged = S.ImageData.rgb16(decode10, w, h, 10, colour=ce.ColourDescription.BT2020_PQ)
    tagged.icc_profile = b"profile"
    bad = S.EvalSession(cfg, ctx=gpu_ctx)
    bad.add_codec_with_decode("both", "1", enc, lambda data: tagged)
    with pytest.raises(ce.MetricCalculation):
        bad.evaluate_image("img", S.ImageData.rgb(ref8, w, h))
    cfg_a = S.EvalConfig.builder().report_dir(str(tmp_path)).metrics(ce.MetricConfig.all()).quality_levels([50.0]).alpha_backgrounds(ce.ALPHA_BLACK_WHITE).build()
    rgba = np.concatenate([decode10, np.full((h, w, 1), 512, np.uint16)], axis=-1)
    bad = S.EvalSession(cfg_a, ctx=gpu_ctx)
    bad.add_codec_with_decode("alpha", "1", enc, lambda data: S.ImageData.rgba16(rgba, w, h, 10, colour=ce.ColourDescription.BT2020_PQ))
    with pytest.raises(ce.MetricCalculation):
        bad.evaluate_image("img", S.ImageData.rgb(ref8, w, h))
