"""Deep input on the device (ce_batch_create_deep and friends), through the C ABI.

The two anchors are EXACT: a deep batch of depths 8 / 8 uses the RGB8 path's table entries, and a depth-16 image holding
v8 * 257 is the same image as the 8-bit one (tests/test_deep_input_cpu.py checks the tables), so every score and every map
is compared with == / array_equal.  Real deep content is held against tests/deep_input_shim.py (the oracle's own stages
behind a 2^depth-entry table) with tests/test_gpu_parity.py's bound.
"""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import deep_input_shim as D
from test_deep_input_cpu import below_8bit_step_pair

pytestmark = pytest.mark.gpu

REL_TOL = 1e-4  # tests/test_gpu_parity.py
FLOORS = {"ssimulacra2": 1.0, "dssim": 1e-6, "butteraugli": 1e-3}  # that file's floors (Butteraugli: tests/test_gpu_butteraugli.py's)


@pytest.fixture(scope="module")
def shim(tmp_path_factory, oracle):
    return D.Shim(tmp_path_factory.mktemp("deep_input_shim"))


def rgb8_pair(workloads, w, h, seed, q=55):
    ref = workloads.make_reference(w, h, seed)
    return np.asarray(ref, np.uint8).reshape(h, w, 3), np.asarray(workloads.distort(ref, q), np.uint8).reshape(h, w, 3)


def run_everything(ce, batch, n_pairs, w, h):
    """All four scores, the 3-norm, and every map of a launch: a dict of comparable things."""
    scores = batch.run(n_pairs, ce.MetricConfig.all(), butteraugli_diffmap=True, ssimulacra2_maps=True)
    out = {"scores": [(s.dssim, s.ssimulacra2, s.butteraugli, s.psnr, s.valid, s.status) for s in scores],
           "pnorm3": batch.butteraugli_pnorm3(n_pairs)}
    if w >= 8 and h >= 8:
        out["diffmap"] = batch.butteraugli_diffmaps(0, n_pairs)
        out["diffmap_b8"] = batch.butteraugli_diffmaps(0, n_pairs, block=8)
        for s in range(len(ce.ssimulacra2_scales(w, h))):
            for c in range(3):
                for k in range(3):
                    out[f"s2_{s}_{c}_{k}"] = batch.ssimulacra2_maps(s, c, k, 0, n_pairs)
    for lvl in range(len(ce.dssim_levels(w, h))):
        out[f"ds_{lvl}"] = batch.dssim_ssim_maps(lvl, 0, n_pairs)
    return out


def same(a, b, skip_psnr=False):
    """== on every double, array_equal on every map."""
    assert a.keys() == b.keys()
    for k in a:
        if k == "scores":
            for x, y in zip(a[k], b[k]):
                x, y = list(x), list(y)
                if skip_psnr:
                    x[3] = y[3] = 0.0
                    x[4] &= ~8
                    y[4] &= ~8
                assert x == y, (k, x, y)
        elif isinstance(a[k], tuple):
            for x, y in zip(a[k], b[k]):
                assert np.array_equal(np.asarray(x), np.asarray(y)), k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def fill(batch, refs, tests, pair_ref):
    for i, r in enumerate(refs):
        batch.set_reference(i, r)
    for p, (t, ri) in enumerate(zip(tests, pair_ref)):
        batch.set_test(p, ri, t)


def grid(workloads, w, h, n_refs, n_pairs, seed):
    refs, tests, pair_ref = [], [], []
    for i in range(n_refs):
        refs.append(rgb8_pair(workloads, w, h, seed + i)[0])
    for p in range(n_pairs):
        ri = p % n_refs
        tests.append(np.asarray(workloads.distort(refs[ri], min(30 + 7 * p, 95)), np.uint8).reshape(h, w, 3))
        pair_ref.append(ri)
    return refs, tests, pair_ref


SHAPES = [(37, 29, 1, 1), (12, 10, 1, 2), (768, 512, 1, 2), (96, 64, 3, 9)]  # odd, under 16 x 16, Kodak, multi-reference


@pytest.mark.parametrize("w,h,n_refs,n_pairs", SHAPES)
def test_anchor1_depth_8_8_equals_the_rgb8_batch(ce, gpu_ctx, workloads, w, h, n_refs, n_pairs):
    refs, tests, pair_ref = grid(workloads, w, h, n_refs, n_pairs, 11)
    plain = ce.Batch(gpu_ctx, w, h, n_refs, n_pairs)
    deep = gpu_ctx.batch_deep(w, h, n_refs, n_pairs, 8, 8)
    try:
        fill(plain, refs, tests, pair_ref)
        want = run_everything(ce, plain, n_pairs, w, h)
        fill(deep, refs, tests, pair_ref)  # RGB8 pixels, widened on the device
        same(run_everything(ce, deep, n_pairs, w, h), want)
        fill(deep, [r.astype(np.uint16) for r in refs], [t.astype(np.uint16) for t in tests], pair_ref)  # the same as u16
        same(run_everything(ce, deep, n_pairs, w, h), want)
    finally:
        plain.close()
        deep.close()


@pytest.mark.parametrize("w,h,n_refs,n_pairs", SHAPES)
def test_anchor2_depth16_v8_times_257_equals_the_rgb8_batch(ce, gpu_ctx, workloads, shim, w, h, n_refs, n_pairs):
    refs, tests, pair_ref = grid(workloads, w, h, n_refs, n_pairs, 23)
    refs16 = [r.astype(np.uint16) * 257 for r in refs]
    tests16 = [t.astype(np.uint16) * 257 for t in tests]
    plain = ce.Batch(gpu_ctx, w, h, n_refs, n_pairs)
    d1616 = gpu_ctx.batch_deep(w, h, n_refs, n_pairs, 16, 16)
    d816 = gpu_ctx.batch_deep(w, h, n_refs, n_pairs, 8, 16)
    try:
        fill(plain, refs, tests, pair_ref)
        want = run_everything(ce, plain, n_pairs, w, h)
        fill(d1616, refs16, tests16, pair_ref)
        got = run_everything(ce, d1616, n_pairs, w, h)
        same(got, want, skip_psnr=True)
        # PSNR: the f64 expression on the host from the exact integer SSE, == (the same libm as the library's host side)
        for p, s in enumerate(got["scores"]):
            host = D.psnr_from_sse(shim.sse(refs16[pair_ref[p]], tests16[p]), w, h, 16)
            print(f"psnr 16/16 {w}x{h} pair {p}: device {s[3]!r} host {host!r}")
            assert s[3] == host and (s[4] & 8)
        fill(d816, refs, tests16, pair_ref)
        mixed = run_everything(ce, d816, n_pairs, w, h)
        same(mixed, want, skip_psnr=True)
        assert all((s[4] & 8) == 0 and s[5] == 0 for s in mixed["scores"])  # unequal depths: no PSNR, the rest runs
    finally:
        plain.close()
        d1616.close()
        d816.close()


PAIRS = {"random": D.random_pair, "gradient_noise": D.gradient_noise_pair, "blocky": D.blocky_pair}
worst = {}


@pytest.mark.parametrize("rd,td", [(10, 10), (12, 12), (16, 16), (8, 10)])
@pytest.mark.parametrize("kind", sorted(PAIRS))
def test_parity_on_deep_content(ce, gpu_ctx, shim, kind, rd, td):
    w, h = 160, 120
    ref, test = PAIRS[kind](w, h, rd, td, 100 + rd + td)
    got = gpu_ctx.eval_pair_deep(ref, rd, test, td, w, h, ce.MetricConfig.all())
    want = {"ssimulacra2": shim.ssimulacra2(ref, rd, test, td, w, h, 1), "dssim": shim.dssim(ref, rd, test, td, w, h),
            "butteraugli": shim.butteraugli(ref, rd, test, td, w, h)[0]}
    for key, floor in FLOORS.items():
        g = getattr(got, key)
        gap = abs(g - want[key]) / max(abs(want[key]), floor)
        worst[key] = max(worst.get(key, 0.0), gap)
        print(f"deep parity {kind} {rd}/{td} {key}: device {g!r} shim {want[key]!r} gap {gap:.3e} (worst so far {worst[key]:.3e})")
    for key, floor in FLOORS.items():
        assert abs(getattr(got, key) - want[key]) <= REL_TOL * max(abs(want[key]), floor), (kind, rd, td, key)
    if rd == td:
        assert got.psnr == D.psnr_from_sse(shim.sse(ref, test), w, h, rd)
    else:
        assert got.psnr is None


def test_deep_batch_sees_what_to_8bit_hides(ce, gpu_ctx, shim):
    """The point of the feature.  A 10-bit pair that differs only where to_8bit maps both sides to the same byte: identical
    through CE_PIXEL_RGB16_10BIT (existing behaviour), different through a deep batch."""
    w, h = 128, 96
    ref, test, changed = below_8bit_step_pair(w, h)
    assert changed >= 0.25
    cfg = ce.MetricConfig.all()
    plain = ce.Batch(gpu_ctx, w, h, 1, 1)
    deep = gpu_ctx.batch_deep(w, h, 1, 1, 10, 10)
    try:
        plain.set_reference_fmt(0, ref, ce.PIXEL_RGB16_10BIT)
        plain.set_test_fmt(0, 0, test, ce.PIXEL_RGB16_10BIT)
        s = plain.run(1, cfg)[0]
        assert s.status == 0 and math.isinf(s.psnr) and s.ssimulacra2 == 100.0 and s.dssim == 0.0 and s.butteraugli == 0.0
        deep.set_reference(0, ref)
        deep.set_test(0, 0, test)
        s = deep.run(1, cfg)[0]
        host = D.psnr_from_sse(shim.sse(ref, test), w, h, 10)
        print(f"below the 8-bit step: psnr {s.psnr!r} (host {host!r}) ssimulacra2 {s.ssimulacra2!r} dssim {s.dssim!r} butteraugli {s.butteraugli!r}")
        assert s.status == 0 and s.valid == 15
        assert math.isfinite(s.psnr) and s.psnr == host
        assert s.dssim > 0.0 and s.butteraugli > 0.0 and s.ssimulacra2 < 100.0
    finally:
        plain.close()
        deep.close()


def hip_runtime():
    """The HIP runtime the library itself is linked against (already loaded in this process)."""
    import os

    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def test_clamping_alpha_and_in_place_slab_writes(ce, gpu_ctx):
    w, h = 50, 34
    rng = np.random.default_rng(9)
    ref = rng.integers(0, 1024, (h, w, 3)).astype(np.uint16)
    test = np.clip(ref.astype(np.int32) + rng.integers(-40, 41, ref.shape), 0, 1023).astype(np.uint16)
    test[::3, ::5] = 1023
    cfg = ce.MetricConfig.all()
    b = gpu_ctx.batch_deep(w, h, 1, 1, 10, 10)
    try:
        def score():
            s = b.run(1, cfg)[0]
            assert s.status == 0
            return (s.dssim, s.ssimulacra2, s.butteraugli, s.psnr, s.valid)

        b.set_reference(0, ref)
        b.set_test(0, 0, test)
        want = score()
        over = test.copy()
        over[test == 1023] = 65535
        over[1::3, 2::5][test[1::3, 2::5] == 1023] = 1024
        b.set_test(0, 0, over)  # samples above 2^d - 1 score as 2^d - 1
        assert score() == want
        rgba = np.concatenate([test, rng.integers(0, 65536, (h, w, 1)).astype(np.uint16)], axis=-1)
        b.set_test(0, 0, rgba)  # RGBA16: alpha dropped
        assert score() == want
        b.set_reference(0, np.concatenate([ref, np.zeros((h, w, 1), np.uint16)], axis=-1))
        assert score() == want
        # in place: the u16 slab written by the caller, then bound
        b.set_test(0, 0, np.zeros_like(test))
        gpu_ctx.synchronize()
        b.run(1, cfg)
        assert hip_runtime().hipMemcpy(b.test_slab, test.ctypes.data, test.nbytes, 1) == 0  # host to device, blocking
        b.bind_pair(0, 0)
        assert score() == want
    finally:
        b.close()


def test_refusals_leave_the_batch_usable(ce, gpu_ctx, workloads):
    w, h = 40, 24
    ref8, test8 = rgb8_pair(workloads, w, h, 3)
    cfg = ce.MetricConfig.all()
    L = ce.lib()

    def refused(rc):
        assert rc == ce.CE_ERR_INVALID_ARG
        assert L.ce_last_error(gpu_ctx._h).decode() != ""

    out = C.c_void_p()
    for rd, td in ((9, 10), (10, 0), (16, 32), (7, 7)):
        refused(L.ce_batch_create_deep(gpu_ctx._h, w, h, 1, 1, rd, td, C.byref(out)))
        assert not out.value
    b = gpu_ctx.batch_deep(w, h, 1, 1, 8, 10)
    table = None
    try:
        ref16 = ref8.astype(np.uint16)
        test10 = (test8.astype(np.uint16) * 4)
        b.set_reference(0, ref8)
        b.set_test(0, 0, test10)
        want = b.run(1, cfg)[0]
        assert want.status == 0 and want.valid == 7
        s = (ce.CeScores * 1)()
        refused(L.ce_batch_run(b._h, 1, cfg.mask, ce.FLAG_XYB_ROUNDTRIP, 80.0, s))
        h_out = (ce.CeImageHeuristics * 1)()
        refused(L.ce_batch_image_heuristics(b._h, ce.BATCH_REFERENCES, 0, 1, h_out))
        table = ce.ColorTable(gpu_ctx, ce.ColorTable.identity_cube())
        refused(L.ce_batch_set_test_lut(b._h, 0, 0, test10.ctypes.data, test10.nbytes, ce.PIXEL_RGB16, table._h))
        refused(L.ce_batch_set_reference_lut(b._h, 0, ref16.ctypes.data, ref16.nbytes, ce.PIXEL_RGB16, table._h))
        refused(L.ce_batch_set_test_fmt(b._h, 0, 0, test10.ctypes.data, test10.nbytes, ce.PIXEL_RGB16_10BIT))
        refused(L.ce_batch_set_test_fmt(b._h, 0, 0, test8.ctypes.data, test8.nbytes, ce.PIXEL_RGB8))  # the test side is 10-bit
        plain = ce.Batch(gpu_ctx, w, h, 1, 1)
        try:
            refused(L.ce_batch_set_test_fmt(plain._h, 0, 0, test10.ctypes.data, test10.nbytes, ce.PIXEL_RGB16))
        finally:
            plain.close()
        refused(L.ce_eval_pair_deep(gpu_ctx._h, ref16.ctypes.data, ref16.nbytes, 8, test10.ctypes.data, test10.nbytes, 11, w, h,
                                    cfg.mask, 0, 80.0, s))
        refused(L.ce_eval_pair_deep(gpu_ctx._h, ref16.ctypes.data, ref16.nbytes, 8, test10.ctypes.data, test10.nbytes, 10, w, h,
                                    cfg.mask, ce.FLAG_XYB_ROUNDTRIP, 80.0, s))
        assert L.ce_eval_pair_deep(gpu_ctx._h, ref16.ctypes.data, ref16.nbytes, 8, test10.ctypes.data, test10.nbytes - 6, 10, w, h,
                                   cfg.mask, 0, 80.0, s) == ce.CE_ERR_DIM_MISMATCH
        assert L.ce_eval_pair_deep(gpu_ctx._h, ref16.ctypes.data, ref16.nbytes - 6, 8, test10.ctypes.data, test10.nbytes - 6, 10, w, h,
                                   cfg.mask, 0, 80.0, s) == ce.CE_ERR_BAD_LENGTH
        # a null table is no table; and after all of the above the batch still scores what it scored
        b.set_test_lut(0, 0, test10, ce.PIXEL_RGB16, None)
        again = b.run(1, cfg)[0]
        assert (again.dssim, again.ssimulacra2, again.butteraugli, again.valid, again.status) == \
               (want.dssim, want.ssimulacra2, want.butteraugli, want.valid, want.status)
        leaf = gpu_ctx.eval_pair_deep(ref16, 8, test10, 10, w, h, cfg)
        assert (leaf.dssim, leaf.ssimulacra2, leaf.butteraugli, leaf.psnr) == (want.dssim, want.ssimulacra2, want.butteraugli, None)
    finally:
        if table is not None:
            table.close()
        b.close()


def test_session_scores_a_deep_decode_through_a_deep_batch(ce, gpu_ctx, workloads, tmp_path):
    S = importlib.import_module("codec-eval_amd.session")
    w, h = 64, 48
    ref8, test8 = rgb8_pair(workloads, w, h, 4)
    rng = np.random.default_rng(2)
    decode10 = np.clip(test8.astype(np.int32) * 4 + rng.integers(0, 4, test8.shape), 0, 1023).astype(np.uint16)
    cfg = S.EvalConfig.builder().report_dir(str(tmp_path)).metrics(ce.MetricConfig.all()).quality_levels([50.0]).build()
    sess = S.EvalSession(cfg, ctx=gpu_ctx)
    sess.add_codec_with_decode("deep", "1", lambda img, req: b"x", lambda data: S.ImageData.rgb16(decode10, w, h, 10))
    sess.add_codec_with_decode("flat", "1", lambda img, req: b"x", lambda data: S.ImageData.rgb(test8, w, h))
    report = sess.evaluate_image("img", S.ImageData.rgb(ref8, w, h))
    rows = {r.codec_id: r for r in report.results}
    b = gpu_ctx.batch_deep(w, h, 1, 1, 8, 10)
    try:
        b.set_reference(0, ref8)
        b.set_test(0, 0, decode10)
        want = ce.MetricResult.from_c(b.run(1, ce.MetricConfig.all())[0])
    finally:
        b.close()
    d = rows["deep"]
    assert (d.dssim, d.ssimulacra2, d.butteraugli, d.psnr) == (want.dssim, want.ssimulacra2, want.butteraugli, None)
    today = gpu_ctx.calculate_metrics(ref8, test8, w, h, ce.MetricConfig.all())
    f = rows["flat"]
    assert (f.dssim, f.ssimulacra2, f.butteraugli, f.psnr) == (today.dssim, today.ssimulacra2, today.butteraugli, today.psnr)
