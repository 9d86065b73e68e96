"""Matrix/TRC ICC profiles applied on the device (include/ce_metrics.h: ce_icc_*, ce_batch_set_*_icc).
The definition - host-built tone tables, the separately rounded f32 matrix, the clamp of a linear image and, for integer
slots, the search of the sRGB code thresholds - is restated in numpy (tests/icc_restatement.py); the device must equal it on
every byte of every slot of every batch kind, the scores of what it wrote must equal those of the same samples taken in by
the existing routes, and a session without a cms must apply such profiles by itself."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

S = importlib.import_module("codec-eval_amd.session")
F = R.fixtures()
SHAPES = ((1, 1), (3, 5), (7, 2), (16, 1), (17, 9), (100, 76), (768, 512))
# sample type, channels and source depths of the four formats
FORMATS = ((np.uint8, 3, (8,)), (np.uint8, 4, (8,)), (np.uint16, 3, R.DEPTHS), (np.uint16, 4, R.DEPTHS))
PROFILES = ("p3", "srgb_curv1024", "mixed_curv", "adobe", "mixed_para", "srgb_para", "prophoto", "p3_gamma22")


def read_slab(ce, address, nbytes):
    """Device bytes -> host after everything queued on the device (the slot writes run on the batch's upload stream)."""
    assert ce.lib().hipDeviceSynchronize() == 0
    out = np.empty(nbytes, np.uint8)
    assert ce.lib().hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(address), C.c_size_t(nbytes), 2) == 0
    return out


def random_codes(rng, w, h, channels, dt, depth):
    maxv = (1 << depth) - 1
    px = rng.integers(0, maxv + 1, (h, w, channels)).astype(dt)
    if dt == np.uint16 and depth < 16:
        px[rng.random(px.shape) < 0.05] = dt(min(65535, maxv + 1 + int(rng.integers(0, 1000))))  # above maxv: clamped
    return px


def scores_tuple(s):
    return (s.status, s.valid, s.dssim, s.ssimulacra2, s.butteraugli, s.psnr)


@pytest.fixture(scope="module")
def profiles(ce, gpu_ctx):
    made = {name: ce.IccProfile(gpu_ctx, F[name]) for name in PROFILES}
    yield made
    for p in made.values():
        p.close()


@pytest.fixture(scope="module")
def p3_cube(ce):
    """The restatement of the P3 profile on all 2^24 colours, in ColorTable's order: computed once, never written to."""
    cube = ce.ColorTable.identity_cube()
    out = R.to_srgb(cube, F["p3"], 8, 8)
    out.setflags(write=False)
    return cube, out


def batches_of(ce, ctx, w, h):
    """(kind, batch, slot's depth per slab (0: linear), sample type) for the three batch kinds, every deep depth on both slabs"""
    out = [("linear", ctx.batch_linear(w, h, 3, 3), (0, 0), np.float32), ("rgb8", ce.Batch(ctx, w, h, 3, 3), (8, 8), np.uint8)]
    for depths in ((8, 16), (10, 12), (16, 8), (12, 10)):
        out.append(("deep", ctx.batch_deep(w, h, 3, 3, *depths), depths, np.uint16))
    return out


@pytest.mark.parametrize("w,h", SHAPES)
def test_slab_bytes_equal_the_restatement(ce, gpu_ctx, profiles, w, h):
    """Every format x source depth - at 768x512 every format once in each batch, at one source depth - walking through slots
    0, 1 and 2 of both slabs of a linear, an RGB8 and four deep batches (odd shapes change the store width with the slot); the
    other slots are checked untouched, and the leaf call of the same conversion returns the slot's samples."""
    rng = np.random.default_rng(w * 1000 + h)
    big = w * h > 100000
    k = 0
    for bi, (kind, b, slot_depths, sample) in enumerate(batches_of(ce, gpu_ctx, w, h)):
        try:
            nbytes = w * h * 3 * np.dtype(sample).itemsize
            if kind == "linear":
                slabs = [[rng.random((h, w, 3), np.float32) for _ in range(3)] for _ in range(2)]
            else:
                slabs = [[rng.integers(0, 1 << slot_depths[s], (h, w, 3)).astype(sample) for _ in range(3)] for s in range(2)]
            for i in range(3):
                b.set_reference(i, slabs[0][i])
                b.set_test(i, i, slabs[1][i])
            for fi, (dt, ch, depths) in enumerate(FORMATS):
                if kind == "rgb8" and dt == np.uint16:
                    continue  # refused: see test_refusals
                if big:  # the large shape: every format the batch takes once in each of the six batches, the source depth walking
                    depths = (depths[(bi + fi) % len(depths)],)
                for depth in depths:
                    k += 1
                    slot, which, name = k % 3, (k // 3) % 2, PROFILES[k % len(PROFILES)]
                    px = random_codes(rng, w, h, ch, dt, depth)
                    D = slot_depths[which]
                    if kind == "linear":
                        want = R.to_linear(px, F[name], depth)
                        leaf = gpu_ctx.icc_to_linear(px, w, h, depth, profiles[name])
                    else:
                        want = R.to_srgb(px, F[name], depth, D, out16=kind == "deep")
                        leaf = gpu_ctx.icc_to_srgb(px, w, h, depth, profiles[name], depth_out=D) if (kind == "rgb8" or D != 8) else None
                    if which == 0:
                        b.set_reference_icc(slot, px, depth, profiles[name])
                    else:
                        b.set_test_icc(slot, (slot + 1) % 3, px, depth, profiles[name])
                        assert b.pair_reference(slot) == (slot + 1) % 3
                    slabs[which][slot] = want
                    where = (kind, slot_depths, dt.__name__, ch, depth, name, slot, which)
                    if leaf is not None:
                        assert leaf.dtype == want.dtype and np.array_equal(leaf.view(np.uint8), want.view(np.uint8)), where
                    for s, address in ((0, b.reference_slab), (1, b.test_slab)):
                        got = read_slab(ce, address, 3 * nbytes)
                        assert np.array_equal(got, np.concatenate([np.ascontiguousarray(x).reshape(-1).view(np.uint8) for x in slabs[s]])), (where, s)
        finally:
            b.close()


def test_srgb16_leaf_at_depth_8_is_the_u8_leaf(ce, gpu_ctx, profiles):
    """ce_icc_to_srgb16 with depth_out = 8 (a deep side of depth 8): the codes of ce_icc_to_srgb8 in u16 samples."""
    rng = np.random.default_rng(8)
    px = random_codes(rng, 33, 7, 3, np.uint16, 12)
    out16 = np.empty((7, 33, 3), np.uint16)
    gpu_ctx._check(ce.lib().ce_icc_to_srgb16(gpu_ctx._h, px.ctypes.data, px.nbytes, ce.PIXEL_RGB16, 12, profiles["adobe"]._h, 33, 7, 8,
                                             out16.ctypes.data, out16.size))
    out8 = gpu_ctx.icc_to_srgb(px, 33, 7, 12, profiles["adobe"])
    assert out8.dtype == np.uint8 and np.array_equal(out16, out8) and np.array_equal(out8, R.to_srgb(px, F["adobe"], 12, 8))


def test_the_whole_colour_cube_through_the_p3_profile(ce, gpu_ctx, profiles, p3_cube):
    cube, want = p3_cube
    got = gpu_ctx.icc_to_srgb(cube.reshape(4096, 4096, 3), 4096, 4096, 8, profiles["p3"])
    assert np.array_equal(got.reshape(-1, 3), want)
    assert (want != cube).any(axis=1).mean() > 0.9  # the transform moves nearly every colour


def test_rgb8_scores_equal_those_of_the_restated_bytes_and_of_the_table_route(ce, gpu_ctx, workloads, profiles, p3_cube):
    """set_*_icc, set_* with the restated bytes, and set_*_lut with a table built from the restatement on the identity cube fill
    a slot with the same bytes: == on every score."""
    w, h = 96, 80
    src = workloads.make_reference(w, h, 11)
    decs = [workloads.distort(src, q) for q in (40, 85)]
    rgba = np.concatenate([decs[1], np.full((h, w, 1), 7, np.uint8)], axis=-1)
    lut = ce.ColorTable(gpu_ctx, p3_cube[1])
    got = []
    for route in ("icc", "bytes", "lut"):
        b = ce.Batch(gpu_ctx, w, h, 1, 3)
        try:
            if route == "icc":
                b.set_reference_icc(0, src, 8, profiles["p3"])
                b.set_test_icc(0, 0, decs[0], 8, profiles["p3"])
                b.set_test_icc(1, 0, decs[1], 8, profiles["p3"])
                b.set_test_icc(2, 0, rgba, 8, profiles["p3"])
            elif route == "bytes":
                b.set_reference(0, R.to_srgb(src, F["p3"], 8))
                for i, d in enumerate((decs[0], decs[1], rgba)):
                    b.set_test(i, 0, R.to_srgb(d, F["p3"], 8))
            else:
                b.set_reference_lut(0, src, ce.PIXEL_RGB8, lut)
                b.set_test_lut(0, 0, decs[0], ce.PIXEL_RGB8, lut)
                b.set_test_lut(1, 0, decs[1], ce.PIXEL_RGB8, lut)
                b.set_test_lut(2, 0, rgba, ce.PIXEL_RGBA8, lut)
            got.append([scores_tuple(s) for s in b.run(3, ce.MetricConfig.all())])
        finally:
            b.close()
    lut.close()
    assert got[0] == got[1] == got[2]
    assert all(s[0] == 0 and s[1] == 15 for s in got[0]) and got[0][0] != got[0][1] and got[0][1] == got[0][2]


def test_linear_scores_equal_those_of_the_restated_floats(ce, gpu_ctx, workloads, profiles):
    w, h = 96, 80
    rng = np.random.default_rng(3)
    src = random_codes(rng, w, h, 3, np.uint16, 10)
    dec = np.minimum(src + rng.integers(0, 9, src.shape).astype(np.uint16), 1023).astype(np.uint16)
    got = []
    for restated in (False, True):
        b = gpu_ctx.batch_linear(w, h, 1, 1)
        try:
            if restated:
                b.set_reference_fmt(0, R.to_linear(src, F["prophoto"], 10), ce.PIXEL_RGB_F32)
                b.set_test_fmt(0, 0, R.to_linear(dec, F["prophoto"], 10), ce.PIXEL_RGB_F32)
            else:
                b.set_reference_icc(0, src, 10, profiles["prophoto"])
                b.set_test_icc(0, 0, dec, 10, profiles["prophoto"])
            got.append([scores_tuple(s) for s in b.run(1, ce.MetricConfig.all())])
        finally:
            b.close()
    assert got[0] == got[1] and got[0][0][0] == 0 and got[0][0][3] < 100.0


def test_a_difference_outside_the_srgb_gamut_shows_in_linear_light_only(ce, gpu_ctx, profiles):
    """Saturated P3 greens whose red differs: both land on the same sRGB codes (red clips at 0), so the RGB8 route scores the
    pair identical; their linear values differ below zero, and the linear route scores that."""
    w, h = 64, 64
    rng = np.random.default_rng(12)
    a = np.stack([rng.integers(0, 24, (h, w)), rng.integers(200, 256, (h, w)), rng.integers(0, 24, (h, w))], axis=-1).astype(np.uint8)
    bb = a.copy()
    bb[..., 0] = rng.integers(0, 24, (h, w))
    same_codes = (R.to_srgb(a, F["p3"], 8) == R.to_srgb(bb, F["p3"], 8)).all(axis=-1)
    bb[~same_codes] = a[~same_codes]
    differ = (a != bb).any(axis=-1)
    assert differ.sum() > w * h // 2 and np.array_equal(R.to_srgb(a, F["p3"], 8), R.to_srgb(bb, F["p3"], 8))
    la, lb = R.to_linear(a, F["p3"], 8), R.to_linear(bb, F["p3"], 8)
    assert (la[differ] != lb[differ]).any(axis=-1).all() and la[..., 0].max() < 0.0
    b8, lin = ce.Batch(gpu_ctx, w, h, 1, 1), gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        for b in (b8, lin):
            b.set_reference_icc(0, a, 8, profiles["p3"])
            b.set_test_icc(0, 0, bb, 8, profiles["p3"])
        s8, sl = b8.run(1, ce.MetricConfig.all())[0], lin.run(1, ce.MetricConfig.all())[0]
    finally:
        b8.close()
        lin.close()
    assert (s8.status, s8.psnr, s8.dssim, s8.ssimulacra2, s8.butteraugli) == (0, float("inf"), 0.0, 100.0, 0.0)
    assert sl.status == 0 and sl.butteraugli > 0.0 and sl.ssimulacra2 < 100.0


def test_a_set_between_launch_and_collect_returns_the_first_images_scores(ce, gpu_ctx, workloads, profiles):
    w, h = 96, 80
    src = workloads.make_reference(w, h, 5)
    d1, d2 = (workloads.distort(src, q) for q in (30, 90))
    for make in (lambda: ce.Batch(gpu_ctx, w, h, 1, 1), lambda: gpu_ctx.batch_linear(w, h, 1, 1), lambda: gpu_ctx.batch_deep(w, h, 1, 1, 8, 12)):
        b = make()
        try:
            b.set_reference_icc(0, src, 8, profiles["adobe"])
            b.set_test_icc(0, 0, d1, 8, profiles["adobe"])
            first = [scores_tuple(s) for s in b.run(1, ce.MetricConfig.all())]
            b.launch(1, ce.MetricConfig.all())
            b.set_test_icc(0, 0, d2, 8, profiles["adobe"])  # waits for the launch on the device, not on the host
            assert [scores_tuple(s) for s in b.collect(1)] == first
            second = [scores_tuple(s) for s in b.run(1, ce.MetricConfig.all())]
            assert second != first and second[0][3] > first[0][3]
        finally:
            b.close()


def _lut_based(profile):
    at = profile.index(b"cprt", 132)
    return profile[:at] + b"A2B0" + profile[at + 4:]


def test_refusals(ce, gpu_ctx, workloads, profiles):
    """Every refusal, each with its status and a reason, the batch still usable afterwards."""
    L = ce.lib()
    # profiles that are not matrix/TRC: no handle, CE_ERR_INVALID_ARG, the kind and the parser's reason in the text
    gray = R.write_profile([(b"kTRC", R.curv_tag())], 4, colour_space=b"GRAY")
    for bad, word in ((_lut_based(F["p3"]), "LUT-based"), (gray, "not an RGB profile"), (b"fake", "malformed"), (F["p3"][:300], "malformed")):
        with pytest.raises(ce.CodecEvalError, match=word) as e:
            ce.IccProfile(gpu_ctx, bad)
        assert e.value.status == ce.CE_ERR_INVALID_ARG
    h_out = C.c_void_p(1)
    assert L.ce_icc_create(gpu_ctx._h, None, 0, C.byref(h_out)) == ce.CE_ERR_INVALID_ARG and not h_out.value
    assert L.ce_icc_create(None, F["p3"], len(F["p3"]), C.byref(h_out)) == ce.CE_ERR_INVALID_ARG
    L.ce_icc_destroy(None)

    w, h = 32, 24
    src = workloads.make_reference(w, h, 2)
    dec = workloads.distort(src, 60)
    p = profiles["p3"]
    px16 = src.astype(np.uint16) * 4
    rgb8, deep, lin = ce.Batch(gpu_ctx, w, h, 1, 1), gpu_ctx.batch_deep(w, h, 1, 1, 10, 10), gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        before = {}
        for b in (rgb8, deep, lin):
            b.set_reference_icc(0, src, 8, p)
            b.set_test_icc(0, 0, dec, 8, p)
            before[id(b)] = [scores_tuple(s) for s in b.run(1, ce.MetricConfig.all())]

        def refused(call, status, word):
            rc = call()
            assert rc == status, (rc, word)
            assert word in gpu_ctx._err(), (gpu_ctx._err(), word)

        n8, n16 = src.nbytes, px16.nbytes
        for b in (rgb8, deep, lin):
            bh = b._h
            refused(lambda: L.ce_batch_set_test_icc(bh, 0, 0, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, None), ce.CE_ERR_INVALID_ARG, "null pointer")
            refused(lambda: L.ce_batch_set_reference_icc(bh, 0, None, n8, ce.PIXEL_RGB8, 8, p._h), ce.CE_ERR_INVALID_ARG, "null pointer")
            for fmt in (2, 3, ce.PIXEL_RGB_F32, 6, -1):  # the *_10BIT formats, f32, not a format
                refused(lambda: L.ce_batch_set_test_icc(bh, 0, 0, px16.ctypes.data, n16, fmt, 10, p._h), ce.CE_ERR_INVALID_ARG, "format must be")
            for depth in (0, 9, 14, 32):
                refused(lambda: L.ce_batch_set_test_icc(bh, 0, 0, px16.ctypes.data, n16, ce.PIXEL_RGB16, depth, p._h), ce.CE_ERR_INVALID_ARG,
                        "depth must be 8, 10, 12 or 16")
            refused(lambda: L.ce_batch_set_test_icc(bh, 0, 0, src.ctypes.data, n8, ce.PIXEL_RGB8, 10, p._h), ce.CE_ERR_INVALID_ARG,
                    "an 8-bit format needs depth 8")
            refused(lambda: L.ce_batch_set_test_icc(bh, 0, 0, src.ctypes.data, n8 - 3, ce.PIXEL_RGB8, 8, p._h), ce.CE_ERR_BAD_LENGTH, "Invalid image size")
            refused(lambda: L.ce_batch_set_reference_icc(bh, 0, src.ctypes.data, n8, ce.PIXEL_RGBA8, 8, p._h), ce.CE_ERR_BAD_LENGTH, "Invalid image size")
            refused(lambda: L.ce_batch_set_test_icc(bh, 1, 0, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h), ce.CE_ERR_INVALID_ARG, "out of range")
            refused(lambda: L.ce_batch_set_test_icc(bh, 0, 1, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h), ce.CE_ERR_INVALID_ARG, "out of range")
            refused(lambda: L.ce_batch_set_reference_icc(bh, 1, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h), ce.CE_ERR_INVALID_ARG, "out of range")
        # an RGB8 batch takes the 8-bit formats only
        for fmt in (ce.PIXEL_RGB16, ce.PIXEL_RGBA16):
            refused(lambda: L.ce_batch_set_test_icc(rgb8._h, 0, 0, px16.ctypes.data, n16, fmt, 10, p._h), ce.CE_ERR_INVALID_ARG, "an RGB8 batch takes")
        assert L.ce_batch_set_test_icc(None, 0, 0, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h) == ce.CE_ERR_INVALID_ARG
        # the leaves
        out = np.empty(w * h * 3, np.float32)
        out8, out16 = np.empty(w * h * 3, np.uint8), np.empty(w * h * 3, np.uint16)
        c = gpu_ctx._h
        refused(lambda: L.ce_icc_to_linear(c, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h, w, h, out.ctypes.data, out.size - 1), ce.CE_ERR_BAD_LENGTH, "out_len")
        refused(lambda: L.ce_icc_to_srgb8(c, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h, w, h, out8.ctypes.data, out8.size + 1), ce.CE_ERR_BAD_LENGTH, "out_len")
        refused(lambda: L.ce_icc_to_srgb16(c, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h, w, h, 10, out16.ctypes.data, 5), ce.CE_ERR_BAD_LENGTH, "out_len")
        refused(lambda: L.ce_icc_to_srgb16(c, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h, w, h, 11, out16.ctypes.data, out16.size), ce.CE_ERR_INVALID_ARG,
                "the output depth must be")
        refused(lambda: L.ce_icc_to_srgb8(c, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h, 0, h, out8.ctypes.data, 0), ce.CE_ERR_INVALID_ARG, "empty image")
        refused(lambda: L.ce_icc_to_srgb8(c, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h, w, h, None, out8.size), ce.CE_ERR_INVALID_ARG, "null output")
        refused(lambda: L.ce_icc_to_linear(c, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, None, w, h, out.ctypes.data, out.size), ce.CE_ERR_INVALID_ARG, "null pointer")
        refused(lambda: L.ce_icc_to_linear(c, src.ctypes.data, n8 + 1, ce.PIXEL_RGB8, 8, p._h, w, h, out.ctypes.data, out.size), ce.CE_ERR_BAD_LENGTH,
                "Invalid image size")
        refused(lambda: L.ce_icc_to_linear(c, src.ctypes.data, n8, ce.PIXEL_RGB8, 12, p._h, w, h, out.ctypes.data, out.size), ce.CE_ERR_INVALID_ARG,
                "an 8-bit format needs depth 8")
        assert L.ce_icc_to_linear(None, src.ctypes.data, n8, ce.PIXEL_RGB8, 8, p._h, w, h, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
        # every batch is as it was
        for b in (rgb8, deep, lin):
            assert [scores_tuple(s) for s in b.run(1, ce.MetricConfig.all())] == before[id(b)]
            assert b.pair_reference(0) == 0
    finally:
        for b in (rgb8, deep, lin):
            b.close()


# ---- the session ------------------------------------------------------------------------------------------------------------------

def _session(ce, gpu_ctx, tmp_path, decode, cms=None, qualities=(45, 80)):
    cfg = S.EvalConfig.builder().report_dir(tmp_path / "rep").metrics(ce.MetricConfig.all()).quality_levels(list(qualities)).build()
    ses = S.EvalSession(cfg, ctx=gpu_ctx, cms=cms)
    ses.add_codec_with_decode("tagging", "1", lambda im, rq: np.array([rq.quality], np.float32).tobytes(), decode)
    return ses


def _row(r):
    return (r.psnr, r.ssimulacra2, r.dssim, r.butteraugli)


def test_session_without_a_cms_applies_matrix_trc_profiles_in_every_group(ce, gpu_ctx, workloads, tmp_path):
    w, h = 80, 56
    src = workloads.make_reference(w, h, 31)
    quality = lambda blob: float(np.frombuffer(blob, np.float32)[0])
    all_metrics = ce.MetricConfig.all()

    # RGB8: an 8-bit decode tagged with the P3 profile; the source's own profile stays unapplied
    ses = _session(ce, gpu_ctx, tmp_path, lambda blob: S.ImageData.rgb_with_icc(workloads.distort(src, quality(blob)), w, h, F["p3"]))
    rep = ses.evaluate_image("x.png", S.ImageData.rgb_with_icc(src, w, h, F["adobe"]))
    assert len(rep.results) == 2
    for r in rep.results:
        want = R.to_srgb(workloads.distort(src, r.quality), F["p3"], 8)
        m = gpu_ctx.calculate_metrics(src, want, w, h, all_metrics)
        assert _row(r) == (m.psnr, m.ssimulacra2, m.dssim, m.butteraugli), r.quality
    plain = _session(ce, gpu_ctx, tmp_path, lambda blob: S.ImageData.rgb(workloads.distort(src, quality(blob)), w, h))
    assert _row(plain.evaluate_image("x.png", S.ImageData.rgb(src, w, h)).results[0]) != _row(rep.results[0])  # the profile changed the pixels
    assert len(ses._profiles) == 1  # one handle per profile for the session's lifetime
    ses.close()
    plain.close()

    # deep: a 10-bit decode (ImageData.rgb16 with icc_profile) against the 8-bit source, written at its own depth
    dec10 = lambda q: (workloads.distort(src, q).astype(np.uint16) * 4 + 1).reshape(h, w, 3)
    ses = _session(ce, gpu_ctx, tmp_path, lambda blob: S.ImageData.rgb16(dec10(quality(blob)), w, h, 10, icc_profile=F["adobe"]))
    rep = ses.evaluate_image("x.png", S.ImageData.rgb(src, w, h))
    b = gpu_ctx.batch_deep(w, h, 1, 2, 8, 10)
    try:
        b.set_reference(0, src)
        for i, r in enumerate(rep.results):
            b.set_test(i, 0, R.to_srgb(dec10(r.quality), F["adobe"], 10, 10))
        want = b.run(2, all_metrics)
    finally:
        b.close()
    ses.close()
    assert [_row(r) for r in rep.results] == [_row(ce.MetricResult.from_c(s)) for s in want]

    # linear: a source in linear light, the tagged 8-bit decode converted to linear light by the profile
    lin_src = ce.srgb_table(8, 0)[src]
    ses = _session(ce, gpu_ctx, tmp_path, lambda blob: S.ImageData.rgb_with_icc(workloads.distort(src, quality(blob)), w, h, F["prophoto"]))
    rep = ses.evaluate_image("x.png", S.ImageData.linear_f32(lin_src, w, h))
    b = gpu_ctx.batch_linear(w, h, 1, 2)
    try:
        b.set_reference(0, lin_src)
        for i, r in enumerate(rep.results):
            b.set_test(i, 0, R.to_linear(workloads.distort(src, r.quality), F["prophoto"], 8))
        want = b.run(2, all_metrics)
    finally:
        b.close()
    ses.close()
    assert [_row(r) for r in rep.results] == [_row(ce.MetricResult.from_c(s)) for s in want]


def test_session_keeps_todays_behaviour_with_a_cms_and_for_other_profiles(ce, gpu_ctx, workloads, tmp_path):
    w, h = 48, 40
    src = workloads.make_reference(w, h, 9)
    dec = workloads.distort(src, 60)
    calls = []

    def cms(profile, rgb):
        calls.append(profile)
        return 255 - rgb

    # with a cms everything is as it was: the callable is evaluated on the cube, for a matrix/TRC profile too
    ses = _session(ce, gpu_ctx, tmp_path, lambda blob: S.ImageData.rgb_with_icc(dec, w, h, F["p3"]), cms=cms, qualities=(50,))
    rep = ses.evaluate_image("x.png", S.ImageData.rgb(src, w, h))
    m = gpu_ctx.calculate_metrics(src, 255 - dec, w, h, ce.MetricConfig.all())
    assert calls == [F["p3"]] and _row(rep.results[0]) == (m.psnr, m.ssimulacra2, m.dssim, m.butteraugli) and not ses._profiles
    with pytest.raises(ce.MetricCalculation, match="an ICC profile is not applied in linear light"):
        ses.evaluate_image("x.png", S.ImageData.linear_f32(ce.srgb_table(8, 0)[src], w, h))
    ses.close()
    # without one, any other profile raises today's error, word for word: in an RGB8 and in a deep group before anything
    # reaches the device, for b"fake" as for a LUT-based profile
    for profile in (b"fake", _lut_based(F["p3"])):
        for decode in (lambda blob: S.ImageData.rgb_with_icc(dec, w, h, profile),
                       lambda blob: S.ImageData.rgb16(dec.astype(np.uint16), w, h, 10, icc_profile=profile)):
            ses = _session(ce, gpu_ctx, tmp_path, decode, qualities=(50,))
            with pytest.raises(ce.MetricCalculation) as e:
                ses.evaluate_image("x.png", S.ImageData.rgb(src, w, h))
            assert str(e.value).endswith("Metric calculation failed: ICC: ICC profile support requires the 'icc' feature")
            ses.close()
    # the source image's profile is never read, whatever it is
    ses = _session(ce, gpu_ctx, tmp_path, lambda blob: S.ImageData.rgb(dec, w, h), qualities=(50,))
    a = ses.evaluate_image("x.png", S.ImageData.rgb_with_icc(src, w, h, b"fake")).results[0]
    b = ses.evaluate_image("x.png", S.ImageData.rgb(src, w, h)).results[0]
    assert _row(a) == _row(b)
    ses.close()


def test_a_session_that_made_its_context_closes_it_after_its_profiles(ce, gpu_ctx, workloads, tmp_path):
    """EvalSession() without ctx= owns its context: close() destroys the profile handles and the colour tables first, then
    the context; a session that was given a context leaves it open."""
    w, h = 48, 40
    src = workloads.make_reference(w, h, 4)
    cfg = S.EvalConfig.builder().report_dir(tmp_path / "rep").metrics(ce.MetricConfig.fast()).quality_levels([50]).build()
    own = S.EvalSession(cfg)
    own.add_codec_with_decode("tagging", "1", lambda im, rq: b"x", lambda blob: S.ImageData.rgb_with_icc(workloads.distort(src, 60), w, h, F["p3"]))
    assert own.evaluate_image("x.png", S.ImageData.rgb(src, w, h)).results[0].psnr is not None
    ctx, (profile,) = own.ctx, own._profiles.values()
    assert ctx is not gpu_ctx and ctx._h and profile._h
    own.close()
    assert not ctx._h and not profile._h and not own._profiles
    own.close()  # a second close finds nothing left
    lent = _session(ce, gpu_ctx, tmp_path, lambda blob: S.ImageData.rgb(src, w, h), qualities=(50,))
    lent.close()
    assert gpu_ctx._h and gpu_ctx.calculate_metrics(src, src, w, h, ce.MetricConfig.fast()).psnr == float("inf")
