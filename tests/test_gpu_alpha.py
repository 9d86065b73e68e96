"""Alpha compositing on the device (ce_batch_set_*_over, ce_composite_rgba*) against the numpy restatement
(tests/alpha_restatement.py, itself pinned to Pillow in test_alpha_composite_cpu.py) bit for bit: slab bytes of RGB8 and
deep batches at odd slot offsets, one call over K backgrounds against K calls, the leaves, scores against uploads of the
restated composites; the two score errors that dropping alpha makes (hidden differences scored, alpha damage not scored)
and that compositing removes; the session; every refusal; ordering against a launch in flight."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_restatement as A  # noqa: E402

pytestmark = pytest.mark.gpu

S = importlib.import_module("codec-eval_amd.session")
SHAPES = ((1, 1), (3, 5), (7, 2), (17, 9), (301, 9), (64, 64), (768, 512))
BLACK, WHITE = (0, 0, 0), (255, 255, 255)


def read_slab(ce, address, nbytes):
    """Device bytes -> host after everything queued on the device (the slot writes run on the batch's upload stream)."""
    assert ce.lib().hipDeviceSynchronize() == 0
    out = np.empty(nbytes, np.uint8)
    assert ce.lib().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(address), ctypes.c_size_t(nbytes), 2) == 0
    return out


def scores_tuple(s):
    return (s.status, s.valid, s.dssim, s.ssimulacra2, s.butteraugli, s.psnr)


def backgrounds(rng, K, m):
    bg = rng.integers(0, m + 1, (K, 3))
    bg[0] = (0, m, m // 2)
    return bg


# (source depth / dtype, batch depths): RGBA8 into an RGB8 batch, RGBA8 into a deep side of depth 8, RGBA16 at every depth
FORMS = [(8, np.uint8, None), (8, np.uint8, (8, 8)), (8, np.uint16, (8, 8)), (10, np.uint16, (10, 10)), (12, np.uint16, (12, 12)),
         (16, np.uint16, (16, 16))]


@pytest.mark.parametrize("w,h", SHAPES)
def test_slab_bytes_equal_the_restatement(gpu_ctx, ce, w, h):
    """first_ref = first_pair = 1: slot 1 of an RGB8 slab starts at w * h * 3 bytes, odd for odd w * h, and slot 1 + k at
    every other alignment; the slots in front of and behind the written ones keep their bytes."""
    rng = np.random.default_rng(w * 1000 + h)
    for d, dt, depths in FORMS if w * h < 100000 else (FORMS[0], FORMS[3]):
        m = (1 << d) - 1
        out_dt = np.uint8 if depths is None else np.uint16
        fmt = ce.PIXEL_RGBA8 if dt == np.uint8 else ce.PIXEL_RGBA16
        for K in (1, 2, 8):
            n = K + 2
            batch = ce.Batch(gpu_ctx, w, h, n, n, depths=depths)
            try:
                fill = rng.integers(0, m + 1, (2, n, h, w, 3)).astype(out_dt)
                for i in range(n):
                    batch.set_reference(i, fill[0, i])
                    batch.set_test(i, 0, fill[1, i])
                ref_px, test_px = A.random_rgba(rng, w, h, d, dt, over=True), A.random_rgba(rng, w, h, d, dt, over=True)
                bg_r, bg_t = backgrounds(rng, K, m), backgrounds(rng, K, m)
                batch.set_reference_over(1, ref_px, fmt, bg_r)
                refs = [(k * 3 + 1) % n for k in range(K)]
                batch.set_test_over(1, refs, test_px, fmt, bg_t)
                assert [batch.pair_reference(1 + k) for k in range(K)] == refs
                want = fill.copy()
                for k in range(K):
                    want[0, 1 + k] = A.composite(ref_px, bg_r[k], d)
                    want[1, 1 + k] = A.composite(test_px, bg_t[k], d)
                got_r = read_slab(ce, batch.reference_slab, want[0].nbytes).view(out_dt).reshape(want[0].shape)
                got_t = read_slab(ce, batch.test_slab, want[1].nbytes).view(out_dt).reshape(want[1].shape)
                for i in range(n):
                    assert np.array_equal(got_r[i], want[0, i]), (d, dt, depths, K, "reference slot", i)
                    assert np.array_equal(got_t[i], want[1, i]), (d, dt, depths, K, "test slot", i)
            finally:
                batch.close()


@pytest.mark.parametrize("deep", [False, True])
def test_one_call_equals_k_calls_and_the_leaves(gpu_ctx, ce, deep):
    w, h = 17, 9
    rng = np.random.default_rng(23)
    d = 10 if deep else 8
    m = (1 << d) - 1
    px = A.random_rgba(rng, w, h, d)
    fmt = ce.PIXEL_RGBA16 if deep else ce.PIXEL_RGBA8
    K = 8
    bg = backgrounds(rng, K, m)
    a, b = (ce.Batch(gpu_ctx, w, h, K + 1, K + 1, depths=(10, 10) if deep else None) for _ in range(2))
    try:
        a.set_reference_over(1, px, fmt, bg)
        a.set_test_over(1, list(range(K)), px, fmt, bg)
        for k in range(K):
            b.set_reference_over(1 + k, px, fmt, bg[k:k + 1])
            b.set_test_over(1 + k, [k], px, fmt, bg[k:k + 1])
        nbytes = (K + 1) * w * h * 3 * (2 if deep else 1)
        off = nbytes // (K + 1)  # slot 0 was never written
        ra, rb = read_slab(ce, a.reference_slab, nbytes), read_slab(ce, b.reference_slab, nbytes)
        ta, tb = read_slab(ce, a.test_slab, nbytes), read_slab(ce, b.test_slab, nbytes)
        assert np.array_equal(ra[off:], rb[off:]) and np.array_equal(ta[off:], tb[off:])
        slots = ra[off:].view(np.uint16 if deep else np.uint8).reshape(K, h, w, 3)
        for k in range(K):
            leaf = gpu_ctx.composite_rgba16(px, w, h, d, bg[k]) if deep else gpu_ctx.composite_rgba8(px, w, h, bg[k])
            assert leaf.shape == (h, w, 3) and np.array_equal(leaf, slots[k]) and np.array_equal(leaf, A.composite(px, bg[k], d))
    finally:
        a.close(), b.close()
    # the leaves on the other shapes and depths, the large one included
    for (lw, lh), ld in (((768, 512), 8), ((301, 9), 12), ((3, 5), 16), ((1, 1), 8), ((64, 64), 16)):
        lm = (1 << ld) - 1
        lp = A.random_rgba(rng, lw, lh, ld, np.uint16, over=True)
        lbg = tuple(int(v) for v in rng.integers(0, lm + 1, 3))
        assert np.array_equal(gpu_ctx.composite_rgba16(lp, lw, lh, ld, lbg), A.composite(lp, lbg, ld))
        if ld == 8:
            lp8 = A.random_rgba(rng, lw, lh, 8)
            assert np.array_equal(gpu_ctx.composite_rgba8(lp8, lw, lh, lbg), A.composite(lp8, lbg))


def smooth_rgba(workloads, w, h, seed, alpha):
    rgb = np.asarray(workloads.make_reference(w, h, seed), np.uint8).reshape(h, w, 3)
    return np.ascontiguousarray(np.dstack([rgb, alpha.astype(np.uint8)]))


def soft_alpha(w, h):
    """a soft-edged disc: opaque inside, clear outside, every level in between on the rim"""
    y, x = np.mgrid[0:h, 0:w]
    r = np.hypot((x - w / 2) / (w / 2), (y - h / 2) / (h / 2))
    return np.clip(np.rint((0.9 - r) * 255 / 0.35), 0, 255)


@pytest.mark.parametrize("deep", [False, True])
def test_scores_equal_those_of_the_restated_composites(gpu_ctx, ce, workloads, deep):
    w, h = 100, 76
    ref = smooth_rgba(workloads, w, h, 3, soft_alpha(w, h))
    test = ref.copy()
    test[..., :3] = np.asarray(workloads.distort(np.ascontiguousarray(ref[..., :3]), 50), np.uint8).reshape(h, w, 3)
    test[..., 3] = (test[..., 3] >> 4) * 17
    d = 8
    if deep:  # 8-bit values spread over 10 bits
        d, ref, test = 10, (ref.astype(np.uint32) * 1023 + 127) // 255, (test.astype(np.uint32) * 1023 + 127) // 255
        ref, test = ref.astype(np.uint16), test.astype(np.uint16)
    m = (1 << d) - 1
    fmt = ce.PIXEL_RGBA16 if deep else ce.PIXEL_RGBA8
    bg = np.array([A.scale_background(c, d) for c in (BLACK, WHITE, (255, 0, 128))])
    K = len(bg)
    depths = (10, 10) if deep else None
    a, b = ce.Batch(gpu_ctx, w, h, K, K, depths=depths), ce.Batch(gpu_ctx, w, h, K, K, depths=depths)
    try:
        a.set_reference_over(0, ref, fmt, bg)
        a.set_test_over(0, list(range(K)), test, fmt, bg)
        for k in range(K):
            b.set_reference(k, A.composite(ref, bg[k], d))
            b.set_test(k, k, A.composite(test, bg[k], d))
        sa = a.run(K, ce.MetricConfig.all(), butteraugli_diffmap=True)
        sb = b.run(K, ce.MetricConfig.all(), butteraugli_diffmap=True)
        for x, y in zip(sa, sb):
            assert x.status == 0 and x.valid == 15
            assert scores_tuple(x) == scores_tuple(y)
        assert np.array_equal(a.butteraugli_diffmaps(0, K), b.butteraugli_diffmaps(0, K))
        assert len({s.ssimulacra2 for s in sa}) == K  # the backgrounds differ, and the scores see it
    finally:
        a.close(), b.close()


def test_hidden_differences_are_not_scored(gpu_ctx, ce, workloads):
    """RGB that differs only under alpha = 0 (what libwebp writes without -exact): identical over black and over white,
    while the alpha-dropping route scores the invisible pixels."""
    w, h = 96, 64
    alpha = np.where(soft_alpha(w, h) > 0, 255, 0)
    alpha[:, : w // 8] = 0
    ref = smooth_rgba(workloads, w, h, 5, alpha)
    test = ref.copy()
    hidden = test[..., 3] == 0
    assert hidden.sum() > w * h // 8
    test[hidden, :3] = 0  # the encoder's choice under transparent pixels
    assert np.any(ref[hidden, :3] != 0) and np.array_equal(ref[~hidden], test[~hidden])
    batch = ce.Batch(gpu_ctx, w, h, 2, 3)
    try:
        batch.set_reference_over(0, ref, ce.PIXEL_RGBA8, [BLACK, WHITE])
        batch.set_test_over(0, [0, 1], test, ce.PIXEL_RGBA8, [BLACK, WHITE])
        for s in batch.run(2, ce.MetricConfig.all()):
            assert s.status == 0 and s.valid == 15
            assert s.ssimulacra2 == 100.0 and s.dssim == 0.0 and s.butteraugli == 0.0
        batch.set_reference_fmt(0, ref, ce.PIXEL_RGBA8)
        batch.set_test_fmt(2, 0, test, ce.PIXEL_RGBA8)
        s = batch.run(3, ce.MetricConfig.all())[2]
        assert s.status == 0 and s.ssimulacra2 < 100.0 and s.dssim > 0.0 and s.butteraugli > 0.0
    finally:
        batch.close()


def test_alpha_damage_is_scored(gpu_ctx, ce, workloads):
    """Equal RGB, alpha quantised to 4 bits: worse than identical over a background of another colour than the image, where
    the change shows; the alpha-dropping route calls the pair identical; a flat image over its own colour IS identical."""
    w, h = 96, 64
    y, x = np.mgrid[0:h, 0:w]
    ramp = np.clip(np.rint(255 * (x + y) / (w + h - 2)), 0, 255)
    ref = smooth_rgba(workloads, w, h, 9, ramp)
    test = ref.copy()
    test[..., 3] = (test[..., 3] >> 4) << 4
    assert np.any(test[..., 3] != ref[..., 3]) and np.array_equal(test[..., :3], ref[..., :3])
    batch = ce.Batch(gpu_ctx, w, h, 2, 3)
    try:
        batch.set_reference_over(0, ref, ce.PIXEL_RGBA8, [BLACK, WHITE])
        batch.set_test_over(0, [0, 1], test, ce.PIXEL_RGBA8, [BLACK, WHITE])
        for s in batch.run(2, ce.MetricConfig.all()):
            assert s.status == 0 and s.valid == 15
            assert s.ssimulacra2 < 100.0 and s.dssim > 0.0 and s.butteraugli > 0.0
        batch.set_reference_fmt(0, ref, ce.PIXEL_RGBA8)
        batch.set_test_fmt(2, 0, test, ce.PIXEL_RGBA8)
        s = batch.run(3, ce.MetricConfig.all())[2]
        assert s.ssimulacra2 == 100.0 and s.dssim == 0.0 and s.butteraugli == 0.0
        # a flat colour: over that colour every alpha gives the colour, over another one the quantisation shows
        colour = (40, 170, 90)
        flat_r, flat_t = ref.copy(), test.copy()
        flat_r[..., :3] = flat_t[..., :3] = colour
        batch.set_reference_over(0, flat_r, ce.PIXEL_RGBA8, [colour, WHITE])
        batch.set_test_over(0, [0, 1], flat_t, ce.PIXEL_RGBA8, [colour, WHITE])
        same, other = batch.run(2, ce.MetricConfig.all())
        assert same.ssimulacra2 == 100.0 and same.dssim == 0.0 and same.butteraugli == 0.0
        assert other.ssimulacra2 < 100.0 and other.dssim > 0.0 and other.butteraugli > 0.0
    finally:
        batch.close()


def _session_rows(gpu_ctx, ce, tmp_path, tag, source, decodes, alpha_backgrounds):
    b = S.EvalConfig.builder().report_dir(tmp_path / tag).metrics(ce.MetricConfig.all()).quality_levels(sorted(decodes))
    cfg = b.alpha_backgrounds(alpha_backgrounds).build()
    ses = S.EvalSession(cfg, ctx=gpu_ctx)
    ses.add_codec_with_decode("c", "1", lambda im, rq: b"%d" % int(rq.quality), lambda blob: decodes[int(blob)])
    rep = ses.evaluate_image("x", source)
    return rep, [(r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in rep.results]


def test_session(gpu_ctx, ce, workloads, tmp_path, monkeypatch):
    w, h = 100, 76
    src = smooth_rgba(workloads, w, h, 13, soft_alpha(w, h))
    dec = {}
    for q in (40, 80):
        t = src.copy()
        t[..., :3] = np.asarray(workloads.distort(np.ascontiguousarray(src[..., :3]), q), np.uint8).reshape(h, w, 3)
        t[..., 3] = (t[..., 3] >> 4) * 17
        dec[q] = t
    source = S.ImageData.rgba(src, w, h)
    decodes = {q: S.ImageData.rgba(t, w, h) for q, t in dec.items()}
    decodes[90] = S.ImageData.rgb(np.ascontiguousarray(dec[80][..., :3]), w, h)  # an opaque decode of a source with alpha

    # None: the parent's behaviour, bit for bit - alpha dropped on both sides
    rep0, rows0 = _session_rows(gpu_ctx, ce, tmp_path, "none", source, decodes, None)
    assert S.EvalConfig("x").alpha_backgrounds is None and rep0.alpha_scores == {}
    batch = ce.Batch(gpu_ctx, w, h, 1, 3)
    try:
        batch.set_reference(0, np.ascontiguousarray(src[..., :3]))
        for i, q in enumerate((40, 80, 90)):
            batch.set_test(i, 0, np.ascontiguousarray(dec[min(q, 80)][..., :3]))
        want0 = [(s.dssim, s.ssimulacra2, s.butteraugli, s.psnr) for s in batch.run(3, ce.MetricConfig.all())]
    finally:
        batch.close()
    assert rows0 == want0

    # black + white: the worst of the manual per-background scores, each retrievable
    rep, rows = _session_rows(gpu_ctx, ce, tmp_path, "bw", source, decodes, S.ALPHA_BLACK_WHITE)
    batch = ce.Batch(gpu_ctx, w, h, 2, 6)
    try:
        for k, bg in enumerate(S.ALPHA_BLACK_WHITE):
            batch.set_reference(k, A.composite(src, bg))
            for i, q in enumerate((40, 80)):
                batch.set_test(2 * i + k, k, A.composite(dec[q], bg))
            batch.set_test(4 + k, k, np.ascontiguousarray(dec[80][..., :3]))
        manual = batch.run(6, ce.MetricConfig.all())
    finally:
        batch.close()
    for i in range(3):
        per_bg = [manual[2 * i + k] for k in range(2)]
        assert [(m.dssim, m.ssimulacra2, m.butteraugli, m.psnr) for m in rep.alpha_scores[i]] == \
               [(s.dssim, s.ssimulacra2, s.butteraugli, s.psnr) for s in per_bg]
        assert rows[i] == (max(s.dssim for s in per_bg), min(s.ssimulacra2 for s in per_bg), max(s.butteraugli for s in per_bg),
                           min(s.psnr for s in per_bg))
    assert rows != rows0
    assert "alpha" not in rep.to_obj() and "alpha" not in str(rep.to_obj())

    # the device-free multi-device session composites on the host: the same rows
    md = importlib.import_module("codec-eval_amd.multidevice")
    cfg = S.EvalConfig.builder().report_dir(tmp_path / "multi").metrics(ce.MetricConfig.all()).quality_levels([40, 80, 90]) \
        .alpha_backgrounds(S.ALPHA_BLACK_WHITE).build()
    multi = md.MultiDeviceEvalSession(cfg)
    try:
        multi.add_codec_with_decode("c", "1", lambda im, rq: b"%d" % int(rq.quality), lambda blob: decodes[int(blob)])
        corpus, _stats = multi.evaluate_corpus("c", [("x", source)])
        assert [(r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in corpus.images[0].results] == rows
        assert sorted(corpus.images[0].alpha_scores) == [0, 1, 2]
    finally:
        multi.close()

    # an RGB-only corpus uses no extra slots: the batches it makes are the ones it makes without the setting
    made = []
    real = S.Batch

    def spy(ctx, bw, bh, n_refs, n_pairs, depths=None):
        made.append((bw, bh, n_refs, n_pairs, depths))
        return real(ctx, bw, bh, n_refs, n_pairs, depths=depths)

    monkeypatch.setattr(S, "Batch", spy)
    rgb_src = S.ImageData.rgb(np.ascontiguousarray(src[..., :3]), w, h)
    rgb_dec = {q: S.ImageData.rgb(np.ascontiguousarray(dec[q][..., :3]), w, h) for q in (40, 80)}
    rep_a, rows_a = _session_rows(gpu_ctx, ce, tmp_path, "rgb_bw", rgb_src, rgb_dec, S.ALPHA_BLACK_WHITE)
    made_a, made[:] = list(made), []
    rep_b, rows_b = _session_rows(gpu_ctx, ce, tmp_path, "rgb_none", rgb_src, rgb_dec, None)
    assert made_a == made == [(w, h, 1, 2, None)] and rows_a == rows_b == want0[:2] and rep_a.alpha_scores == {}
    # an opaque source with decodes that have alpha: one reference slot, one test slot per background and pair
    made[:] = []
    rep_c, _ = _session_rows(gpu_ctx, ce, tmp_path, "mixed", rgb_src, {40: decodes[40], 80: rgb_dec[80]}, S.ALPHA_BLACK_WHITE)
    assert made == [(w, h, 1, 3, None)] and sorted(rep_c.alpha_scores) == [0]


def test_session_deep(gpu_ctx, ce, workloads, tmp_path):
    """a 10-bit decode with alpha against an 8-bit source with alpha: each side's backgrounds at its own depth"""
    w, h = 64, 48
    src = smooth_rgba(workloads, w, h, 17, soft_alpha(w, h))
    dec = ((src.astype(np.uint32) * 1023 + 127) // 255).astype(np.uint16)
    dec[..., 3] = (dec[..., 3] >> 6) << 6
    rep, rows = _session_rows(gpu_ctx, ce, tmp_path, "deep", S.ImageData.rgba(src, w, h), {50: S.ImageData.rgba16(dec, w, h, 10)}, S.ALPHA_BLACK_WHITE)
    batch = ce.Batch(gpu_ctx, w, h, 2, 2, depths=(8, 10))
    try:
        for k, bg in enumerate(S.ALPHA_BLACK_WHITE):
            batch.set_reference(k, A.composite(src, bg).astype(np.uint16))
            batch.set_test(k, k, A.composite(dec, A.scale_background(bg, 10), 10))
        manual = batch.run(2, ce.MetricConfig.all())
    finally:
        batch.close()
    assert [(m.dssim, m.ssimulacra2, m.butteraugli) for m in rep.alpha_scores[0]] == [(s.dssim, s.ssimulacra2, s.butteraugli) for s in manual]
    assert rows[0][:3] == (max(s.dssim for s in manual), min(s.ssimulacra2 for s in manual), max(s.butteraugli for s in manual))


def test_refusals_leave_the_handles_usable(gpu_ctx, ce):
    w, h = 16, 10
    rng = np.random.default_rng(29)
    px8, px16 = A.random_rgba(rng, w, h, 8), A.random_rgba(rng, w, h, 10)
    bw = np.array([BLACK, WHITE], np.uint16)
    refs = np.array([0, 1], np.uint32)
    L = ce.lib()
    p = lambda a: a.ctypes.data
    b8 = ce.Batch(gpu_ctx, w, h, 2, 2)
    b10 = ce.Batch(gpu_ctx, w, h, 2, 2, depths=(10, 10))
    try:
        def ref_call(batch, first=0, pixels=px8, nbytes=None, fmt=ce.PIXEL_RGBA8, n_bg=2, bg=bw):
            return L.ce_batch_set_reference_over(batch._h if batch else None, first, p(pixels) if pixels is not None else None,
                                                 pixels.nbytes if nbytes is None else nbytes, fmt, n_bg, p(bg) if bg is not None else None)

        def test_call(batch, first=0, r=refs, pixels=px8, nbytes=None, fmt=ce.PIXEL_RGBA8, n_bg=2, bg=bw):
            return L.ce_batch_set_test_over(batch._h if batch else None, first, p(r) if r is not None else None, p(pixels) if pixels is not None else None,
                                            pixels.nbytes if nbytes is None else nbytes, fmt, n_bg, p(bg) if bg is not None else None)

        nine = np.zeros((9, 3), np.uint16)
        rgb16_10bit = np.zeros((h, w, 4), np.uint16)
        bad = {
            "null pixels": dict(pixels=None, nbytes=w * h * 4),
            "null backgrounds": dict(bg=None),
            "format without alpha": dict(fmt=ce.PIXEL_RGB8, nbytes=w * h * 3),
            "RGB16_10BIT": dict(fmt=ce.PIXEL_RGB16_10BIT, pixels=rgb16_10bit),
            "RGBA16_10BIT": dict(fmt=ce.PIXEL_RGBA16_10BIT, pixels=rgb16_10bit),
            "RGBA16 on an RGB8 batch": dict(fmt=ce.PIXEL_RGBA16, pixels=px16),
            "wrong len": dict(nbytes=w * h * 4 - 1),
            "n_bg = 0": dict(n_bg=0),
            "n_bg = 9": dict(n_bg=9, bg=nine),
            "background above m": dict(bg=np.array([BLACK, (0, 256, 0)], np.uint16)),
            "slot range past the batch": dict(first=1),
            "first slot past the batch": dict(first=5, n_bg=1),
        }
        want = [A.composite(px8, bg) for bg in (BLACK, WHITE)]
        for what, kw in bad.items():
            assert ref_call(b8, **kw) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err(), what
            assert test_call(b8, **kw) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err(), what
            b8.set_reference_over(0, px8, ce.PIXEL_RGBA8, bw)
            b8.set_test_over(0, [0, 1], px8, ce.PIXEL_RGBA8, bw)
            s = b8.run(2, ce.MetricConfig.all())
            assert all(x.status == 0 and x.valid == 15 and x.ssimulacra2 == 100.0 for x in s), what
            got = read_slab(ce, b8.test_slab, 2 * w * h * 3).reshape(2, h, w, 3)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
        assert test_call(b8, r=None) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err()
        assert test_call(b8, r=np.array([0, 2], np.uint32)) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err()  # a ref index past the batch
        assert ref_call(None) == ce.CE_ERR_INVALID_ARG and test_call(None) == ce.CE_ERR_INVALID_ARG
        # a deep batch: RGBA8 needs a side of depth 8; the backgrounds are at the side's depth
        assert ref_call(b10) == ce.CE_ERR_INVALID_ARG and "depth 8" in gpu_ctx._err()
        assert test_call(b10) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err()
        assert ref_call(b10, fmt=ce.PIXEL_RGBA16, pixels=px16, bg=np.array([BLACK, (1024, 0, 0)], np.uint16)) == ce.CE_ERR_INVALID_ARG
        bg10 = np.array([BLACK, (1023, 1023, 1023)], np.uint16)
        b10.set_reference_over(0, px16, ce.PIXEL_RGBA16, bg10)
        b10.set_test_over(0, [0, 1], px16, ce.PIXEL_RGBA16, bg10)
        assert all(x.status == 0 and x.ssimulacra2 == 100.0 for x in b10.run(2, ce.MetricConfig.all()))

        # the leaves
        out8, out16 = np.empty(w * h * 3, np.uint8), np.empty(w * h * 3, np.uint16)
        bg8, bg16 = np.array(WHITE, np.uint8), np.array((1023,) * 3, np.uint16)
        c8 = lambda ctx=gpu_ctx._h, src=p(px8), n=px8.size, bg=p(bg8), out=p(out8), on=out8.size: L.ce_composite_rgba8(ctx, src, n, w, h, bg, out, on)
        c16 = lambda ctx=gpu_ctx._h, src=p(px16), n=px16.size, depth=10, bg=p(bg16), out=p(out16), on=out16.size: \
            L.ce_composite_rgba16(ctx, src, n, w, h, depth, bg, out, on)
        for kw in (dict(ctx=None), dict(src=None), dict(bg=None), dict(out=None), dict(n=px8.size - 4), dict(on=out8.size + 1)):
            assert c8(**kw) == ce.CE_ERR_INVALID_ARG, kw
            assert c16(**kw) == ce.CE_ERR_INVALID_ARG, kw
            if kw != dict(ctx=None):
                assert gpu_ctx._err(), kw
        for depth in (0, 9, 14, 17):
            assert c16(depth=depth) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err(), depth
        assert c16(bg=p(np.array((1024, 0, 0), np.uint16))) == ce.CE_ERR_INVALID_ARG and gpu_ctx._err()
        assert c8() == 0 and np.array_equal(out8.reshape(h, w, 3), A.composite(px8, WHITE))
        assert c16() == 0 and np.array_equal(out16.reshape(h, w, 3), A.composite(px16, (1023,) * 3, 10))
    finally:
        b8.close(), b10.close()


def test_upload_between_launch_and_collect_is_ordered(gpu_ctx, ce, workloads):
    """A composited upload into slots that a launch in flight still reads waits for that launch; the launch that follows
    sees the new images."""
    w, h = 192, 128
    cfg = ce.MetricConfig.all()
    first_r = smooth_rgba(workloads, w, h, 31, soft_alpha(w, h))
    first_t = first_r.copy()
    first_t[..., :3] = np.asarray(workloads.distort(np.ascontiguousarray(first_r[..., :3]), 40), np.uint8).reshape(h, w, 3)
    second_r = smooth_rgba(workloads, w, h, 37, 255 - soft_alpha(w, h))
    second_t = second_r.copy()
    second_t[..., 3] = (second_t[..., 3] >> 5) << 5
    bw = [BLACK, WHITE]

    def fill(b, r, t):
        b.set_reference_over(0, r, ce.PIXEL_RGBA8, bw)
        b.set_test_over(0, [0, 1], t, ce.PIXEL_RGBA8, bw)

    def alone(r, t):
        b = ce.Batch(gpu_ctx, w, h, 2, 2)
        try:
            fill(b, r, t)
            return [scores_tuple(s) for s in b.run(2, cfg)]
        finally:
            b.close()

    want_first, want_second = alone(first_r, first_t), alone(second_r, second_t)
    assert want_first != want_second
    b = ce.Batch(gpu_ctx, w, h, 2, 2)
    try:
        fill(b, first_r, first_t)
        b.launch(2, cfg)
        fill(b, second_r, second_t)  # while the launch is in flight
        assert [scores_tuple(s) for s in b.collect(2)] == want_first
        assert [scores_tuple(s) for s in b.run(2, cfg)] == want_second
        got = read_slab(ce, b.test_slab, 2 * w * h * 3).reshape(2, h, w, 3)
        assert np.array_equal(got[0], A.composite(second_t, BLACK)) and np.array_equal(got[1], A.composite(second_t, WHITE))
    finally:
        b.close()
