"""compute_heuristics (crates/codec-compare/src/image_heuristics.rs:76-305) on the device against the numpy restatement
(tests/heuristics_restatement.py): the per-pixel / per-block fields bit for bit, the whole-image sums within 2 f32 ulp of
the restatement's f64 mode, the same struct from every entry point, and no effect on a launch's scores or maps."""
import ctypes

import numpy as np
import pytest

import heuristics_restatement as H

pytestmark = pytest.mark.gpu

F = np.float32
EXACT = ("width", "height", "pixels") + H.TIER_A
# DESIGN.md section 2, the ledger: over the golden inputs and the benchmark shapes the device's Tier B fields are within
# 4.2e-4 (relative) of the reference's sequential f32 sums, except where exact arithmetic gives 0 - a flat image, whose
# sequential mean drifts and leaves a variance of 8.8e-6 (standard deviation 3.0e-3) - so: relative 5e-4, or 3e-3 absolute
LEDGER_REL_GAP, LEDGER_ABS_GAP = 5e-4, 3e-3


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _gradient(w, h):
    x = np.linspace(0, 255, w)[None, :, None]
    y = np.linspace(0, 255, h)[:, None, None]
    return np.broadcast_to(np.concatenate([x + 0 * y, y + 0 * x, (x + y) / 2], axis=2), (h, w, 3)).astype(np.uint8)


def _flat(w, h):
    return np.broadcast_to(np.array([90, 140, 200], np.uint8), (h, w, 3)).copy()


def _exact_gray_colors(targets):
    """An RGB8 colour whose f32 gray is exactly each target value."""
    found = {}
    g = np.arange(256, dtype=np.float32)[:, None]
    b = np.arange(256, dtype=np.float32)[None, :]
    for r in range(256):
        gray = (F(0.299) * F(r) + F(0.587) * g) + F(0.114) * b
        for t in targets:
            if t not in found:
                idx = np.argwhere(gray == F(t))
                if len(idx):
                    found[t] = (r, int(idx[0][0]), int(idx[0][1]))
        if len(found) == len(targets):
            return found
    raise AssertionError(f"no exact colour for {set(targets) - set(found)}")


def threshold_image():
    """64 x 32: gradients of exactly 30 and adjacent differences of exactly 10 and 30, and 8x8 blocks whose variance is
    exactly 100, 500, 1000, 2000 and 5000 (two levels m +- d around m = 100 over n pixels each: var = 2 n d^2 / 64, every
    partial sum an exact integer)."""
    c = _exact_gray_colors([0, 10, 20, 30, 60, 90, 100, 110, 140, 180])
    img = np.zeros((32, 64, 3), np.uint8)
    col = np.arange(64)
    img[0:8][:, (col % 4) >= 2] = c[30]    # columns 0,0,30,30,...: gx = 30, |diff| = 30
    img[8:16][:, (col % 4) >= 2] = c[10]   # |diff| = 10
    img[16:32] = c[100]
    for k, (t, d) in enumerate([(100, 10), (500, 40), (1000, 40), (2000, 80), (5000, 80)]):
        n = 32 * t // (d * d)
        vals = [100 + d] * n + [100 - d] * n + [100] * (64 - 2 * n)
        blk = np.array([c[v] for v in vals], np.uint8).reshape(8, 8, 3)
        img[16:24, 8 * k:8 * k + 8] = blk
    return img


def _check(got, rgb, w, h, label, counts=None):
    want = H.compute(rgb, w, h, "f64")
    for f in EXACT:
        g, e = getattr(got, f), want[f]
        if f in ("width", "height", "pixels"):
            assert g == e, (label, f, g, e)
        else:
            assert F(g).view(np.int32) == F(e).view(np.int32), (label, f, float(g), float(e))
    for f in H.TIER_B:
        d = H.ulp_distance(getattr(got, f), want[f])
        assert d <= 2, (label, f, float(getattr(got, f)), float(want[f]), d)
        if counts is not None and d:
            counts[f] = counts.get(f, 0) + 1
    return want


SHAPES = [(3, 3), (7, 7), (8, 8), (9, 17), (17, 9), (63, 64), (65, 64), (64, 63), (64, 65), (63, 63), (65, 65),
          (127, 129), (512, 512), (768, 512), (512, 768)]


def test_tier_a_exact_and_tier_b_within_two_ulp(ce, gpu_ctx):
    diffs, n = {}, 0
    for w, h in SHAPES:
        for kind, img in (("noise", _noise(w, h, w * 1000 + h)), ("gradient", _gradient(w, h)), ("flat", _flat(w, h))):
            _check(gpu_ctx.image_heuristics(img, w, h), img, w, h, f"{kind} {w}x{h}", diffs)
            n += 1
    for w, h in ((1920, 1080), (3840, 2160)):
        for kind, img in (("noise", _noise(w, h, 7)), ("gradient", _gradient(w, h))):
            _check(gpu_ctx.image_heuristics(img, w, h), img, w, h, f"{kind} {w}x{h}", diffs)
            n += 1
    print(f"\n{n} images: Tier B fields 1-2 ulp from the f64 restatement: {sum(diffs.values())} {diffs}")


def test_golden_inputs(ce, gpu_ctx):
    import os

    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "inputs.npz"))
    diffs = {}
    for name in d.files:
        img = d[name]
        h, w = img.shape[:2]
        _check(gpu_ctx.image_heuristics(img, w, h, name), img, w, h, name, diffs)
    print(f"\n{len(d.files)} golden images: Tier B fields 1-2 ulp from the f64 restatement: {sum(diffs.values())} {diffs}")


def test_values_exactly_on_the_thresholds(ce, gpu_ctx):
    img = threshold_image()
    h, w = img.shape[:2]
    gray = H.gray_of(img)
    es, diff, bv = H.edge_strengths(gray), H.adjacent_diffs(gray), H.block_variances(gray)
    assert (es == F(30.0)).any() and (diff == F(30.0)).any() and (diff == F(10.0)).any()
    for t in (100, 500, 1000, 2000, 5000):
        assert (bv == F(t)).any(), t
    got = gpu_ctx.image_heuristics(img, w, h)
    want = _check(got, img, w, h, "thresholds")
    # the strict / non-strict comparisons decide these: a variance on 1000 is mid but not "> 1000", ...
    assert want["mid_var_block_pct"] > 0 and want["high_var_block_pct"] > 0 and want["detail_block_pct"] > 0
    assert want["analyze_detail_block_pct"] < want["mid_var_block_pct"] + want["high_var_block_pct"] + want["detail_block_pct"]


def test_every_entry_point_gives_the_same_struct(ce, gpu_ctx):
    w, h = 768, 512
    imgs = [_noise(w, h, 50 + i) if i % 3 else _gradient(w, h) ^ np.uint8(i) for i in range(64)]
    one = [gpu_ctx.image_heuristics(im, w, h) for im in imgs]
    b = ce.Batch(gpu_ctx, w, h, 64, 64)
    try:
        for i, im in enumerate(imgs):
            b.set_reference(63 - i, im)
            b.set_test(i, 63 - i, im)
        refs = b.image_heuristics(0, 64)
        tests = b.image_heuristics(0, 64, tests=True)
        assert [refs[63 - i] for i in range(64)] == one
        assert tests == one
        assert b.image_heuristics(17, 1) == [one[63 - 17]]
        assert b.image_heuristics(5, 3, tests=True) == one[5:8]
    finally:
        b.close()
    r = ce.ReferenceHandle(gpu_ctx, imgs[9], w, h)
    try:
        assert r.image_heuristics() == one[9]
        r.compare_many([imgs[1]] * 3, ce.MetricConfig.all())  # grows the handle's batch: the reference moves with it
        assert r.image_heuristics() == one[9]
    finally:
        r.close()
    assert gpu_ctx.image_heuristics(imgs[9], w, h) == one[9]


def test_after_ingest_formats_and_tables(ce, gpu_ctx):
    w, h = 131, 97
    rgb = _noise(w, h, 3)
    rgba = np.concatenate([rgb, np.full((h, w, 1), 77, np.uint8)], axis=2)
    wide = np.random.default_rng(4).integers(0, 1024, (h, w, 3), dtype=np.uint16)
    wide8 = np.minimum((wide.astype(np.uint32) * 255 + 512) // 1023, 255).astype(np.uint8)  # avif_config.rs:122-170
    table = ce.ColorTable(gpu_ctx, 255 - ce.ColorTable.identity_cube())
    b = ce.Batch(gpu_ctx, w, h, 4, 2)
    try:
        b.set_reference_fmt(0, rgba, ce.PIXEL_RGBA8)
        b.set_reference_fmt(1, wide, ce.PIXEL_RGB16_10BIT)
        b.set_reference_lut(2, rgb, ce.PIXEL_RGB8, table)
        b.set_reference(3, rgb)
        b.set_test_lut(0, 0, rgba, ce.PIXEL_RGBA8, table)
        b.set_test(1, 1, wide8)
        got = b.image_heuristics(0, 4)
        for g, want in zip(got, (rgb, wide8, 255 - rgb, rgb)):
            _check(g, want, w, h, "ingest")
        got_t = b.image_heuristics(0, 2, tests=True)
        _check(got_t[0], 255 - rgb, w, h, "ingest test lut")
        assert got_t[1] == got[1]
    finally:
        b.close()
        table.close()


def test_no_interference_with_a_launch(ce, gpu_ctx, workloads):
    w, h = 192, 128
    refs = [workloads.make_reference(w, h, 11 + i) for i in range(2)]
    tests = [workloads.distort(refs[i % 2], 60 + 10 * i) for i in range(4)]
    cfg = ce.MetricConfig.all()

    def run(between):
        b = ce.Batch(gpu_ctx, w, h, 2, 4)
        try:
            for i, r in enumerate(refs):
                b.set_reference(i, r)
            for i, t in enumerate(tests):
                b.set_test(i, i % 2, t)
            b.launch(4, cfg, butteraugli_diffmap=True, ssimulacra2_maps=True)
            heur = between(b)
            s = b.collect(4)
            scores = [(x.dssim, x.ssimulacra2, x.butteraugli, x.psnr, x.valid, x.status) for x in s]
            maps = (b.butteraugli_diffmaps(0, 4), b.dssim_ssim_maps(0, 0, 4), b.ssimulacra2_maps(0, 1, 0, 0, 4))
            return scores, maps, heur
        finally:
            b.close()

    s0, m0, _ = run(lambda b: None)
    s1, m1, heur = run(lambda b: (b.image_heuristics(0, 2), b.image_heuristics(0, 4, tests=True)))
    assert s0 == s1
    np.testing.assert_array_equal(m0[0], m1[0])
    for a, c in zip(m0[1:], m1[1:]):
        np.testing.assert_array_equal(a[0], c[0])
        np.testing.assert_array_equal(a[1], c[1])
    for g, im in zip(heur[0] + heur[1], refs + tests):
        _check(g, im, w, h, "between launch and collect")


def test_error_codes(ce, gpu_ctx):
    L = ce.lib()
    out = ce.CeImageHeuristics()
    for w, h in ((2, 5), (5, 2), (1, 9), (2, 2)):
        a = np.zeros(w * h * 3, np.uint8)
        assert L.ce_image_heuristics_rgb8(gpu_ctx._h, a.ctypes.data, a.size, w, h, ctypes.byref(out)) == ce.CE_ERR_TOO_SMALL
    a = np.zeros(9 * 9 * 3, np.uint8)
    assert L.ce_image_heuristics_rgb8(gpu_ctx._h, a.ctypes.data, a.size - 1, 9, 9, ctypes.byref(out)) == ce.CE_ERR_BAD_LENGTH
    assert L.ce_image_heuristics_rgb8(gpu_ctx._h, a.ctypes.data, a.size, 9, 8, ctypes.byref(out)) == ce.CE_ERR_BAD_LENGTH
    with pytest.raises(ce.MetricCalculation):
        gpu_ctx.image_heuristics(np.zeros(2 * 9 * 3, np.uint8), 2, 9)
    b = ce.Batch(gpu_ctx, 9, 9, 3, 2)
    try:
        arr = (ce.CeImageHeuristics * 4)()
        for which, first, count in ((0, 0, 0), (0, 3, 1), (0, 2, 2), (1, 0, 3), (1, 2, 1), (2, 0, 1), (0, 4, 0xFFFFFFFF)):
            assert L.ce_batch_image_heuristics(b._h, which, first, count, arr) == ce.CE_ERR_INVALID_ARG, (which, first, count)
        assert L.ce_batch_image_heuristics(b._h, 0, 0, 3, arr) == ce.CE_OK
        assert L.ce_batch_image_heuristics(b._h, 1, 0, 2, arr) == ce.CE_OK
    finally:
        b.close()
    small = ce.Batch(gpu_ctx, 2, 8, 1, 1)
    try:
        assert L.ce_batch_image_heuristics(small._h, 0, 0, 1, ctypes.byref(out)) == ce.CE_ERR_TOO_SMALL
    finally:
        small.close()
    r = ce.ReferenceHandle(gpu_ctx, np.zeros(8 * 2 * 3, np.uint8), 8, 2)
    try:
        assert L.ce_ref_image_heuristics(r._h, ctypes.byref(out)) == ce.CE_ERR_TOO_SMALL
    finally:
        r.close()


def test_gap_to_the_reference_sequential_sums(ce, gpu_ctx, workloads):
    """The Tier B deviation the ledger records: device vs the reference's own sequential f32 sums."""
    import os

    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "inputs.npz"))
    imgs = [(d[n], n) for n in d.files]
    imgs += [(workloads.make_reference(w, h, 3000 + i), f"bench {w}x{h} #{i}") for i, (w, h) in
             enumerate([(768, 512), (512, 768), (512, 512), (512, 512)])]
    worst = {}
    for img, name in imgs:
        h, w = img.shape[:2]
        got = gpu_ctx.image_heuristics(img, w, h)
        seq = H.compute(img, w, h, "seq_f32")
        for f in H.TIER_B:
            g, s = float(getattr(got, f)), float(seq[f])
            gap = abs(g - s)
            rel = gap / abs(s) if gap else 0.0
            if rel > worst.get(f, (0.0, 0.0, ""))[0]:
                worst[f] = (rel, gap, name)
            assert gap <= LEDGER_REL_GAP * abs(s) or gap <= LEDGER_ABS_GAP, (name, f, g, s)
        for f in H.TIER_A:
            assert F(getattr(got, f)) == seq[f], (name, f)
    print("\nlargest gap to the sequential f32 sums per field (relative, absolute):")
    for f, (rel, gap, name) in sorted(worst.items(), key=lambda kv: -kv[1][0]):
        print(f"  {f:24s} {rel:.3e} {gap:.3e}  ({name})")
