"""EvalConfig.alpha_backgrounds without a device: the session's slot layout, the worst-per-metric rule and the per-background
scores it keeps, against a stand-in batch that composites with the restatement and scores by mean squared error; the
device-free multi-device sweep (host composite, injected scorer) gives the same rows; None changes nothing.  The ctypes
layer refuses null handles for the four new entry points."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_restatement as A  # noqa: E402

W, H = 8, 6


def _mse_scores(ce, ref, test):
    mse = float(np.mean((ref.astype(np.int64) - test.astype(np.int64)) ** 2))
    s = ce.CeScores()
    s.status, s.valid = 0, 15
    s.dssim, s.butteraugli, s.ssimulacra2, s.psnr = mse / 100, mse / 10, 100 - mse, 99 - mse
    return s


@pytest.fixture
def fake(ce, monkeypatch):
    S = importlib.import_module("codec-eval_amd.session")

    class FakeCtx:
        def memory_info(self):
            return (1 << 34, 1 << 34)

        def _err(self):
            return ""

    class FakeBatch:
        made = []

        def __init__(self, ctx, w, h, n_refs, n_pairs, depths=None):
            self.depths = depths
            self.refs, self.tests, self.bind = [None] * n_refs, [None] * n_pairs, [None] * n_pairs
            FakeBatch.made.append((w, h, n_refs, n_pairs, depths))

        @staticmethod
        def _rgb(px, fmt):
            return np.asarray(px).reshape(-1, 4 if fmt in (ce.PIXEL_RGBA8, ce.PIXEL_RGBA16) else 3)[:, :3]

        def set_reference_fmt(self, i, px, fmt):
            self.refs[i] = self._rgb(px, fmt)

        def set_test_lut(self, k, r, px, fmt, table):
            self.tests[k], self.bind[k] = self._rgb(px, fmt), r

        def set_reference_over(self, first, px, fmt, bgs):
            for k, bg in enumerate(bgs):
                self.refs[first + k] = A.composite(np.asarray(px).reshape(-1, 4), bg, self.depths[0] if self.depths else 8)

        def set_test_over(self, first, refs, px, fmt, bgs):
            assert len(refs) == len(bgs)
            for k, bg in enumerate(bgs):
                self.tests[first + k] = A.composite(np.asarray(px).reshape(-1, 4), bg, self.depths[1] if self.depths else 8)
                self.bind[first + k] = refs[k]

        def run(self, n, cfg):
            return [_mse_scores(ce, self.refs[self.bind[k]], self.tests[k]) for k in range(n)]

        def close(self):
            pass

    monkeypatch.setattr(S, "Batch", FakeBatch)
    monkeypatch.setattr(S, "estimate_batch_bytes", lambda *a: 1000)

    def run(source, decodes, bgs):
        FakeBatch.made = []
        cfg = S.EvalConfig.builder().report_dir("unused").quality_levels(sorted(decodes)).alpha_backgrounds(bgs).build()
        ses = S.EvalSession(cfg, ctx=FakeCtx())
        ses.add_codec_with_decode("c", "1", lambda im, rq: b"%d" % int(rq.quality), lambda blob: decodes[int(blob)])
        rep = ses.evaluate_image("x", source)
        return rep, [(r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in rep.results], list(FakeBatch.made)

    return S, run


def test_session_slots_worst_value_and_per_background_scores(ce, fake):
    S, run = fake
    rng = np.random.default_rng(0)
    src = A.random_rgba(rng, W, H)
    dec = {40: S.ImageData.rgba(A.random_rgba(rng, W, H), W, H), 80: S.ImageData.rgb(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), W, H)}
    rgba_src, rgb_src = S.ImageData.rgba(src, W, H), S.ImageData.rgb(np.ascontiguousarray(src[..., :3]), W, H)
    assert S.EvalConfig("x").alpha_backgrounds is None and S.ALPHA_BLACK_WHITE == ((0, 0, 0), (255, 255, 255))
    rep, rows0, made = run(rgba_src, dec, None)  # None: one slot per image, alpha dropped, nothing kept
    assert made == [(W, H, 1, 2, None)] and rep.alpha_scores == {}
    assert rows0[0][1] == 100 - float(np.mean((src[..., :3].astype(np.int64) - dec[40].data.reshape(H, W, 4)[..., :3].astype(np.int64)) ** 2))
    rep, rows, made = run(rgba_src, dec, S.ALPHA_BLACK_WHITE)  # a source with alpha: every pair over both backgrounds
    assert made == [(W, H, 2, 4, None)] and sorted(rep.alpha_scores) == [0, 1]
    for i, q in enumerate((40, 80)):
        want = [_mse_scores(ce, A.composite(src, bg), A.composite(dec[q].data.reshape(H, W, 4), bg) if q == 40 else dec[q].data.reshape(H, W, 3))
                for bg in S.ALPHA_BLACK_WHITE]
        assert [(m.dssim, m.ssimulacra2, m.butteraugli, m.psnr) for m in rep.alpha_scores[i]] == [(s.dssim, s.ssimulacra2, s.butteraugli, s.psnr) for s in want]
        assert rows[i] == (max(s.dssim for s in want), min(s.ssimulacra2 for s in want), max(s.butteraugli for s in want), min(s.psnr for s in want))
    assert "alpha" not in str(rep.to_obj())
    rep, _, made = run(rgb_src, dec, S.ALPHA_BLACK_WHITE)  # an opaque source: one reference slot; only the decode with alpha fans out
    assert made == [(W, H, 1, 3, None)] and sorted(rep.alpha_scores) == [0]
    rep, rows_rgb, made = run(rgb_src, {80: dec[80]}, S.ALPHA_BLACK_WHITE)  # no alpha anywhere: no extra slots
    assert made == [(W, H, 1, 1, None)] and rep.alpha_scores == {} and rows_rgb == run(rgb_src, {80: dec[80]}, None)[1]
    deep = {50: S.ImageData.rgba16(A.random_rgba(rng, W, H, 10), W, H, 10)}  # each side's backgrounds at its own depth
    rep, rows, made = run(rgba_src, deep, S.ALPHA_BLACK_WHITE)
    assert made == [(W, H, 2, 2, (8, 10))]
    want = [_mse_scores(ce, A.composite(src, bg), A.composite(deep[50].data.reshape(H, W, 4), A.scale_background(bg, 10), 10)) for bg in S.ALPHA_BLACK_WHITE]
    assert [m.ssimulacra2 for m in rep.alpha_scores[0]] == [s.ssimulacra2 for s in want]
    for bad in ([], [(0, 0, 0)] * 9, [(0, 0, 256)], [(0, 0)]):
        with pytest.raises(ValueError):
            S.EvalConfig.builder().alpha_backgrounds(bad)


def test_multidevice_sweep_composites_on_the_host(ce, fake):
    S, run = fake
    md = importlib.import_module("codec-eval_amd.multidevice")
    rng = np.random.default_rng(1)
    src = A.random_rgba(rng, W, H)
    dec = {40: S.ImageData.rgba(A.random_rgba(rng, W, H), W, H), 80: S.ImageData.rgb(rng.integers(0, 256, (H, W, 3), dtype=np.uint8), W, H)}

    def scorer(worker, jobs):
        for j in jobs:
            j.scores = [_mse_scores(ce, j.reference, t) for t in j.tests]

    pool = md.DevicePool(scorer=scorer, mock_workers=2)
    images = [("x", S.ImageData.rgba(src, W, H)), ("y", S.ImageData.rgb(np.ascontiguousarray(src[..., :3]), W, H))]

    def sweep(bgs):
        cfg = S.EvalConfig.builder().report_dir("unused").quality_levels([40, 80]).alpha_backgrounds(bgs).build()
        multi = md.MultiDeviceEvalSession(cfg, pool=pool)
        multi.add_codec_with_decode("c", "1", lambda im, rq: b"%d" % int(rq.quality), lambda blob: dec[int(blob)])
        return multi.evaluate_corpus("c", images)[0]

    corpus = sweep(S.ALPHA_BLACK_WHITE)
    for (name, image), report in zip(images, corpus.images):
        assert [(r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in report.results] == run(image, dec, S.ALPHA_BLACK_WHITE)[1], name
    assert sorted(corpus.images[0].alpha_scores) == [0, 1] and sorted(corpus.images[1].alpha_scores) == [0]
    plain = sweep(None)
    for (name, image), report in zip(images, plain.images):
        assert report.alpha_scores == {}
        assert [(r.dssim, r.ssimulacra2, r.butteraugli, r.psnr) for r in report.results] == run(image, dec, None)[1], name
    # the deep host composite: at the image's depth, then to_8bit's rule
    d10 = A.random_rgba(rng, W, H, 10)
    got = S.ImageData.rgba16(d10, W, H, 10).composited_rgb8_vec((255, 255, 255))
    want = A.composite(d10, (1023,) * 3, 10).astype(np.uint64)
    assert np.array_equal(got, np.minimum((want * 255 + 511) // 1023, 255).astype(np.uint8).reshape(-1))


def test_ctypes_layer_binds_the_new_entry_points(ce):
    L = ce.lib()
    px, bg, refs, out = np.zeros(16, np.uint8), np.zeros(3, np.uint16), np.zeros(1, np.uint32), np.zeros(12, np.uint8)
    assert L.ce_batch_set_reference_over(None, 0, px.ctypes.data, 16, ce.PIXEL_RGBA8, 1, bg.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_set_test_over(None, 0, refs.ctypes.data, px.ctypes.data, 16, ce.PIXEL_RGBA8, 1, bg.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_composite_rgba8(None, px.ctypes.data, 16, 2, 2, out.ctypes.data, out.ctypes.data, 12) == ce.CE_ERR_INVALID_ARG
    assert L.ce_composite_rgba16(None, px.ctypes.data, 8, 2, 1, 10, bg.ctypes.data, out.ctypes.data, 6) == ce.CE_ERR_INVALID_ARG
    for name in ("ce_batch_set_reference_over", "ce_batch_set_test_over", "ce_composite_rgba8", "ce_composite_rgba16"):
        assert name in ce.ABI_SYMBOLS
