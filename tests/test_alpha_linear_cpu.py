"""Linear-light compositing without a device: ce_alpha_table against numpy, hand-derived cases of the restatement
(tests/alpha_linear_restatement.py), the binding's signatures against the header, EvalConfig.alpha_blend's default and every
session refusal that stays, and the session's slot layout under ALPHA_BLEND_LINEAR against a stand-in batch that blends with
the restatement."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_linear_restatement as A  # noqa: E402
import cicp_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 8, 6
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


@pytest.mark.parametrize("depth", A.DEPTHS)
def test_alpha_table_is_one_f32_division_per_entry(ce, depth):
    m = (1 << depth) - 1
    want = np.array([np.float32(k) / np.float32(m) for k in range(m + 1)], np.float32)
    got = ce.alpha_table(depth)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(A.alpha_table(depth).view(np.uint32), want.view(np.uint32))
    assert got[0] == 0.0 and got[m] == 1.0 and np.all(np.diff(got) > 0)


def test_alpha_table_refuses_what_it_cannot_build(ce):
    out = np.empty(256, np.float32)
    for depth, n in ((9, 512), (0, 1), (8, 255), (16, 256)):
        assert ce.lib().ce_alpha_table(depth, out.ctypes.data, n) == ce.CE_ERR_INVALID_ARG
    assert ce.lib().ce_alpha_table(8, None, 256) == ce.CE_ERR_INVALID_ARG


def test_hand_derived_cases_of_the_restatement():
    bg = np.array([0.25, -0.5, 2.0], F)
    v = np.array([[-0.0, 0.5, 1024.0]], F)
    # a = m gives v on every bit, -0.0 included; a = 0 gives bg on every bit
    for depth in A.DEPTHS:
        m = (1 << depth) - 1
        assert np.array_equal(bits(A.over_int(v, np.array([m]), depth, [bg])), bits(v))
        assert np.array_equal(bits(A.over_int(v, np.array([0]), depth, [bg])), bits(bg))
        assert np.array_equal(bits(A.over_int(v, np.array([0]), depth, [[-0.0, 0.0, -0.0]])), bits(np.array([-0.0, 0.0, -0.0], F)))
    # white over black at a = 128 / 255: atab[128] of the light, not the sRGB decode of code 128
    white = np.ones((1, 3), F)
    got = A.over_int(white, np.array([128]), 8, [[0.0, 0.0, 0.0]])[0, 0]
    t = F(128) / F(255)
    assert np.array_equal(bits(got), bits(np.full(3, t, F)))
    assert abs(float(got[0]) - 0.50196) < 1e-5 and abs(float(R.transfer_table(13, 8)[128]) - 0.21586) < 1e-5
    # the general blend: two products and one sum, each rounded to f32
    c, b, a = F(0.7), F(0.3), 77
    t = F(a) / F(255)
    u = F(1.0) - t
    assert A.over_int(np.full((1, 3), c, F), np.array([a]), 8, [[b, b, b]])[0, 0, 0] == F(F(c * t) + F(b * u))
    # alpha above m is clamped to m at depths 10 and 12: the pixel is opaque
    for depth in (10, 12):
        m = (1 << depth) - 1
        for a in (m + 1, 4 * m, 65535):
            assert np.array_equal(bits(A.over_int(v, np.array([a]), depth, [bg])), bits(v))
    # step 4: the clamp acts on the blend
    big = A.over_int(np.full((1, 3), 1024.0, F), np.array([254]), 8, [[1024.0, 1024.0, 1024.0]])
    assert np.all(big <= 1024.0)


def test_hand_derived_cases_of_the_float_form():
    bg = np.array([0.25, -0.5, 2.0], F)
    px = lambda r, g, b, a: np.array([[r, g, b, a]], F)
    # alpha NaN, below 0 and -0.0 hide the pixel; above 1 is opaque; the samples get the clamp of a linear image
    for a in (np.nan, -3.0, -0.0, 0.0):
        assert np.array_equal(bits(A.over_f32(px(0.5, 0.6, 0.7, a), False, [bg])), bits(bg)), a
    for a in (1.0, 1.5, np.inf):
        assert np.array_equal(bits(A.over_f32(px(np.nan, 5000.0, -0.0, a), False, [bg])), bits(np.array([0.0, 1024.0, -0.0], F))), a
    half = A.over_f32(px(1.0, 0.0, 0.5, 0.5), False, [bg])[0, 0]
    assert np.array_equal(bits(half), bits(np.array([0.625, -0.25, 1.25], F)))
    # premultiplied: o = v + bg * u, v as it is where u == 0
    pre = A.over_f32(px(0.5, 0.0, 0.25, 0.5), True, [bg])[0, 0]
    assert np.array_equal(bits(pre), bits(np.array([0.625, -0.25, 1.25], F)))
    assert np.array_equal(bits(A.over_f32(px(-0.0, 0.3, 9.0, 1.0), True, [bg])), bits(np.array([-0.0, 0.3, 9.0], F)))
    assert np.array_equal(bits(A.over_f32(px(0.0, 0.0, 0.0, 0.0), True, [bg])), bits(bg))
    assert np.array_equal(bits(A.over_f32(px(0.1, 0.1, 0.1, np.nan), True, [bg])), bits(np.array([0.1, 0.1, 0.1], F) + bg))


NEW = ("ce_alpha_table", "ce_batch_set_reference_cicp_over", "ce_batch_set_test_cicp_over", "ce_batch_set_reference_hlg_over",
       "ce_batch_set_test_hlg_over", "ce_batch_set_reference_icc_over", "ce_batch_set_test_icc_over", "ce_batch_set_reference_linear_over",
       "ce_batch_set_test_linear_over", "ce_cicp_over_to_linear", "ce_hlg_over_to_linear", "ce_icc_over_to_linear", "ce_linear_over")


def test_binding_signatures_and_constants(ce):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ce_metrics.h")).read(), flags=re.S)
    protos = {p[0]: p for p in ce._PROTOTYPES}
    hpp = open(os.path.join(ROOT, "codec-eval_amd", "host", "codec_eval.hpp")).read()
    rust = open(os.path.join(ROOT, "bindings", "rust", "codec-eval-hip", "src", "lib.rs")).read()
    for name in NEW:
        m = re.search(r"\b" + name + r"\(([^;{]*?)\);", header, flags=re.S)
        assert m, name
        assert len(protos[name][2]) == len([a for a in m.group(1).split(",") if a.strip()]), name
        assert name in ce.ABI_SYMBOLS and hasattr(ce.lib(), name)
        assert name + "(" in hpp and "sys::" + name + "(" in rust or name == "ce_alpha_table", name
    assert ce.PIXEL_RGBA_F32 == 8 == int(re.search(r"CE_PIXEL_RGBA_F32\s*=\s*(\d+)", header).group(1))
    assert ce.lib().ce_pixel_bytes(ce.PIXEL_RGBA_F32) == 0  # not a format of ce_batch_set_*_fmt
    assert ce.MAX_BACKGROUNDS == A.MAX_BACKGROUNDS == int(re.search(r"#define CE_MAX_BACKGROUNDS (\d+)", header).group(1))
    for method in ("set_reference_cicp_over", "set_test_cicp_over", "set_reference_hlg_over", "set_test_hlg_over", "set_reference_icc_over",
                   "set_test_icc_over", "set_reference_linear_over", "set_test_linear_over"):
        assert callable(getattr(ce.Batch, method))
    for method in ("cicp_over_to_linear", "hlg_over_to_linear", "icc_over_to_linear", "linear_over"):
        assert callable(getattr(ce.Context, method))


def test_null_handles_are_refused_by_every_entry_point(ce):
    L = ce.lib()
    px, bg, refs, out = np.zeros(64, np.uint8), np.zeros(3, np.float32), np.zeros(1, np.uint32), np.zeros(12, np.float32)
    c, h = ce.CeColour(1, 13, 8, 203.0), ce.CeHlg(9, 8, 1000.0, 0.0, 203.0)
    p, b, r, o = px.ctypes.data, bg.ctypes.data, refs.ctypes.data, out.ctypes.data
    assert L.ce_batch_set_reference_cicp_over(None, 0, p, 16, ce.PIXEL_RGBA8, c, 1, b) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_set_test_cicp_over(None, 0, r, p, 16, ce.PIXEL_RGBA8, c, 1, b) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_set_reference_hlg_over(None, 0, p, 16, ce.PIXEL_RGBA8, h, 1, b) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_set_test_hlg_over(None, 0, r, p, 16, ce.PIXEL_RGBA8, h, 1, b) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_set_reference_icc_over(None, 0, p, 16, ce.PIXEL_RGBA8, 8, None, 1, b) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_set_test_icc_over(None, 0, r, p, 16, ce.PIXEL_RGBA8, 8, None, 1, b) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_set_reference_linear_over(None, 0, p, 64, ce.PIXEL_RGBA_F32, 0, 1, b) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_set_test_linear_over(None, 0, r, p, 64, ce.PIXEL_RGBA_F32, 0, 1, b) == ce.CE_ERR_INVALID_ARG
    assert L.ce_cicp_over_to_linear(None, p, 16, ce.PIXEL_RGBA8, c, 2, 2, b, o, 12) == ce.CE_ERR_INVALID_ARG
    assert L.ce_hlg_over_to_linear(None, p, 16, ce.PIXEL_RGBA8, h, 2, 2, b, o, 12) == ce.CE_ERR_INVALID_ARG
    assert L.ce_icc_over_to_linear(None, p, 16, ce.PIXEL_RGBA8, 8, None, 2, 2, b, o, 12) == ce.CE_ERR_INVALID_ARG
    assert L.ce_linear_over(None, p, 64, ce.PIXEL_RGBA_F32, 0, 2, 2, b, o, 12) == ce.CE_ERR_INVALID_ARG


def _mse_scores(ce, ref, test):
    mse = float(np.mean((ref.astype(np.float64) - test.astype(np.float64)) ** 2))
    s = ce.CeScores()
    s.status, s.valid = 0, 7
    s.dssim, s.butteraugli, s.ssimulacra2, s.psnr = mse / 100, mse / 10, 100 - mse, 0.0
    return s


@pytest.fixture
def fake(ce, monkeypatch):
    """A session over a stand-in linear batch: sRGB-tagged code values and float images, blended with the restatement."""
    S = importlib.import_module("codec-eval_amd.session")

    class FakeCtx:
        def memory_info(self):
            return (1 << 34, 1 << 34)

        def _err(self):
            return ""

    class FakeBatch:
        made, calls = [], []

        def __init__(self, ctx, w, h, n_refs, n_pairs, depths=None, linear=False):
            assert linear
            self.refs, self.tests, self.bind = [None] * n_refs, [None] * n_pairs, [None] * n_pairs
            FakeBatch.made.append((w, h, n_refs, n_pairs))

        @staticmethod
        def _lin(px, colour):
            return R.to_linear(np.asarray(px), colour.primaries, colour.transfer, colour.depth, colour.white_nits)

        def set_reference_cicp(self, i, px, colour):
            FakeBatch.calls.append("ref_cicp")
            self.refs[i] = self._lin(px, colour)

        def set_test_cicp(self, k, r, px, colour):
            FakeBatch.calls.append("test_cicp")
            self.tests[k], self.bind[k] = self._lin(px, colour), r

        def set_reference(self, i, data):
            self.refs[i] = np.asarray(data, np.float32).reshape(H, W, 3)

        def set_test(self, k, r, data):
            self.tests[k], self.bind[k] = np.asarray(data, np.float32).reshape(H, W, 3), r

        def set_reference_cicp_over(self, first, px, colour, bgs):
            FakeBatch.calls.append("ref_cicp_over")
            for k, o in enumerate(A.over_int(self._lin(px, colour), np.asarray(px)[..., 3], colour.depth, bgs)):
                self.refs[first + k] = o

        def set_test_cicp_over(self, first, refs, px, colour, bgs):
            FakeBatch.calls.append("test_cicp_over")
            assert len(refs) == len(bgs)
            for k, o in enumerate(A.over_int(self._lin(px, colour), np.asarray(px)[..., 3], colour.depth, bgs)):
                self.tests[first + k], self.bind[first + k] = o, refs[k]

        def set_reference_linear_over(self, first, px, bgs, premultiplied=False):
            FakeBatch.calls.append("ref_linear_over")
            for k, o in enumerate(A.over_f32(px, premultiplied, bgs)):
                self.refs[first + k] = o

        def set_test_linear_over(self, first, refs, px, bgs, premultiplied=False):
            FakeBatch.calls.append("test_linear_over")
            for k, o in enumerate(A.over_f32(px, premultiplied, bgs)):
                self.tests[first + k], self.bind[first + k] = o, refs[k]

        def run(self, n, cfg):
            return [_mse_scores(ce, self.refs[self.bind[k]], self.tests[k]) for k in range(n)]

        def close(self):
            pass

    monkeypatch.setattr(S, "Batch", FakeBatch)
    monkeypatch.setattr(S, "estimate_batch_bytes", lambda *a: 1000)

    def run(source, decodes, bgs, blend):
        FakeBatch.made, FakeBatch.calls = [], []
        cfg = S.EvalConfig.builder().report_dir("unused").quality_levels(sorted(decodes)).alpha_backgrounds(bgs).alpha_blend(blend).build()
        ses = S.EvalSession(cfg, ctx=FakeCtx())
        ses.add_codec_with_decode("c", "1", lambda im, rq: b"%d" % int(rq.quality), lambda blob: decodes[int(blob)])
        rep = ses.evaluate_image("x", source)
        return rep, [(r.dssim, r.ssimulacra2, r.butteraugli) for r in rep.results], list(FakeBatch.made), list(FakeBatch.calls)

    return S, run


def rgba16(rng, depth=10):
    return rng.integers(0, 1 << depth, (H, W, 4)).astype(np.uint16)


def test_alpha_blend_defaults_to_none_and_every_refusal_stays(ce, fake):
    S, run = fake
    md = importlib.import_module("codec-eval_amd.multidevice")
    rng = np.random.default_rng(3)
    PQ = ce.ColourDescription(9, 16, 10, 203.0)
    src = S.ImageData.rgba16(rgba16(rng), W, H, 10, colour=PQ)
    dec = {50: S.ImageData.rgba16(rgba16(rng), W, H, 10, colour=PQ)}
    assert S.EvalConfig("x").alpha_blend is None and S.EvalConfig.builder().report_dir("x").build().alpha_blend is None
    assert S.ALPHA_BLEND_LINEAR == "linear"
    with pytest.raises(ValueError):
        S.EvalConfig.builder().alpha_blend("gamma")
    # without the knob: alpha is dropped without backgrounds, and the pair is refused with them, word for word
    rep, _, made, calls = run(src, dec, None, None)
    assert made == [(W, H, 1, 1)] and calls == ["ref_cicp", "test_cicp"] and rep.alpha_scores == {}
    with pytest.raises(ce.MetricCalculation, match="linear-light scoring: alpha_backgrounds with a colour description is not supported"):
        run(src, dec, S.ALPHA_BLACK_WHITE, None)
    # the knob without backgrounds changes nothing
    assert run(src, dec, None, S.ALPHA_BLEND_LINEAR)[1:] == run(src, dec, None, None)[1:]
    # a float RGBA image has nothing else to be: it needs both
    frgba = S.ImageData.linear_f32(rng.random((H, W, 4), np.float32), W, H, channels=4)
    for bgs, blend in ((None, None), (None, S.ALPHA_BLEND_LINEAR)):
        with pytest.raises(ce.MetricCalculation, match="float RGBA"):
            run(frgba, {50: frgba}, bgs, blend)
    with pytest.raises(ce.MetricCalculation, match="alpha_backgrounds with a colour description"):
        run(frgba, {50: frgba}, S.ALPHA_BLACK_WHITE, None)
    with pytest.raises(ValueError):
        S.ImageData.linear_f32(np.zeros((H, W, 3), np.float32), W, H, premultiplied=True)
    with pytest.raises(ValueError):
        S.ImageData.linear_f32(np.zeros((H, W, 3), np.float32), W, H, channels=4)
    # gain-map images with alpha stay refused, with a message that says so
    gm = ce.GainMap(np.full((2, 2), 128, np.uint8))
    with_map = S.ImageData.rgba(rng.integers(0, 256, (H, W, 4), dtype=np.uint8), W, H, gain_map=gm)
    with pytest.raises(ce.MetricCalculation, match="gain-map image with alpha"):
        run(src, {50: with_map}, S.ALPHA_BLACK_WHITE, S.ALPHA_BLEND_LINEAR)
    # a description together with an ICC profile stays refused
    both = S.ImageData.rgba16(rgba16(rng), W, H, 10, colour=PQ)
    both.icc_profile = b"profile"
    with pytest.raises(ce.MetricCalculation, match="ICC profile"):
        run(src, {50: both}, S.ALPHA_BLACK_WHITE, S.ALPHA_BLEND_LINEAR)
    # the multi-device session refuses the knob with a message of its own
    cfg = S.EvalConfig.builder().report_dir("unused").alpha_backgrounds(S.ALPHA_BLACK_WHITE).alpha_blend(S.ALPHA_BLEND_LINEAR).build()
    with pytest.raises(ValueError, match="MultiDeviceEvalSession does not take alpha_blend"):
        md.MultiDeviceEvalSession(cfg, pool=md.DevicePool(scorer=lambda w, j: None, mock_workers=1))


def test_session_fans_linear_pairs_over_the_backgrounds(ce, fake):
    S, run = fake
    rng = np.random.default_rng(4)
    PQ = ce.ColourDescription(9, 16, 10, 203.0)
    bgs = S.ALPHA_BLACK_WHITE
    lin = ce.srgb_table(8, 0)[np.asarray(bgs)]
    assert lin.dtype == np.float32 and lin.tolist() == [[0.0] * 3, [1.0] * 3]
    src_px, dec_px, opaque_px = rgba16(rng), rgba16(rng), np.ascontiguousarray(rgba16(rng)[..., :3])
    src, src_rgb = S.ImageData.rgba16(src_px, W, H, 10, colour=PQ), S.ImageData.rgb16(np.ascontiguousarray(src_px[..., :3]), W, H, 10, colour=PQ)
    dec = {40: S.ImageData.rgba16(dec_px, W, H, 10, colour=PQ), 80: S.ImageData.rgb16(opaque_px, W, H, 10, colour=PQ)}
    to_lin = lambda px: R.to_linear(px, 9, 16, 10, 203.0)
    # a source with alpha: one reference slot per background, every pair over both
    rep, rows, made, calls = run(src, dec, bgs, S.ALPHA_BLEND_LINEAR)
    assert made == [(W, H, 2, 4)] and calls == ["ref_cicp_over", "test_cicp_over", "test_cicp", "test_cicp"]
    assert sorted(rep.alpha_scores) == [0, 1]
    refs = A.over_int(to_lin(src_px), src_px[..., 3], 10, lin)
    tests = {40: A.over_int(to_lin(dec_px), dec_px[..., 3], 10, lin), 80: [to_lin(opaque_px)] * 2}
    for i, q in enumerate((40, 80)):
        want = [_mse_scores(ce, refs[k], tests[q][k]) for k in range(2)]
        assert [(m.dssim, m.ssimulacra2, m.butteraugli) for m in rep.alpha_scores[i]] == [(s.dssim, s.ssimulacra2, s.butteraugli) for s in want]
        assert rows[i] == (max(s.dssim for s in want), min(s.ssimulacra2 for s in want), max(s.butteraugli for s in want))
    # an opaque source: one reference slot; only the decode with alpha fans out
    rep, _, made, calls = run(src_rgb, dec, bgs, S.ALPHA_BLEND_LINEAR)
    assert made == [(W, H, 1, 3)] and calls == ["ref_cicp", "test_cicp_over", "test_cicp"] and sorted(rep.alpha_scores) == [0]
    # no alpha anywhere: no extra slots, the rows of a session without the knob
    only = {80: dec[80]}
    rep, rows, made, _ = run(src_rgb, only, bgs, S.ALPHA_BLEND_LINEAR)
    assert made == [(W, H, 1, 1)] and rep.alpha_scores == {} and rows == run(src_rgb, only, None, None)[1]
    # float RGBA, straight source and premultiplied decode
    f_src, f_dec = rng.random((H, W, 4), np.float32), rng.random((H, W, 4), np.float32)
    rep, rows, made, calls = run(S.ImageData.linear_f32(f_src, W, H, channels=4),
                                 {50: S.ImageData.linear_f32(f_dec, W, H, channels=4, premultiplied=True)}, bgs, S.ALPHA_BLEND_LINEAR)
    assert made == [(W, H, 2, 2)] and calls == ["ref_linear_over", "test_linear_over"]
    want = [_mse_scores(ce, A.over_f32(f_src, False, lin)[k], A.over_f32(f_dec, True, lin)[k]) for k in range(2)]
    assert [m.ssimulacra2 for m in rep.alpha_scores[0]] == [s.ssimulacra2 for s in want]
