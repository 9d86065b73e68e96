"""Gain-map images into a linear batch (include/ce_metrics.h: ce_batch_set_*_gainmap, ce_gainmap_to_linear; DESIGN.md section
21).  The definition - the base's transfer table, the map sampled around each pixel's centre, the host-built log2-gain
tables, the f64 interpolation, gm_exp2's fixed f64 sequence, the one rounding to f32, matrix and clamp - is restated in numpy
(tests/gainmap_restatement.py), and the device must equal it on every float, bit for bit; the scores of what it wrote must
equal those of the same floats taken in by the existing routes."""
import ctypes as C
import dataclasses
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import gainmap_restatement as G  # noqa: E402
from test_gainmap_cpu import gain_map  # noqa: E402
from test_gainmap_kernel_host_cpu import SHAPES  # noqa: E402
from test_gpu_deep_input import run_everything, same  # noqa: E402
from test_gpu_linear_input import golden, random_codes  # noqa: E402
from test_gpu_yuv_ingest import read_slab  # noqa: E402

pytestmark = pytest.mark.gpu

S = importlib.import_module("codec-eval_amd.session")
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
# sample type, channels and depths of the four formats
FORMATS = ((np.uint8, 3, (8,)), (np.uint8, 4, (8,)), (np.uint16, 3, R.DEPTHS), (np.uint16, 4, R.DEPTHS))
# an Ultra HDR-like description: a single-channel map of up to three stops over an sRGB base, the usual 1 / 64 offsets
ULTRA = G.Meta(gain_min=(0.0,) * 3, gain_max=(3.0,) * 3, gamma=(1.0,) * 3, base_offset=(1 / 64,) * 3, alternate_offset=(1 / 64,) * 3,
               base_headroom=0.0, alternate_headroom=3.0, display_headroom=3.0)


@pytest.mark.parametrize("base,gmap", SHAPES + (((257, 129), (65, 33)),))
def test_ingest_equals_the_restatement_bit_for_bit(ce, gpu_ctx, base, gmap):
    """Every format x map channels, the depth, primaries, transfer and metadata walking through their lists, into slots 0, 1
    and 2 of both slabs (odd shapes change the store width with the slot); the other slots are checked untouched, and
    ce_gainmap_to_linear returns the slot's floats."""
    (w, h), (gw, gh) = base, gmap
    rng = np.random.default_rng(w * 1000 + h + gw)
    n = w * h * 3
    b = gpu_ctx.batch_linear(w, h, 3, 3)
    try:
        slabs = [[rng.random((h, w, 3), np.float32) for _ in range(3)] for _ in range(2)]
        for i in range(3):
            b.set_reference(i, slabs[0][i])
            b.set_test(i, i, slabs[1][i])
        k = 0
        for dt, ch, depths in FORMATS:
            for channels in (1, 3):
                for prim in R.PRIMARIES:
                    depth, transfer, meta = depths[k % len(depths)], R.TRANSFERS[k % 3], G.METAS[k % len(G.METAS)]
                    slot, which = k % 3, (k // 3) % 2
                    k += 1
                    px = random_codes(rng, w, h, ch, dt, depth)
                    samples = rng.integers(0, 256, (gh, gw, channels)).astype(np.uint8)
                    colour, gm = ce.ColourDescription(prim, transfer, depth), gain_map(samples, meta)
                    want = G.to_linear(px, prim, transfer, depth, samples, meta)
                    if which == 0:
                        b.set_reference_gainmap(slot, px, colour, gm)
                    else:
                        b.set_test_gainmap(slot, (slot + 1) % 3, px, colour, gm)
                        assert b.pair_reference(slot) == (slot + 1) % 3
                    slabs[which][slot] = want
                    got = gpu_ctx.gainmap_to_linear(px, w, h, colour, gm)
                    assert got.shape == (h, w, 3) and np.array_equal(bits(got), bits(want)), (dt, ch, channels, depth, prim, transfer, meta)
                    for s, address in ((0, b.reference_slab), (1, b.test_slab)):
                        slab = read_slab(ce, address, 3 * n * 4).view(np.uint32)
                        assert np.array_equal(slab, np.concatenate([bits(x).reshape(-1) for x in slabs[s]])), (dt, ch, channels, depth, prim, s)
    finally:
        b.close()


def gain_map_pair(rng, ref, test, scale=4, channels=1):
    """a golden pair as two gain-map images: the bases as they are, one smooth random map of a `scale`-th of their size"""
    h, w = ref.shape[:2]
    gh, gw = -(-h // scale), -(-w // scale)
    coarse = rng.integers(0, 256, (-(-gh // 4) + 1, -(-gw // 4) + 1, channels)).astype(np.float64)
    samples = np.kron(coarse, np.ones((4, 4, 1)))[:gh, :gw]
    samples = np.clip(samples + rng.integers(-8, 9, samples.shape), 0, 255).astype(np.uint8)
    return samples


def hdr_everything(ce, batch, w, h):
    out = run_everything(ce, batch, 1, w, h)
    f = batch.hdr_fidelity(1)[0]
    out["hdr"] = np.array([f.pq_sse, f.itp_sum_q20, f.itp_max_q20], np.uint64)
    out["hdr_scores"] = np.array([f.pq_psnr, f.delta_e_itp_mean, f.delta_e_itp_max])
    maps, counts = batch.delta_e_itp_maps(0, 1, thresholds_q20=[1 << 18, 1 << 20, 1 << 22])
    out["itp_map"], out["itp_counts"] = maps, counts
    out["itp_map_b8"] = batch.delta_e_itp_maps(0, 1, block=8)[0]
    return out


def test_batch_leaf_and_direct_upload_agree(ce, gpu_ctx):
    """set_*_gainmap, ce_gainmap_to_linear's floats and the restated floats uploaded as CE_PIXEL_RGB_F32: == on every score of
    MetricConfig.all(), on hdr_fidelity, on the Delta E ITP maps and counts, on the Butteraugli diffmap and every other map."""
    ref, test = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    rng = np.random.default_rng(7)
    samples = gain_map_pair(rng, ref, test, channels=3)
    damaged = np.clip(samples.astype(np.int64) + rng.integers(-20, 21, samples.shape), 0, 255).astype(np.uint8)
    meta = G.METAS[1]
    colour = ce.ColourDescription.DISPLAY_P3
    gm_r, gm_t = gain_map(samples, meta), gain_map(damaged, meta)
    batches = [gpu_ctx.batch_linear(w, h, 1, 1) for _ in range(3)]
    try:
        batches[0].set_reference_gainmap(0, ref, colour, gm_r)
        batches[0].set_test_gainmap(0, 0, test, colour, gm_t)
        batches[1].set_reference(0, gpu_ctx.gainmap_to_linear(ref, w, h, colour, gm_r))
        batches[1].set_test(0, 0, gpu_ctx.gainmap_to_linear(test, w, h, colour, gm_t))
        batches[2].set_reference(0, G.to_linear(ref, 12, 13, 8, samples, meta))
        batches[2].set_test(0, 0, G.to_linear(test, 12, 13, 8, damaged, meta))
        a, b, c = (hdr_everything(ce, x, w, h) for x in batches)
        assert a["scores"][0][5] == 0 and (a["scores"][0][4] & 7) == 7 and a["scores"][0][1] < 100.0
        assert "diffmap" in a and a["hdr"][2] > 0
        same(a, b)
        same(a, c)
    finally:
        for x in batches:
            x.close()


@pytest.mark.parametrize("prim,transfer,depth", [(1, 13, 8), (9, 16, 10), (12, 13, 16)])
def test_weight_zero_writes_what_the_cicp_ingest_writes(ce, gpu_ctx, prim, transfer, depth):
    w, h = 33, 7
    rng = np.random.default_rng(depth)
    px = random_codes(rng, w, h, 3, np.uint8 if depth == 8 else np.uint16, depth)
    colour = ce.ColourDescription(prim, transfer, depth)
    gm = gain_map(rng.integers(0, 256, (3, 9, 3)).astype(np.uint8), G.METAS[2])
    assert ce.gainmap_weight(gm) == 0.0
    b = gpu_ctx.batch_linear(w, h, 2, 2)
    try:
        b.set_reference_cicp(0, px, colour)
        b.set_reference_gainmap(1, px, colour, gm)
        b.set_test_cicp(0, 0, px, colour)
        b.set_test_gainmap(1, 1, px, colour, gm)
        for address in (b.reference_slab, b.test_slab):
            slab = read_slab(ce, address, 2 * w * h * 12).view(np.uint32).reshape(2, -1)
            assert np.array_equal(slab[0], slab[1]) and np.array_equal(slab[0], bits(R.to_linear(px, prim, transfer, depth)).reshape(-1))
    finally:
        b.close()
    assert np.array_equal(bits(gpu_ctx.gainmap_to_linear(px, w, h, colour, gm)), bits(gpu_ctx.cicp_to_linear(px, w, h, colour)))


def test_gain_one_doubles_the_base(ce, gpu_ctx):
    w, h = 16, 7
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    gm = ce.GainMap(np.full((2, 5), 99, np.uint8), gain_min=1.0, gain_max=1.0, gamma=2.2, base_offset=0.0, alternate_offset=0.0)
    got = gpu_ctx.gainmap_to_linear(px, w, h, ce.ColourDescription.SRGB, gm)
    assert np.array_equal(bits(got), bits(np.float32(2.0) * ce.transfer_table(13, 8)[px]))


def test_setting_a_reference_again_rebuilds_its_state(ce, gpu_ctx):
    """The setter invalidates what the metrics keep of the references: after another map the scores are a fresh batch's, and
    Batch.ref_stats() shows one more build of every metric's reference side."""
    ref, test = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    rng = np.random.default_rng(11)
    first = gain_map_pair(rng, ref, test)
    second = np.ascontiguousarray(255 - first)
    colour, cfg = ce.ColourDescription.SRGB, ce.MetricConfig.all()
    row = lambda s: (s.status, s.valid, s.dssim, s.ssimulacra2, s.butteraugli)  # noqa: E731

    def fresh(samples):
        b = gpu_ctx.batch_linear(w, h, 1, 1)
        try:
            b.set_reference_gainmap(0, ref, colour, gain_map(samples, ULTRA))
            b.set_test_gainmap(0, 0, test, colour, gain_map(first, ULTRA))
            return row(b.run(1, cfg)[0])
        finally:
            b.close()

    want_first, want_second = fresh(first), fresh(second)
    assert want_first != want_second and want_first[0] == 0 and want_second[0] == 0
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        b.set_reference_gainmap(0, ref, colour, gain_map(first, ULTRA))
        b.set_test_gainmap(0, 0, test, colour, gain_map(first, ULTRA))
        assert row(b.run(1, cfg)[0]) == want_first and b.ref_stats() == (1, 1, 1)
        assert row(b.run(1, cfg)[0]) == want_first and b.ref_stats() == (1, 1, 1)
        b.set_test_gainmap(0, 0, test, colour, gain_map(first, ULTRA))  # a test image leaves the references' state alone
        assert row(b.run(1, cfg)[0]) == want_first and b.ref_stats() == (1, 1, 1)
        b.set_reference_gainmap(0, ref, colour, gain_map(second, ULTRA))
        assert row(b.run(1, cfg)[0]) == want_second and b.ref_stats() == (2, 2, 2)
    finally:
        b.close()


def test_refusals_leave_the_batch_usable(ce, gpu_ctx):
    w, h = 16, 10
    rng = np.random.default_rng(31)
    lib = ce.lib()
    px8, other8 = (rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2))
    px16 = rng.integers(0, 1024, (h, w, 3)).astype(np.uint16)
    f32 = rng.random((h, w, 3), np.float32)
    samples = rng.integers(0, 256, (5, 4, 3)).astype(np.uint8)
    meta = G.METAS[1]
    good = gain_map(samples, meta)
    c8, c10 = ce.CeColour(1, 13, 8, 203.0), ce.CeColour(9, 16, 10, 203.0)
    nan, inf = float("nan"), float("inf")
    out = np.empty(w * h * 3, np.float32)
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    plain, deep = ce.Batch(gpu_ctx, w, h, 1, 1), gpu_ctx.batch_deep(w, h, 1, 1, 16, 16)
    try:
        b.set_reference_gainmap(0, px8, ce.ColourDescription.SRGB, good)
        b.set_test_gainmap(0, 0, other8, ce.ColourDescription.SRGB, good)
        first = b.run(1, ce.MetricConfig.all())[0]
        assert first.status == 0 and first.valid == 7
        want = G.to_linear(px8, 1, 13, 8, samples, meta)

        def refused(rc, what):
            assert rc == ce.CE_ERR_INVALID_ARG, what
            assert gpu_ctx._err(), what

        def calls(px, n, fmt, colour, img, m):
            p = px.ctypes.data if px is not None else None
            return (lambda: lib.ce_batch_set_reference_gainmap(b._h, 0, p, n, fmt, colour, img, m),
                    lambda: lib.ce_batch_set_test_gainmap(b._h, 0, 0, p, n, fmt, colour, img, m),
                    lambda: lib.ce_gainmap_to_linear(gpu_ctx._h, p, n, fmt, colour, img, m, w, h, out.ctypes.data, out.size))

        img, m = good._c()
        ok = (px8, px8.nbytes, ce.PIXEL_RGB8, C.byref(c8))

        def with_meta(**change):
            return C.byref(gain_map(samples, dataclasses.replace(meta, **change))._meta())

        def with_image(**fields):
            i = good._c()[0]
            for k, v in fields.items():
                setattr(i, k, v)
            return C.byref(i)

        third = lambda v, rest=0.0: (rest, rest, v)  # noqa: E731
        bad_meta = {
            "gain_min NaN": dict(gain_min=third(nan)), "gain_max inf": dict(gain_max=third(inf, 2.0)), "gamma NaN": dict(gamma=third(nan, 1.0)),
            "base_offset inf": dict(base_offset=third(inf)), "alternate_offset NaN": dict(alternate_offset=third(nan)),
            "base_headroom NaN": dict(base_headroom=nan), "alternate_headroom inf": dict(alternate_headroom=inf),
            "display_headroom NaN": dict(display_headroom=nan),
            "gamma 0": dict(gamma=third(0.0, 1.0)), "gamma negative": dict(gamma=third(-2.2, 1.0)),
            "gain_min above gain_max": dict(gain_min=third(5.0, -1.0)),
            "gain above 16": dict(gain_max=third(16.5, 4.0)), "gain under -16": dict(gain_min=third(-16.5, -1.0)),
            "headroom above 16": dict(alternate_headroom=16.5), "headroom under -16": dict(base_headroom=-16.5), "display above 16": dict(display_headroom=17.0),
            "base_offset above 1": dict(base_offset=third(1.5)), "alternate_offset under -1": dict(alternate_offset=third(-1.5)),
            "alternate_headroom == base_headroom": dict(alternate_headroom=0.0),
        }
        for what, change in bad_meta.items():
            for call in calls(*ok, C.byref(img), with_meta(**change)):
                refused(call(), what)
        bad_images = {"channels 2": dict(channels=2), "channels 0": dict(channels=0), "channels 4": dict(channels=4), "width 0": dict(width=0),
                      "height 0": dict(height=0), "width above the base's": dict(width=w + 1), "height above the base's": dict(height=h + 1),
                      "null samples": dict(samples=None)}
        for what, fields in bad_images.items():
            for call in calls(*ok, with_image(**fields), C.byref(m)):
                refused(call(), what)
        # null pointers
        for call in (calls(None, px8.nbytes, ce.PIXEL_RGB8, C.byref(c8), C.byref(img), C.byref(m)) + calls(px8, px8.nbytes, ce.PIXEL_RGB8, None, C.byref(img), C.byref(m)) +
                     calls(*ok, None, C.byref(m)) + calls(*ok, C.byref(img), None)):
            refused(call(), "null pointer")
        # everything *_cicp refuses about the base
        bad_colours = {"primaries 2": ce.CeColour(2, 13, 8, 203.0), "transfer 18": ce.CeColour(9, 18, 8, 203.0), "transfer 1": ce.CeColour(1, 1, 8, 203.0),
                       "depth 9": ce.CeColour(1, 13, 9, 203.0), "an 8-bit format with depth 10": c10, "PQ without white": ce.CeColour(9, 16, 8, 0.0),
                       "PQ with white NaN": ce.CeColour(9, 16, 8, nan)}
        for what, colour in bad_colours.items():
            for call in calls(px8, px8.nbytes, ce.PIXEL_RGB8, C.byref(colour), C.byref(img), C.byref(m)):
                refused(call(), what)
        for fmt, px in ((ce.PIXEL_RGB16_10BIT, px16), (ce.PIXEL_RGBA16_10BIT, px16), (ce.PIXEL_RGB_F32, f32), (6, px16), (-1, px16)):
            for call in calls(px, px.nbytes, fmt, C.byref(c10), C.byref(img), C.byref(m)):
                refused(call(), f"format {fmt}")
        for other in (plain, deep):  # a batch that is not linear
            refused(lib.ce_batch_set_reference_gainmap(other._h, 0, px8.ctypes.data, px8.nbytes, ce.PIXEL_RGB8, C.byref(c8), C.byref(img), C.byref(m)), "not linear")
            refused(lib.ce_batch_set_test_gainmap(other._h, 0, 0, px8.ctypes.data, px8.nbytes, ce.PIXEL_RGB8, C.byref(c8), C.byref(img), C.byref(m)), "not linear")
        # slot indices past the batch
        raw = (px8.ctypes.data, px8.nbytes, ce.PIXEL_RGB8, C.byref(c8), C.byref(img), C.byref(m))
        refused(lib.ce_batch_set_reference_gainmap(b._h, 1, *raw), "ref_index")
        refused(lib.ce_batch_set_test_gainmap(b._h, 1, 0, *raw), "pair_index")
        refused(lib.ce_batch_set_test_gainmap(b._h, 0, 1, *raw), "ref_index")
        # wrong lengths
        for call in calls(px8, px8.nbytes - 3, ce.PIXEL_RGB8, C.byref(c8), C.byref(img), C.byref(m)):
            assert call() == ce.CE_ERR_BAD_LENGTH and gpu_ctx._err()
        assert lib.ce_gainmap_to_linear(gpu_ctx._h, *raw, w, h, out.ctypes.data, out.size - 3) == ce.CE_ERR_BAD_LENGTH
        # after all of that: the slots are what they were, the batch scores what it scored, and the calls work
        again = b.run(1, ce.MetricConfig.all())[0]
        assert (again.status, again.valid, again.dssim, again.ssimulacra2, again.butteraugli) == \
               (first.status, first.valid, first.dssim, first.ssimulacra2, first.butteraugli)
        assert np.array_equal(read_slab(ce, b.reference_slab, w * h * 12).view(np.uint32), bits(want).reshape(-1))
        assert np.array_equal(bits(gpu_ctx.gainmap_to_linear(px8, w, h, ce.ColourDescription.SRGB, good)), bits(want))
    finally:
        for x in (b, plain, deep):
            x.close()


def test_session_scores_gain_map_images_through_the_new_calls(ce, gpu_ctx, tmp_path):
    ref, test = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    rng = np.random.default_rng(13)
    samples = gain_map_pair(rng, ref, test)
    decoded = np.ascontiguousarray((samples.astype(np.int64) + 8) // 16 * 16).clip(0, 255).astype(np.uint8)
    gm_src, gm_dec = gain_map(samples, ULTRA), gain_map(decoded, ULTRA)
    cfg = S.EvalConfig.builder().report_dir(str(tmp_path)).metrics(ce.MetricConfig.all()).quality_levels([50.0]).build()
    enc = lambda img, req: b"x"  # noqa: E731
    row_of = lambda r: (r.dssim, r.ssimulacra2, r.butteraugli, r.psnr)  # noqa: E731

    def manual(fill):
        b = gpu_ctx.batch_linear(w, h, 1, 1)
        try:
            fill(b)
            m = ce.MetricResult.from_c(b.run(1, ce.MetricConfig.all())[0])
        finally:
            b.close()
        assert m.ssimulacra2 is not None and m.ssimulacra2 < 100.0
        return (m.dssim, m.ssimulacra2, m.butteraugli, None)

    sess = S.EvalSession(cfg, ctx=gpu_ctx)
    sess.add_codec_with_decode("gm", "1", enc, lambda data: S.ImageData.rgb(test, w, h, gain_map=gm_dec))
    row = sess.evaluate_image("img", S.ImageData.rgb(ref, w, h, gain_map=gm_src)).results[0]
    srgb = ce.ColourDescription.SRGB
    assert row_of(row) == manual(lambda b: (b.set_reference_gainmap(0, ref, srgb, gm_src), b.set_test_gainmap(0, 0, test, srgb, gm_dec)))
    # a Display P3 RGBA16 decode with a map against a plain sRGB source
    p3 = ce.ColourDescription.DISPLAY_P3
    rgba = np.concatenate([test.astype(np.uint16) << 2, np.full((h, w, 1), 1023, np.uint16)], axis=-1)
    mixed = S.EvalSession(cfg, ctx=gpu_ctx)
    mixed.add_codec_with_decode("gm", "1", enc, lambda data: S.ImageData.rgba16(rgba, w, h, 10, colour=p3, gain_map=gm_dec))
    row = mixed.evaluate_image("img", S.ImageData.rgb(ref, w, h)).results[0]
    assert row_of(row) == manual(lambda b: (b.set_reference_cicp(0, ref, srgb), b.set_test_gainmap(0, 0, rgba, p3.with_depth(10), gm_dec)))


def test_a_damaged_map_shows_only_through_the_new_route(ce, gpu_ctx):
    """Identical bases; the decode's map is the source's with its codes rounded to multiples of 16.  Scored base-only as RGB8
    the pair is identical - PSNR inf, SSIMULACRA2 100, Butteraugli 0; through the gain-map route it is not."""
    ref, _ = golden("nat97x131_q75_420")
    h, w = ref.shape[:2]
    rng = np.random.default_rng(17)
    samples = gain_map_pair(rng, ref, ref)
    rounded = np.clip((samples.astype(np.int64) + 8) // 16 * 16, 0, 255).astype(np.uint8)
    assert np.any(rounded != samples)
    base_only = gpu_ctx.calculate_metrics(ref, ref, w, h, ce.MetricConfig.all())
    assert base_only.psnr == float("inf") and base_only.ssimulacra2 == 100.0 and base_only.butteraugli == 0.0
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        b.set_reference_gainmap(0, ref, ce.ColourDescription.SRGB, gain_map(samples, ULTRA))
        b.set_test_gainmap(0, 0, ref, ce.ColourDescription.SRGB, gain_map(rounded, ULTRA))
        m = ce.MetricResult.from_c(b.run(1, ce.MetricConfig.all())[0])
        fidelity = b.hdr_fidelity(1)[0]
        assert m.ssimulacra2 < 100.0 and m.butteraugli > 0.0
        assert fidelity.delta_e_itp_max > 0.0 and fidelity.itp_max_q20 > 0
        assert int(b.delta_e_itp_maps(0, 1)[0].max()) == fidelity.itp_max_q20
    finally:
        b.close()
