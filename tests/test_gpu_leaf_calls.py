"""The context's kept one-pair batches (ce_eval_pair_deep, ce_eval_pair_linear, ce_eval_pair_hdr_fidelity and the three map
leaves) when calls of different kinds, shapes and depths alternate on one context: every result equals, in every bit, what
the same input gives through a freshly created 1 x 1 batch of its kind; a refused call leaves the next one as it was.  Then
every refusal of the one-pair calls, with its status and its message as the library words them.  No tolerance anywhere."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_linear_restatement as RL  # noqa: E402
import resample_restatement as R8  # noqa: E402

pytestmark = pytest.mark.gpu

A, B = (23, 9), (16, 11)  # both at least 8 x 8 (Butteraugli, SSIMULACRA2); 23 x 9 is no multiple of 4 pixels


def rgb8_pair(w, h):
    ref = R8.content(w, h, "pattern", seed=1)
    noise = np.random.default_rng(w * 31 + h).integers(-9, 10, ref.shape)
    return ref, np.clip(ref.astype(np.int32) + noise, 0, 255).astype(np.uint8)


def deep_image(w, h, depth, seed):
    maxv = (1 << depth) - 1
    base = R8.content(w, h, "pattern", seed=0).astype(np.int64) * maxv // 255
    noise = np.random.default_rng(seed * 1000 + w * 31 + h + depth).integers(-(maxv // 40) - 1, maxv // 40 + 2, base.shape)
    return np.clip(base + noise, 0, maxv).astype(np.uint16)


def linear_pair(w, h):
    ref = RL.content(w, h, seed=5, negatives=True)
    return ref, (ref * np.float32(0.97) + np.float32(0.004)).astype(np.float32)


def f64_bits(v):
    return None if v is None else int(np.float64(v).view(np.uint64))


def result_bits(m):
    """A MetricResult as raw 64-bit patterns (None where `valid` leaves a metric out): NaN equals NaN."""
    return tuple(f64_bits(v) for v in (m.dssim, m.ssimulacra2, m.butteraugli, m.psnr))


def hdr_bits(s):
    return (f64_bits(s.pq_psnr), f64_bits(s.delta_e_itp_mean), f64_bits(s.delta_e_itp_max), s.pq_sse, s.itp_sum_q20, s.itp_max_q20)


def fresh(ce, batch, ref, test, read):
    """`read(batch)` of the pair loaded into a freshly created 1 x 1 batch, which is closed afterwards."""
    try:
        batch.set_reference(0, ref)
        batch.set_test(0, 0, test)
        return read(batch)
    finally:
        batch.close()


def run_bits(ce, b, config, **kw):
    s = b.run(1, config, **kw)[0]
    assert s.status == 0
    return result_bits(ce.MetricResult.from_c(s))


def test_alternating_kinds_shapes_and_depths_equal_fresh_batches(gpu_ctx, ce):
    ctx, cfg = gpu_ctx, ce.MetricConfig.all()
    rgb = {s: rgb8_pair(*s) for s in (A, B)}
    lin = {s: linear_pair(*s) for s in (A, B)}
    deep = {(s, d): deep_image(*s, d, seed) for s in (A, B) for seed, d in ((1, 10), (2, 12), (3, 8))}
    deep_t = {(s, d): deep_image(*s, d, seed + 10) for s in (A, B) for seed, d in ((1, 10), (2, 12), (3, 8))}

    def deep_step(s, rd, td):
        r, t = deep[(s, rd)], deep_t[(s, td)]
        got = result_bits(ctx.eval_pair_deep(r, rd, t, td, s[0], s[1], cfg))
        want = fresh(ce, ctx.batch_deep(s[0], s[1], 1, 1, rd, td), r, t, lambda b: run_bits(ce, b, cfg))
        assert got == want, ("deep", s, rd, td)
        return got

    def linear_step(s):
        r, t = lin[s]
        got = result_bits(ctx.eval_pair_linear(r, t, s[0], s[1], cfg))
        assert got == fresh(ce, ctx.batch_linear(s[0], s[1], 1, 1), r, t, lambda b: run_bits(ce, b, cfg)), ("linear", s)

    def hdr_step(s, depth):
        r, t = lin[s]
        got = hdr_bits(ctx.hdr_fidelity(r, t, s[0], s[1], depth))
        assert got == fresh(ce, ctx.batch_linear(s[0], s[1], 1, 1), r, t, lambda b: hdr_bits(b.hdr_fidelity(1, depth)[0])), ("hdr", s, depth)

    def diffmap_step(s):
        r, t = rgb[s]
        got = ctx.calculate_butteraugli_diffmap(r, t, s[0], s[1])

        def read(b):
            bits = run_bits(ce, b, ce.MetricConfig(butteraugli=True), butteraugli_diffmap=True)
            return bits[2], b.butteraugli_diffmaps(0, 1)[0]
        score, dm = fresh(ce, ce.Batch(ctx, s[0], s[1], 1, 1), r, t, read)
        assert f64_bits(got.score) == score and np.array_equal(got.diffmap.view(np.uint32), dm.view(np.uint32)), ("diffmap", s)

    def ssim_maps_step(s):
        r, t = rgb[s]
        score, levels = ctx.calculate_dssim_with_ssim_maps(r, t, s[0], s[1])

        def read(b):
            bits = run_bits(ce, b, ce.MetricConfig(dssim=True))
            return bits[0], [b.dssim_ssim_maps(l, 0, 1) for l in range(len(ce.dssim_levels(*s)))]
        want_score, want = fresh(ce, ce.Batch(ctx, s[0], s[1], 1, 1), r, t, read)
        assert f64_bits(score) == want_score and len(levels) == len(want) > 0
        for got_l, (maps, ssim) in zip(levels, want):
            assert np.array_equal(got_l.map.view(np.uint32), maps[0].view(np.uint32)) and f64_bits(got_l.ssim) == f64_bits(ssim[0])

    def ssim2_maps_step(s):
        r, t = rgb[s]
        score, feats, scales = ctx.calculate_ssimulacra2_with_maps(r, t, s[0], s[1])

        def read(b):
            bits = run_bits(ce, b, ce.MetricConfig(ssimulacra2=True), ssimulacra2_maps=True)
            n = len(ce.ssimulacra2_scales(*s))
            return bits[1], b.debug_averages(0), [[[b.ssimulacra2_maps(sc, c, k, 0, 1)[0][0] for k in range(3)] for c in range(3)] for sc in range(n)]
        want_score, avg, want = fresh(ce, ce.Batch(ctx, s[0], s[1], 1, 1), r, t, read)
        n = len(want)
        assert f64_bits(score) == want_score and len(scales) == n > 0
        assert feats[:n].tobytes() == avg[:n].tobytes() and np.all(np.isnan(feats[n:]))
        for sc in range(n):
            assert np.array_equal(scales[sc].view(np.uint32), np.asarray(want[sc]).view(np.uint32)), ("ssim2 maps", s, sc)

    first = deep_step(A, 10, 10)   # 1
    linear_step(A)                 # 2
    hdr_step(A, 10)                # 3: reuses the linear batch
    diffmap_step(A)                # 4
    deep_step(B, 10, 10)           # 5: the shape changes
    hdr_step(B, 12)                # 6: remakes the linear batch
    linear_step(B)                 # 7: keeps it
    deep_step(B, 12, 8)            # 8: only the depths change
    ssim_maps_step(B)              # 9
    ssim2_maps_step(A)             # 10
    assert deep_step(A, 10, 10) == first  # 11

    # three failing calls; the first step again after each
    with pytest.raises(ce.DimensionMismatch):
        ctx.eval_pair_deep(deep[(A, 10)], 10, deep_t[(A, 10)].reshape(-1)[:-3], 10, A[0], A[1], cfg)
    assert deep_step(A, 10, 10) == first
    with pytest.raises(ce.DimensionMismatch):
        ctx.eval_pair_linear(lin[A][0], lin[A][1].reshape(-1)[:-3], A[0], A[1], cfg)
    assert deep_step(A, 10, 10) == first
    small = rgb8_pair(7, 7)
    with pytest.raises(ce.MetricCalculation) as e:
        ctx.calculate_butteraugli_diffmap(small[0], small[1], 7, 7)
    assert e.value.status == ce.CE_ERR_TOO_SMALL
    assert deep_step(A, 10, 10) == first


def refused(ce, ctx, rc, status, message, out=None):
    """A refusal: its status, the context's last error word for word, and out->status where the call writes one."""
    assert rc == status, (rc, ctx._err())
    assert ctx._err() == message
    if out is not None:
        assert out.status == rc


def test_refusals_of_the_scored_one_pair_calls(gpu_ctx, ce):
    ctx, L = gpu_ctx, ce.lib()
    w, h = A
    INV, all_mask = ce.CE_ERR_INVALID_ARG, ce.MetricConfig.all().mask
    r16, t16 = deep_image(w, h, 10, 1), deep_image(w, h, 10, 11)
    rf, tf = linear_pair(w, h)
    n16, nf = r16.nbytes, rf.nbytes

    def deep(rlen=n16, rd=10, tlen=n16, td=10, ww=w, hh=h, mask=all_mask, flags=0, ref=r16.ctypes.data):
        out = ce.CeScores()
        out.status = 77
        return L.ce_eval_pair_deep(ctx._h, ref, rlen, rd, t16.ctypes.data, tlen, td, ww, hh, mask, flags, 80.0, C.byref(out)), out

    def linear(rlen=nf, tlen=nf, ww=w, hh=h, mask=all_mask, flags=0, ref=rf.ctypes.data):
        out = ce.CeScores()
        out.status = 77
        return L.ce_eval_pair_linear(ctx._h, ref, rlen, tf.ctypes.data, tlen, ww, hh, mask, flags, 80.0, C.byref(out)), out

    rc, out = deep(rd=9)
    refused(ce, ctx, rc, INV, "depths must be 8, 10, 12 or 16 bits, got 9 / 10", out)
    rc, out = deep(td=14, rlen=1)  # the depths come before every length
    refused(ce, ctx, rc, INV, "depths must be 8, 10, 12 or 16 bits, got 10 / 14", out)
    for call, n in ((deep, n16), (linear, nf)):
        rc, out = call(tlen=n - 6, mask=1 << 9, flags=ce.FLAG_BUTTERAUGLI_DIFFMAP)  # the mismatch comes before the flags
        refused(ce, ctx, rc, ce.CE_ERR_DIM_MISMATCH, f"Dimension mismatch: reference {n} bytes, test {n - 6} bytes", out)
        rc, out = call(rlen=n - 6, tlen=n - 6)
        refused(ce, ctx, rc, ce.CE_ERR_BAD_LENGTH, f"Invalid image size: expected {n} bytes, got {n - 6}", out)
        for flag in (ce.FLAG_BUTTERAUGLI_DIFFMAP, ce.FLAG_SSIMULACRA2_MAPS):
            rc, out = call(flags=flag, mask=1 << 9)  # the flags come before the metric bits
            refused(ce, ctx, rc, INV, "map flags need a ce_batch: this call's batch does not outlive it", out)
        rc, out = call(mask=all_mask | 1 << 9)
        refused(ce, ctx, rc, INV, "unknown metric bit", out)
        # an empty image: a status and no message (the last error stays the one before); a null pointer: not even out->status
        for kw in ({"ww": 0}, {"hh": 0}):
            rc, out = call(rlen=0, tlen=0, **kw)
            refused(ce, ctx, rc, INV, "unknown metric bit", out)
        rc, out = call(ref=None)
        assert rc == INV and out.status == 77 and ctx._err() == "unknown metric bit"
    # a count of samples is not a length
    rc, out = deep(rlen=r16.size, tlen=r16.size)
    refused(ce, ctx, rc, ce.CE_ERR_BAD_LENGTH, f"Invalid image size: expected {n16} bytes, got {r16.size}", out)


def test_refusals_of_hdr_fidelity(gpu_ctx, ce):
    ctx, L = gpu_ctx, ce.lib()
    w, h = A
    INV = ce.CE_ERR_INVALID_ARG
    rf, tf = linear_pair(w, h)
    nf = rf.nbytes

    def pair(rlen=nf, tlen=nf, ww=w, hh=h, depth=10, white=203.0, ref=rf.ctypes.data, out=True):
        s = ce.CeHdrScores()
        return L.ce_eval_pair_hdr_fidelity(ctx._h, ref, rlen, tf.ctypes.data, tlen, ww, hh, depth, white, C.byref(s) if out else None)

    refused(ce, ctx, pair(ref=None), INV, "HDR fidelity: null pointer")
    refused(ce, ctx, pair(out=False), INV, "HDR fidelity: null pointer")
    refused(ce, ctx, pair(ww=0, depth=8), INV, "HDR fidelity: empty image")  # before the depth
    for d in (8, 11, 14):
        refused(ce, ctx, pair(depth=d, white=0.0, rlen=1), INV, f"HDR fidelity: depth must be 10, 12 or 16, got {d}")  # before white_nits
    for white in (0.0, -1.0, float("inf"), float("nan")):
        refused(ce, ctx, pair(white=white, rlen=1), INV, "HDR fidelity: white_nits must be finite and > 0")  # before the lengths
    refused(ce, ctx, pair(rlen=nf - 4, tlen=nf - 8), ce.CE_ERR_BAD_LENGTH, f"Invalid image size: expected {nf} bytes, got {nf - 4}")
    refused(ce, ctx, pair(tlen=nf - 8), ce.CE_ERR_BAD_LENGTH, f"Invalid image size: expected {nf} bytes, got {nf - 8}")
    plain, deep, lin = ce.Batch(ctx, w, h, 1, 1), ctx.batch_deep(w, h, 1, 1, 10, 10), ctx.batch_linear(w, h, 1, 2)
    try:
        s = (ce.CeHdrScores * 2)()
        for b in (plain, deep):
            refused(ce, ctx, L.ce_batch_hdr_fidelity(b._h, 1, 8, 0.0, s), INV,
                    "HDR fidelity reads linear light: it needs a linear batch (ce_batch_create_linear)")  # before depth and white_nits
        refused(ce, ctx, L.ce_batch_hdr_fidelity(lin._h, 1, 10, 203.0, None), INV, "HDR fidelity: null pointer")
        refused(ce, ctx, L.ce_batch_hdr_fidelity(lin._h, 3, 9, 203.0, s), INV, "HDR fidelity: depth must be 10, 12 or 16, got 9")
        refused(ce, ctx, L.ce_batch_hdr_fidelity(lin._h, 3, 10, -2.0, s), INV, "HDR fidelity: white_nits must be finite and > 0")
        for n in (0, 3):
            refused(ce, ctx, L.ce_batch_hdr_fidelity(lin._h, n, 10, 203.0, s), INV, "n_pairs out of range")
    finally:
        plain.close(), deep.close(), lin.close()


def test_refusals_of_the_map_leaves(gpu_ctx, ce):
    ctx, L = gpu_ctx, ce.lib()
    w, h = A
    INV = ce.CE_ERR_INVALID_ARG
    ref, test = rgb8_pair(w, h)
    n = ref.size
    score, five = C.c_double(), np.empty(ce.DSSIM_MAX_LEVELS, np.float64)
    feats, maps = np.empty((ce.SSIM2_MAX_SCALES, 3, 6), np.float64), np.empty(16 * w * h, np.float32)

    def diffmap(rlen=n, tlen=n, ww=w, hh=h, r=ref.ctypes.data):
        return L.ce_calculate_butteraugli_diffmap(ctx._h, r, rlen, test.ctypes.data, tlen, ww, hh, 80.0, C.byref(score), maps.ctypes.data)

    def ssim_maps(floats, rlen=n, tlen=n, ww=w, hh=h, r=ref.ctypes.data):
        return L.ce_calculate_dssim_ssim_maps(ctx._h, r, rlen, test.ctypes.data, tlen, ww, hh, C.byref(score), five.ctypes.data,
                                              maps.ctypes.data, floats)

    def ssim2_maps(floats, rlen=n, tlen=n, ww=w, hh=h, r=ref.ctypes.data):
        return L.ce_calculate_ssimulacra2_maps(ctx._h, r, rlen, test.ctypes.data, tlen, ww, hh, C.byref(score), feats.ctypes.data,
                                               maps.ctypes.data, floats)

    ds_want = sum(a * b for a, b in ce.dssim_levels(w, h))
    s2_want = 9 * sum(a * b for a, b in ce.ssimulacra2_scales(w, h))
    for call in (diffmap, lambda **kw: ssim_maps(ds_want, **kw), lambda **kw: ssim2_maps(s2_want, **kw)):
        refused(ce, ctx, call(tlen=n - 3, ww=7, hh=7), ce.CE_ERR_DIM_MISMATCH, f"Dimension mismatch: reference {n} bytes, test {n - 3} bytes")
        refused(ce, ctx, call(rlen=n - 3, tlen=n - 3), ce.CE_ERR_BAD_LENGTH, f"Invalid image size: expected {n} bytes, got {n - 3}")
        assert call(r=None) == INV and ctx._err() == f"Invalid image size: expected {n} bytes, got {n - 3}"  # a null pointer: no message
    # the 8 x 8 minimum, behind the lengths; DSSIM has none
    refused(ce, ctx, diffmap(rlen=147, tlen=147, ww=7, hh=7), ce.CE_ERR_TOO_SMALL, "minimum 8x8 for butteraugli")
    refused(ce, ctx, diffmap(rlen=8 * 7 * 3, tlen=8 * 7 * 3, ww=8, hh=7), ce.CE_ERR_TOO_SMALL, "minimum 8x8 for butteraugli")
    refused(ce, ctx, ssim2_maps(0, rlen=147, tlen=147, ww=7, hh=7), ce.CE_ERR_TOO_SMALL, "minimum 8x8 for ssimulacra2")
    refused(ce, ctx, ssim2_maps(0, rlen=7 * 8 * 3, tlen=7 * 8 * 3, ww=7, hh=8), ce.CE_ERR_TOO_SMALL, "minimum 8x8 for ssimulacra2")
    # an empty image, ahead of the lengths
    refused(ce, ctx, ssim_maps(0, rlen=0, tlen=0, ww=0), INV, "empty image")
    refused(ce, ctx, ssim2_maps(0, tlen=n - 3, hh=0), INV, "empty image")
    # maps_floats, last
    for floats in (0, ds_want - 1, ds_want + 1):
        refused(ce, ctx, ssim_maps(floats), INV, f"SSIM maps of every level need {ds_want} floats, got {floats}")
    for floats in (0, s2_want - 9, s2_want + 1):
        refused(ce, ctx, ssim2_maps(floats), INV, f"SSIMULACRA2 maps of every scale need {s2_want} floats, got {floats}")
    # and the calls as they should be
    assert diffmap() == 0 and ssim_maps(ds_want) == 0 and ssim2_maps(s2_want) == 0
