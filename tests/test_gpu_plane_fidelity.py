"""A decoder's Y'CbCr planes scored as planes on the device (ce_yuv_plane_fidelity).  Everything the device
returns is an exact integer, so every integer of every pair must equal the numpy restatement
(tests/plane_fidelity_restatement.py) and the doubles finished from them within 1e-14 relative (libm's log10 and pow may
differ): the squared error on every subsampling, layout, depth, alignment, pitch and memory kind and on both load paths of the
SSE kernel; one level and five, at every edge of the level kernel's tile on luma and on chroma; shared references and mixed
layouts; against the RGB8 and deep batches' own PSNR and MS-SSIM; the anchors; beside a launch; every refusal."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_fidelity_restatement as P  # noqa: E402

pytestmark = pytest.mark.gpu

Q = 1 << 32


def variants(ce, samples, sub, depth, msbs, keep):
    """the same samples as images of both layouts, every pitch, on the host, on the device, and on the device one sample past
    an aligned allocation (the rows a wide load may not read)"""
    bps = 1 if depth == 8 else 2
    out = []
    for layout in (K.PLANAR, K.SEMIPLANAR):
        for msb in msbs:
            for pad in ([0, 1, 2, 64] if bps == 1 else [0, 2, 64]):
                host = K.image(ce, samples, sub, depth, layout, msb, pad)
                out.append(host)
                for offset in (0, bps):
                    dev, buffers = K.on_device(ce, host, offset)
                    keep.append(buffers)
                    out.append(dev)
    return out


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_squared_error_alone_on_every_layout_pitch_memory_and_load_path(ce, gpu_ctx, depth):
    """levels = 0.  Each shape and subsampling: every variant of the test image against one reference, then variant i of the
    reference against variant n - 1 - i of the test image without a pair table, so that the two sides differ in layout, pitch,
    memory and, at 10 bits, alignment (low- and MSB-aligned images in one call)."""
    msbs = (False, True) if depth == 10 else (False,)
    calls = 0
    for w, h in K.SSE_SHAPES:
        for sub in K.SUBS:
            ref, test = K.planes(w, h, sub, depth)
            want = K.expected(w, h, sub, depth, 0)
            keep = []
            rv, tv = variants(ce, ref, sub, depth, msbs, keep), variants(ce, test, sub, depth, msbs, keep)
            got = gpu_ctx.plane_fidelity(rv[:1], tv, w, h, pair_ref=[0] * len(tv), levels=0)
            got += gpu_ctx.plane_fidelity(rv, tv[::-1], w, h, levels=0)
            for i, g in enumerate(got):
                K.check_integers(g, want, (w, h, sub, depth, i))
            calls += 2
    print(f"depth {depth}: {calls} calls of {len(tv)} pairs; 100 x 76 4:0:0 psnr {got[0].psnr[0]!r}")


def test_clamp_of_low_aligned_samples_above_the_depth(ce, gpu_ctx):
    w, h, sub = 33, 31, P.SUB_420
    rng = np.random.default_rng(11)
    ref = [rng.integers(0, 1 << 16, (ph, pw)).astype(np.uint16) for pw, ph in P.plane_sizes(w, h, sub)]
    test = [rng.integers(0, 1 << 16, (ph, pw)).astype(np.uint16) for pw, ph in P.plane_sizes(w, h, sub)]
    for depth in (10, 12):
        want = P.plane_fidelity([P.sample(p, depth) for p in ref], [P.sample(p, depth) for p in test], depth, sub, 1)
        for layout in (K.PLANAR, K.SEMIPLANAR):
            got = gpu_ctx.plane_fidelity([K.image(ce, ref, sub, depth, layout)], [K.image(ce, test, sub, depth, K.PLANAR, pad=2)], w, h, levels=1)[0]
            K.check_integers(got, want, (depth, layout))
        assert want["n_levels"] == [1, 1, 1] and max(int(p.max()) for p in ref) > 4095


@pytest.mark.parametrize("w,h,sub", K.ONE_LEVEL, ids=lambda v: str(v))
def test_one_level_on_the_smallest_planes(ce, gpu_ctx, w, h, sub):
    ref, test = K.planes(w, h, sub, 8)
    want = K.expected(w, h, sub, 8, 1)
    keep = []
    dev, t = K.on_device(ce, K.image(ce, test, sub, 8, K.SEMIPLANAR, pad=1))
    keep.append(t)
    got = gpu_ctx.plane_fidelity([K.image(ce, ref, sub, 8)], [dev], w, h, levels=1)[0]
    K.check_integers(got, want, (w, h, sub))
    assert got.n_levels == {(21, 22): (1, 1, 1), (20, 20): (1, 0, 0), (12, 11): (1, 1, 1), (11, 75): (1, 0, 0)}[(w, h)]
    assert got.n_pos[0][0] == (w - 10) * (h - 10) and all(np.isnan(v) for v in got.ms_ssim)
    if (w, h) == (21, 22):
        assert got.n_pos[1][0] == got.n_pos[2][0] == 1  # chroma 11 x 11: one window
    if (w, h) == (20, 20):
        assert np.isnan(got.ssim[1]) and got.ssim_q[1] == (0,) * 5 and got.sse[1] > 0 and got.psnr[1] > 20


@pytest.mark.parametrize("w,h,sub,layout,depth,msb", K.FIVE_LEVELS + K.TILE_EDGES, ids=lambda v: str(v))
def test_five_levels_equal_the_restatement_on_every_integer(ce, gpu_ctx, w, h, sub, layout, depth, msb):
    ref, test = K.planes(w, h, sub, depth)
    want = K.expected(w, h, sub, depth, 5)
    dev, keep = K.on_device(ce, K.image(ce, test, sub, depth, layout, msb, pad=64))
    got = gpu_ctx.plane_fidelity([K.image(ce, ref, sub, depth, K.PLANAR)], [dev], w, h)[0]
    K.check_integers(got, want, (w, h, sub, depth))
    cw, ch = P.plane_sizes(w, h, sub)[1]
    assert got.n_levels == (5, 5 if min(cw, ch) > 160 else 1, 5 if min(cw, ch) > 160 else 1) and 0.35 < got.ms_ssim[0] < 1.0
    print(f"{w} x {h} sub {sub} depth {depth}: psnr {got.psnr!r} overall {got.psnr_overall!r} ssim {got.ssim!r} ms_ssim {got.ms_ssim!r}")


def test_shared_references_and_mixed_layouts(ce, gpu_ctx):
    """Two planar references on the host, five semiplanar tests on the device with a padded pitch, a pair table that is no
    identity; the identity table against none; and a pair's result whoever shares the call"""
    w, h, sub = 176, 163, P.SUB_420
    refs = [K.image(ce, K.planes(w, h, sub, 8, s)[0], sub, 8) for s in (0, 1)]
    seeds, table = (1, 0, 2, 1, 0), [1, 0, 1, 1, 0]
    keep, tests = [], []
    for s in seeds:
        dev, t = K.on_device(ce, K.image(ce, K.planes(w, h, sub, 8, s)[1], sub, 8, K.SEMIPLANAR, pad=48))
        keep.append(t), tests.append(dev)
    wants = [K.expected(w, h, sub, 8, 5, s, r) for s, r in zip(seeds, table)]
    got = gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table)
    for i in range(5):
        K.check_integers(got[i], wants[i], i)
    assert K.key(gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table)) == K.key(got)
    # pairs 1 and 0 alone, with the identity table and with none; pair 3 alone
    assert K.key(gpu_ctx.plane_fidelity(refs, [tests[1], tests[0]], w, h, pair_ref=[0, 1])) == K.key([got[1], got[0]])
    assert K.key(gpu_ctx.plane_fidelity(refs, [tests[1], tests[0]], w, h)) == K.key([got[1], got[0]])
    assert K.key(gpu_ctx.plane_fidelity(refs[1:], tests[3:4], w, h)) == K.key([got[3]])
    assert gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table, levels=0)[2].sse == got[2].sse


def rgb_of(planes):
    return np.ascontiguousarray(np.stack(planes, axis=-1))


def test_444_planes_against_the_batches_own_psnr_and_ms_ssim(ce, gpu_ctx):
    """The same samples as 4:4:4 planes and packed into a batch as R = Y, G = Cb, B = Cr: the level integers of plane p are the
    batch's of channel p, and the overall PSNR is the batch's PSNR, both finished by one expression from one integer"""
    w, h = 176, 163
    for depth in (8, 10):
        ref, test = K.planes(w, h, P.SUB_444, depth)
        got = gpu_ctx.plane_fidelity([K.image(ce, ref, P.SUB_444, depth)], [K.image(ce, test, P.SUB_444, depth, K.SEMIPLANAR)], w, h)[0]
        b = ce.Batch(gpu_ctx, w, h, 1, 1) if depth == 8 else gpu_ctx.batch_deep(w, h, 1, 1, depth, depth)
        try:
            b.set_reference(0, rgb_of(ref))
            b.set_test(0, 0, rgb_of(test))
            ms = b.ms_ssim(1)[0]
            psnr = b.run(1, ce.MetricConfig(psnr=True))[0].psnr
        finally:
            b.close()
        for p in range(3):
            assert got.ssim_q[p] == tuple(ms.ssim_q[l][p] for l in range(5)) and got.cs_q[p] == tuple(ms.cs_q[l][p] for l in range(5)), (depth, p)
            assert got.n_pos[p] == ms.n and got.ssim[p] == ms.ssim_rgb[p] and got.ms_ssim[p] == ms.ms_ssim_rgb[p]
        assert got.psnr_overall == psnr and 20 < psnr < 60, (depth, got.psnr_overall, psnr)


def test_identity_and_inverted_checkerboard_leave_device_planes_unchanged(ce, gpu_ctx):
    w, h, sub = 322, 330, P.SUB_420
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 1024, (ph, pw)).astype(np.uint16) for pw, ph in P.plane_sizes(w, h, sub)]
    dev, buffers = K.on_device(ce, K.image(ce, planes, sub, 10, K.SEMIPLANAR, True, pad=6))
    before = [b.read() for b in buffers]
    got = gpu_ctx.plane_fidelity([K.image(ce, planes, sub, 10)], [dev], w, h)[0]
    assert [np.array_equal(b.read(), was) for b, was in zip(buffers, before)] == [True, True]
    assert got.sse == (0, 0, 0) and got.psnr == (np.inf,) * 3 and got.psnr_overall == np.inf and got.psnr_weighted == np.inf
    assert got.n_levels == (5, 5, 5) and got.ssim == (1.0,) * 3 and got.ms_ssim == (1.0,) * 3
    for p in range(3):
        assert got.ssim_q[p] == got.cs_q[p] == tuple(n * Q for n in got.n_pos[p]) and min(got.n_pos[p]) > 0
    a, b = K.checkerboard(384, 352, sub)
    got = gpu_ctx.plane_fidelity([K.image(ce, a, sub, 8)], [K.image(ce, b, sub, 8)], 384, 352)[0]
    K.check_integers(got, P.plane_fidelity(a, b, 8, sub, 5), "checkerboard")
    assert all(got.cs_q[p][0] < 0 for p in range(3)) and got.ms_ssim == (0.0,) * 3 and max(got.ssim) < 0
    assert got.sse == tuple(255 * 255 * n for n in got.n) and got.psnr == (0.0,) * 3


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_a_launch_collected_across_the_call_keeps_its_scores_and_diffmap(ce, gpu_ctx):
    w, h, sub = 176, 163, P.SUB_420
    rng = np.random.default_rng(8)
    ref = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    test = np.clip(ref.astype(np.int32) + rng.integers(-9, 10, ref.shape), 0, 255).astype(np.uint8)
    pr, pt = K.planes(w, h, sub, 8)
    cfg = ce.MetricConfig.all()
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference(0, ref)
        b.set_test(0, 0, test)
        scores = b.run(1, cfg, butteraugli_diffmap=True)
        diffmap = b.butteraugli_diffmaps(0, 1).copy()
        b.launch(1, cfg, butteraugli_diffmap=True)
        got = gpu_ctx.plane_fidelity([K.image(ce, pr, sub, 8)], [K.image(ce, pt, sub, 8, K.SEMIPLANAR)], w, h)[0]
        again = b.collect(1)
        key = lambda s: (bits(s.dssim), bits(s.ssimulacra2), bits(s.butteraugli), bits(s.psnr), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in scores] and again[0].valid == 15
        assert np.array_equal(b.butteraugli_diffmaps(0, 1), diffmap)
        K.check_integers(got, K.expected(w, h, sub, 8), "beside a launch")
    finally:
        b.close()


def test_every_refusal_names_its_reason_and_leaves_the_context_usable(ce, gpu_ctx):
    w, h, sub = 40, 36, P.SUB_420
    ref, test = K.planes(w, h, sub, 8)
    want = K.expected(w, h, sub, 8, 1)
    L = ce.lib()
    keep = []

    def c_of(images):
        arr = (ce.CeYuvImage * len(images))()
        for i, img in enumerate(images):
            arr[i], k = img._c()
            keep.append(k)
        return arr

    good_r, good_t = K.image(ce, ref, sub, 8), K.image(ce, test, sub, 8, K.SEMIPLANAR)
    out = (ce.CePlaneScores * 4)()

    def call(refs, n_refs, tests, n_pairs, table, levels, width=w, height=h, out=out):
        t = None if table is None else (C.c_uint32 * len(table))(*table)
        return L.ce_yuv_plane_fidelity(gpu_ctx._h, width, height, refs, n_refs, tests, n_pairs, t, levels, out)

    def refused(rc, word):
        assert rc == ce.CE_ERR_INVALID_ARG and word in gpu_ctx._err(), (rc, word, gpu_ctx._err())
        K.check_integers(gpu_ctx.plane_fidelity([good_r], [good_t], w, h, levels=1)[0], want, "after " + word)

    r1, t1, t2 = c_of([good_r]), c_of([good_t]), c_of([good_t, good_t])
    refused(call(None, 1, t1, 1, None, 1), "null")
    refused(call(r1, 1, None, 1, None, 1), "null")
    refused(call(r1, 1, t1, 1, None, 1, out=None), "null")
    refused(call(r1, 1, t1, 0, None, 1), "no references or no pairs")
    refused(call(r1, 0, t1, 1, [0], 1), "no references or no pairs")
    refused(call(r1, 1, t2, 2, [0, 1], 1), "names reference 1")
    refused(call(r1, 1, t2, 2, None, 1), "pair table")
    for levels in (2, 3, 4, 6):
        refused(call(r1, 1, t1, 1, None, levels), "levels")
    refused(call(r1, 1, t1, 1, None, 5), "160")       # luma too small for five levels
    refused(call(r1, 1, t1, 1, None, 1, 10, 36), "11")  # and for one: the images are checked at the call's size first, so give it planes
    refused(call(r1, 1, t1, 1, None, 0, 0, h), "empty")
    refused(call(r1, 1, t1, 1, None, 0, w, 0), "empty")
    # images of one call that disagree, and pairs that do
    other_sub = K.image(ce, K.planes(w, h, P.SUB_444, 8)[1], P.SUB_444, 8)
    refused(call(r1, 1, c_of([other_sub]), 1, None, 0), "subsampling or depth")
    deeper = K.image(ce, K.planes(w, h, sub, 10)[1], sub, 10)
    refused(call(r1, 1, c_of([deeper]), 1, None, 0), "subsampling or depth")
    refused(call(r1, 1, c_of([K.image(ce, test, sub, 8, matrix=ce.YUV_BT709)]), 1, None, 0), "matrix or range")
    refused(call(r1, 1, c_of([K.image(ce, test, sub, 8, range=ce.YUV_LIMITED)]), 1, None, 0), "matrix or range")
    # what the ingest's own check refuses
    def broken(**change):
        c = c_of([good_t])
        for k, v in change.items():
            if k == "plane1":
                c[0].plane[1] = v
            elif k == "pitch0":
                c[0].pitch[0] = v
            else:
                setattr(c[0], k, v)
        return c

    refused(call(r1, 1, broken(plane1=None), 1, None, 0), "missing")
    refused(call(r1, 1, broken(subsampling=7), 1, None, 0), "subsampling")
    refused(call(r1, 1, broken(layout=2), 1, None, 0), "layout")
    refused(call(r1, 1, broken(matrix=9), 1, None, 0), "matrix")
    refused(call(r1, 1, broken(range=5), 1, None, 0), "range")
    refused(call(r1, 1, broken(upsample=4), 1, None, 0), "upsampling")
    refused(call(r1, 1, broken(memory=3), 1, None, 0), "memory")
    refused(call(r1, 1, broken(depth=9), 1, None, 0), "depth")
    refused(call(r1, 1, broken(msb_aligned=1), 1, None, 0), "msb_aligned")
    refused(call(r1, 1, broken(pitch0=w - 1), 1, None, 0), "pitch")
    refused(call(r1, 1, broken(lut=8), 1, None, 0), "colour table")
    r10, t10 = K.planes(w, h, sub, 10)
    odd = c_of([K.image(ce, t10, sub, 10)])
    odd[0].pitch[0] = 2 * w + 1
    refused(call(c_of([K.image(ce, r10, sub, 10)]), 1, odd, 1, None, 0), "2-byte aligned")
    assert L.ce_yuv_plane_fidelity(None, w, h, r1, 1, t1, 1, None, 0, out) == ce.CE_ERR_INVALID_ARG
    assert C.sizeof(ce.CePlaneScores) == 512
