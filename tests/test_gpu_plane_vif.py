"""VIFp of a decoder's Y'CbCr planes on the device (ce_yuv_plane_vif).  Everything the device returns is an
exact integer and the doubles are pure f64 quotients of them, so every integer and every double of every pair must equal the
numpy restatement (tests/plane_vif_restatement.py) bit for bit: on the shapes of tests/plane_vif_cases.py, each one way for the
kernels to go wrong, with host and device planes, planar and semiplanar layouts, MSB-aligned samples, depths 8, 10 and 12 and
odd pitches; shared references; a repeat; beside a launch and beside the other plane calls; past 65535 pairs; every refusal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_vif_cases as VK  # noqa: E402
import plane_vif_restatement as V  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,sub,depth,layout,msb", VK.SHAPES, ids=lambda v: str(v))
def test_every_shape_equals_the_restatement_on_host_and_device_planes(ce, gpu_ctx, w, h, sub, depth, layout, msb):
    """One planar reference on the host; the test image four times: on the host in the shape's layout with an odd pitch, on the
    device with another pitch at an aligned and at an unaligned base, and on the host in the other layout"""
    ref, test = VK.planes(w, h, sub, depth)
    want = VK.expected(w, h, sub, depth)
    bps = 1 if depth == 8 else 2
    other = K.PLANAR if layout == K.SEMIPLANAR else K.SEMIPLANAR
    keep, tests = [], [K.image(ce, test, sub, depth, layout, msb, pad=bps)]
    for offset in (0, bps):
        dev, buffers = K.on_device(ce, K.image(ce, test, sub, depth, layout, msb, pad=3 * bps), offset)
        keep.append(buffers), tests.append(dev)
    tests.append(K.image(ce, test, sub, depth, other, False, pad=0))
    got = gpu_ctx.plane_vif([K.image(ce, ref, sub, depth)], tests, w, h, pair_ref=[0] * len(tests))
    for i, g in enumerate(got):
        VK.check(g, want, (w, h, sub, depth, i))
    assert got[0].num_q[0][0] > 0 and got[0].n_pos[0][0] == (w - 16) * (h - 16)
    print(f"{w} x {h} sub {sub} depth {depth}: ran {got[0].ran} n_pos {got[0].n_pos[0]} vifp {got[0].vifp!r} scales of luma {got[0].vif_scale[0]!r}")


def test_anchors_on_the_device(ce, gpu_ctx):
    """An identical pair, an inverted one and a flat reference, as tests/test_plane_vif_cpu.py works them out"""
    ref = VK.planes(82, 82, V.SUB_420, 8)[0]
    inv = [255 - p for p in ref]
    img = lambda planes, **kw: K.image(ce, planes, V.SUB_420, 8, **kw)  # noqa: E731
    same, inverted = gpu_ctx.plane_vif([img(ref)], [img(ref, layout=K.SEMIPLANAR), img(inv)], 82, 82, pair_ref=[0, 0])
    assert same.ran == (1, 1, 1) and all(abs(v - 1.0) < 1e-8 for v in same.vifp)
    assert inverted.num_q == ((0,) * 4,) * 3 and inverted.vifp == (0.0, 0.0, 0.0) and inverted.den_q == same.den_q
    VK.check(inverted, V.plane_vif(list(ref), inv, 8, V.SUB_420), "inverted")
    a, b = [np.full((41, 41), 90, np.uint8)], [np.full((41, 41), 93, np.uint8)]
    flat = gpu_ctx.plane_vif([K.image(ce, a, V.SUB_400, 8)], [K.image(ce, b, V.SUB_400, 8)], 41, 41)[0]
    assert flat.den_q[0] == (0,) * 4 and flat.vifp[0] == 1.0 and flat.vif_scale[0] == (1.0,) * 4 and flat.n_planes == 1 and np.isnan(flat.vifp[1])


def test_shared_references_a_repeat_and_the_other_calls_beside_it(ce, gpu_ctx):
    """Three semiplanar references on the host of which one is not named, three planar tests on the device, a pair table that is
    no identity; the call again; ce_yuv_plane_fidelity and ce_yuv_plane_hvs on the same images before and after; and a batch
    launch that is collected across the call"""
    w, h, sub = 131, 99, V.SUB_420
    refs = [K.image(ce, VK.planes(w, h, sub, 8, s)[0], sub, 8, K.SEMIPLANAR, pad=5) for s in (0, 3, 1)]
    seeds, table, ref_seeds = (1, 0, 2), [2, 0, 2], (1, 0, 1)
    keep, tests = [], []
    for s in seeds:
        dev, t = K.on_device(ce, K.image(ce, VK.planes(w, h, sub, 8, s)[1], sub, 8, pad=1))
        keep.append(t), tests.append(dev)
    wants = [VK.expected(w, h, sub, 8, s, r) for s, r in zip(seeds, ref_seeds)]
    fidelity = K.key(gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table, levels=1))
    hvs = K.key(gpu_ctx.plane_hvs(refs, tests, w, h, pair_ref=table, step=7))
    rng = np.random.default_rng(8)
    rgb_ref = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    rgb_test = np.clip(rgb_ref.astype(np.int32) + rng.integers(-9, 10, rgb_ref.shape), 0, 255).astype(np.uint8)
    cfg = ce.MetricConfig.all()
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference(0, rgb_ref)
        b.set_test(0, 0, rgb_test)
        scores = b.run(1, cfg)
        b.launch(1, cfg)
        got = gpu_ctx.plane_vif(refs, tests, w, h, pair_ref=table)
        again = b.collect(1)
        key = lambda s: (VK.bits(s.dssim), VK.bits(s.ssimulacra2), VK.bits(s.butteraugli), VK.bits(s.psnr), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in scores] and again[0].valid == 15
    finally:
        b.close()
    for i in range(3):
        VK.check(got[i], wants[i], i)
    assert K.key(gpu_ctx.plane_vif(refs, tests, w, h, pair_ref=table)) == K.key(got)
    assert K.key(gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table, levels=1)) == fidelity
    assert K.key(gpu_ctx.plane_hvs(refs, tests, w, h, pair_ref=table, step=7)) == hvs
    # pairs 1 and 0 alone with an identity table and with none: a pair's result does not depend on who shares the call
    two = [refs[0], refs[2]]
    assert K.key(gpu_ctx.plane_vif(two, [tests[1], tests[0]], w, h, pair_ref=[0, 1])) == K.key([got[1], got[0]])
    assert K.key(gpu_ctx.plane_vif(two, [tests[1], tests[0]], w, h)) == K.key([got[1], got[0]])


def test_65536_pairs_against_one_reference_split_into_whole_pairs(ce, gpu_ctx):
    """Grid y is (pair, plane) and holds 65535: 65536 pairs of 41 x 41 4:0:0, three device images repeated, take two launches of
    either kernel at every scale; every result equals its image's"""
    w = h = 41
    n = 65536
    ref = K.image(ce, VK.planes(w, h, V.SUB_400, 8, 0)[0], V.SUB_400, 8)
    keep, three = [], (ce.CeYuvImage * 3)()
    for s in range(3):
        dev, buffers = K.on_device(ce, K.image(ce, VK.planes(w, h, V.SUB_400, 8, s)[1], V.SUB_400, 8, pad=7))
        three[s], k = dev._c()
        keep += [buffers, k]
    tests = (ce.CeYuvImage * n)()
    for i in range(n):
        tests[i] = three[i % 3]
    refs = (ce.CeYuvImage * 1)()
    refs[0], k = ref._c()
    table = (C.c_uint32 * n)()
    out = (ce.CePlaneVifScores * n)()
    assert ce.lib().ce_yuv_plane_vif(gpu_ctx._h, w, h, refs, 1, tests, n, table, out) == ce.CE_OK, gpu_ctx._err()
    raw = np.frombuffer(out, np.uint8).reshape(n, C.sizeof(ce.CePlaneVifScores))
    for s in range(3):
        VK.check(ce.PlaneVifScores.from_c(out[s]), VK.expected(w, h, V.SUB_400, 8, s, 0), s)
        assert (raw[s::3] == raw[s]).all(), s
    VK.check(ce.PlaneVifScores.from_c(out[n - 1]), VK.expected(w, h, V.SUB_400, 8, (n - 1) % 3, 0), "the last launch's pair")
    assert out[0].num_q[0][0] != out[1].num_q[0][0] != out[2].num_q[0][0]


def test_every_refusal_names_its_reason_and_leaves_the_context_usable(ce, gpu_ctx):
    w, h, sub = 90, 84, V.SUB_420
    ref, test = VK.planes(w, h, sub, 8)
    want = VK.expected(w, h, sub, 8)
    L = ce.lib()
    keep = []

    def c_of(images):
        arr = (ce.CeYuvImage * len(images))()
        for i, img in enumerate(images):
            arr[i], k = img._c()
            keep.append(k)
        return arr

    good_r, good_t = K.image(ce, ref, sub, 8), K.image(ce, test, sub, 8, K.SEMIPLANAR)
    out = (ce.CePlaneVifScores * 4)()

    def call(refs, n_refs, tests, n_pairs, table, width=w, height=h, out=out):
        t = None if table is None else (C.c_uint32 * len(table))(*table)
        return L.ce_yuv_plane_vif(gpu_ctx._h, width, height, refs, n_refs, tests, n_pairs, t, out)

    def refused(rc, word):
        assert rc == ce.CE_ERR_INVALID_ARG and word in gpu_ctx._err() and "plane vif" in gpu_ctx._err(), (rc, word, gpu_ctx._err())
        VK.check(gpu_ctx.plane_vif([good_r], [good_t], w, h)[0], want, "after " + word)

    r1, t1, t2 = c_of([good_r]), c_of([good_t]), c_of([good_t, good_t])
    refused(call(None, 1, t1, 1, None), "null")
    refused(call(r1, 1, None, 1, None), "null")
    refused(call(r1, 1, t1, 1, None, out=None), "null")
    refused(call(r1, 1, t1, 0, None), "no references or no pairs")
    refused(call(r1, 0, t1, 1, [0]), "no references or no pairs")
    refused(call(r1, 1, t2, 2, [0, 1]), "names reference 1")
    refused(call(r1, 1, t2, 2, None), "pair table")
    refused(call(r1, 1, t1, 1, None, 0, h), "empty")
    refused(call(r1, 1, t1, 1, None, w, 0), "empty")
    refused(call(r1, 1, t1, 1, None, 40, h), "under 41 x 41")  # the images are checked at the call's size first, so give it planes
    refused(call(r1, 1, t1, 1, None, w, 40), "under 41 x 41")
    assert call(r1, 1, t1, 1, None, 41, 41) == ce.CE_OK  # ... and 41 runs: luma alone, chroma 21 x 21 does not
    assert tuple(out[0].ran) == (1, 0, 0) and out[0].n_pos[0][3] == 1 and np.isnan(out[0].vifp[1])
    # images of one call that disagree, and pairs that do
    refused(call(r1, 1, c_of([K.image(ce, K.planes(w, h, V.SUB_444, 8)[1], V.SUB_444, 8)]), 1, None), "subsampling or depth")
    refused(call(r1, 1, c_of([K.image(ce, K.planes(w, h, sub, 10)[1], sub, 10)]), 1, None), "subsampling or depth")
    refused(call(r1, 1, c_of([K.image(ce, test, sub, 8, matrix=ce.YUV_BT709)]), 1, None), "matrix or range")
    refused(call(r1, 1, c_of([K.image(ce, test, sub, 8, range=ce.YUV_LIMITED)]), 1, None), "matrix or range")

    # what the ingest's own check refuses (its reasons are its own)
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

    def refused_by_the_ingest(rc, word):
        assert rc == ce.CE_ERR_INVALID_ARG and word in gpu_ctx._err(), (rc, word, gpu_ctx._err())
        VK.check(gpu_ctx.plane_vif([good_r], [good_t], w, h)[0], want, "after " + word)

    refused_by_the_ingest(call(r1, 1, broken(plane1=None), 1, None), "missing")
    refused_by_the_ingest(call(r1, 1, broken(subsampling=7), 1, None), "subsampling")
    refused_by_the_ingest(call(r1, 1, broken(layout=2), 1, None), "layout")
    refused_by_the_ingest(call(r1, 1, broken(matrix=9), 1, None), "matrix")
    refused_by_the_ingest(call(r1, 1, broken(range=5), 1, None), "range")
    refused_by_the_ingest(call(r1, 1, broken(upsample=4), 1, None), "upsampling")
    refused_by_the_ingest(call(r1, 1, broken(memory=3), 1, None), "memory")
    refused_by_the_ingest(call(r1, 1, broken(depth=9), 1, None), "depth")
    refused_by_the_ingest(call(r1, 1, broken(msb_aligned=1), 1, None), "msb_aligned")
    refused_by_the_ingest(call(r1, 1, broken(pitch0=w - 1), 1, None), "pitch")
    refused_by_the_ingest(call(r1, 1, broken(lut=8), 1, None), "colour table")
    r10, t10 = K.planes(w, h, sub, 10)
    odd = c_of([K.image(ce, t10, sub, 10)])
    odd[0].pitch[0] = 2 * w + 1
    refused_by_the_ingest(call(c_of([K.image(ce, r10, sub, 10)]), 1, odd, 1, None), "2-byte aligned")
    assert L.ce_yuv_plane_vif(None, w, h, r1, 1, t1, 1, None, out) == ce.CE_ERR_INVALID_ARG
    assert C.sizeof(ce.CePlaneVifScores) == 424
