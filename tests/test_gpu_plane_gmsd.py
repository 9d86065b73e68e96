"""GMSD of a decoder's Y'CbCr planes on the device (ce_yuv_plane_gmsd).  Everything the device returns is
an exact integer, so every integer of every pair must equal the numpy restatement (tests/plane_gmsd_restatement.py) and the
doubles finished from them as tests/plane_gmsd_cases.py compares them: on its shapes, each one way for the kernel to go wrong,
with host and device planes, device planes at an aligned base and one sample off it, planar and semiplanar layouts,
MSB-aligned samples, depths 8, 10 and 12 and odd pitches; shared references; a repeat; the identical and the flat-test pair;
beside a launch and beside ce_yuv_plane_fidelity and ce_yuv_plane_hvs, which share its result scratch; every refusal."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_gmsd_cases as GK  # noqa: E402
import plane_gmsd_restatement as G  # noqa: E402
import plane_hvs_cases as HK  # noqa: E402

pytestmark = pytest.mark.gpu
TWO32 = 1 << 32


@pytest.mark.parametrize("w,h,sub,depth,layout,msb", GK.SHAPES, ids=lambda v: str(v))
def test_every_shape_equals_the_restatement_on_host_and_device_planes(ce, gpu_ctx, w, h, sub, depth, layout, msb):
    """One planar reference on the host; the test image four times: on the host in the shape's layout with an odd pitch, on the
    device with another pitch at an aligned and at an unaligned base, and on the host in the other layout.  Then the same
    reference on the device with rows 16 bytes apart against a test laid out alike - every row on the wide path - and the
    flat test against it."""
    ref, test = GK.planes(w, h, sub, depth)
    want = GK.expected(w, h, sub, depth)
    bps = 1 if depth == 8 else 2
    other = K.PLANAR if layout == K.SEMIPLANAR else K.SEMIPLANAR
    keep, tests = [], [K.image(ce, test, sub, depth, layout, msb, pad=bps)]
    for offset in (0, bps):
        dev, buffers = K.on_device(ce, K.image(ce, test, sub, depth, layout, msb, pad=3 * bps), offset)
        keep.append(buffers), tests.append(dev)
    tests.append(K.image(ce, test, sub, depth, other, False, pad=0))
    got = gpu_ctx.plane_gmsd([K.image(ce, ref, sub, depth)], tests, w, h, pair_ref=[0] * len(tests))
    for i, g in enumerate(got):
        GK.check(g, want, (w, h, sub, depth, i))
    assert got[0].n_pos[0] == ((w + 1) // 2) * ((h + 1) // 2) and got[0].sum_q[0] > 0
    # device planes whose every row starts on 16 bytes: the wide path throughout
    flat = GK.planes(w, h, sub, depth, 0, GK.FLAT_TEST)[1]
    wide = []
    for samples in (ref, test, flat):
        pl = GK.stored_planes(samples, sub, depth, layout, msb)
        img = ce.YuvImage(pl, subsampling=sub, layout=layout, depth=depth, msb_aligned=msb, pitches=[K.pitch_of(p) for p in pl])
        dev, buffers = K.on_device(ce, img)
        keep.append(buffers), wide.append(dev)
    aligned = gpu_ctx.plane_gmsd(wide[:1], wide[1:], w, h, pair_ref=[0, 0])
    GK.check(aligned[0], want, (w, h, sub, depth, "wide"))
    GK.check(aligned[1], GK.expected(w, h, sub, depth, 0, None, GK.FLAT_TEST), (w, h, sub, depth, "wide, flat test"))
    print(f"{w} x {h} sub {sub} depth {depth}: n_pos {got[0].n_pos} gmsd {got[0].gmsd!r} gmsm {got[0].gmsm!r} max_dis {got[0].max_dis}")


def test_the_identical_pair_and_the_flat_test_pair(ce, gpu_ctx):
    for w, h, sub, depth in ((93, 67, G.SUB_420, 8), (93, 67, G.SUB_422, 12), (2, 2, G.SUB_420, 8)):
        ref, flat = GK.planes(w, h, sub, depth, 0, GK.FLAT_TEST)
        got = gpu_ctx.plane_gmsd([K.image(ce, ref, sub, depth)], [K.image(ce, ref, sub, depth, K.SEMIPLANAR, pad=2), K.image(ce, flat, sub, depth)],
                                 w, h, pair_ref=[0, 0])
        same, low = got
        for p in range(3):
            n = same.n_pos[p]
            assert n > 0 and same.sum_q[p] == n * TWO32 and same.sum_q2[p] == (0, n) and same.sum_q2_int[p] == n << 64 and same.max_dis[p] == 0
            assert same.gmsd[p] == 0.0 and same.gmsm[p] == 1.0
        GK.check(low, GK.expected(w, h, sub, depth, 0, None, GK.FLAT_TEST), (w, h, sub, depth, "flat test"))
        if w > 2:
            assert all(low.gmsd[p] > 0.2 and low.max_dis[p] > 0.9 * TWO32 for p in range(3))
    one = gpu_ctx.plane_gmsd([K.image(ce, [np.array([[7]], np.uint8)], G.SUB_400, 8)], [K.image(ce, [np.array([[200]], np.uint8)], G.SUB_400, 8)], 1, 1)[0]
    assert one.n_planes == 1 and one.n_pos == (1, 0, 0) and one.sum_q == (TWO32, 0, 0) and one.sum_q2[0] == (0, 1) and one.gmsd[0] == 0.0
    assert np.isnan(one.gmsd[1]) and np.isnan(one.gmsm[2]) and one.sum_q2[1] == (0, 0) and one.max_dis == (0, 0, 0)


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_shared_references_a_repeat_and_the_other_calls_beside_it(ce, gpu_ctx):
    """Two semiplanar references on the host, three planar tests on the device, a pair table that is no identity; the call
    again; ce_yuv_plane_fidelity and ce_yuv_plane_hvs on the same images before and after (they share the result scratch);
    and a batch launch that is collected across the call"""
    w, h, sub = 93, 67, G.SUB_420
    refs = [K.image(ce, GK.planes(w, h, sub, 8, s)[0], sub, 8, K.SEMIPLANAR, pad=5) for s in (0, 1)]
    seeds, table = (1, 0, 2), [1, 0, 1]
    keep, tests = [], []
    for s in seeds:
        dev, t = K.on_device(ce, K.image(ce, GK.planes(w, h, sub, 8, s)[1], sub, 8, pad=1))
        keep.append(t), tests.append(dev)
    wants = [GK.expected(w, h, sub, 8, s, r) for s, r in zip(seeds, table)]
    fidelity = K.key(gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table, levels=1))
    hvs = gpu_ctx.plane_hvs(refs, tests, w, h, pair_ref=table, step=7)
    for i, (s, r) in enumerate(zip(seeds, table)):
        HK.check(hvs[i], HK.expected(w, h, sub, 8, 7, s, r), ("hvs before", i))
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
        got = gpu_ctx.plane_gmsd(refs, tests, w, h, pair_ref=table)
        again = b.collect(1)
        key = lambda s: (bits(s.dssim), bits(s.ssimulacra2), bits(s.butteraugli), bits(s.psnr), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in scores] and again[0].valid == 15
    finally:
        b.close()
    for i in range(3):
        GK.check(got[i], wants[i], i)
    assert K.key(gpu_ctx.plane_gmsd(refs, tests, w, h, pair_ref=table)) == K.key(got)
    assert K.key(gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table, levels=1)) == fidelity
    assert gpu_ctx.plane_hvs(refs, tests, w, h, pair_ref=table, step=7) == hvs
    # pairs 1 and 0 alone with the identity table and with none: a pair's result does not depend on who shares the call
    assert K.key(gpu_ctx.plane_gmsd(refs, [tests[1], tests[0]], w, h, pair_ref=[0, 1])) == K.key([got[1], got[0]])
    assert K.key(gpu_ctx.plane_gmsd(refs, [tests[1], tests[0]], w, h)) == K.key([got[1], got[0]])


def test_every_refusal_names_its_reason_and_leaves_the_context_usable(ce, gpu_ctx):
    w, h, sub = 40, 36, G.SUB_420
    ref, test = GK.planes(w, h, sub, 8)
    want = GK.expected(w, h, sub, 8)
    L = ce.lib()
    keep = []

    def c_of(images):
        arr = (ce.CeYuvImage * len(images))()
        for i, img in enumerate(images):
            arr[i], k = img._c()
            keep.append(k)
        return arr

    good_r, good_t = K.image(ce, ref, sub, 8), K.image(ce, test, sub, 8, K.SEMIPLANAR)
    out = (ce.CePlaneGmsdScores * 4)()

    def call(refs, n_refs, tests, n_pairs, table, width=w, height=h, out=out):
        t = None if table is None else (C.c_uint32 * len(table))(*table)
        return L.ce_yuv_plane_gmsd(gpu_ctx._h, width, height, refs, n_refs, tests, n_pairs, t, out)

    def refused(rc, word):
        assert rc == ce.CE_ERR_INVALID_ARG and word in gpu_ctx._err() and gpu_ctx._err().startswith("plane gmsd: "), (rc, word, gpu_ctx._err())
        GK.check(gpu_ctx.plane_gmsd([good_r], [good_t], w, h)[0], want, "after " + word)

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
    # W2 * H2 = 2^32 exactly, and the largest luma there is
    refused(call(r1, 1, t1, 1, None, 1 << 17, 1 << 17), "2^32")
    refused(call(r1, 1, t1, 1, None, (1 << 17) - 1, 1 << 17), "2^32")
    refused(call(r1, 1, t1, 1, None, 0xffffffff, 0xffffffff), "2^32")
    # images of one call that disagree, and pairs that do
    refused(call(r1, 1, c_of([K.image(ce, K.planes(w, h, G.SUB_444, 8)[1], G.SUB_444, 8)]), 1, None), "subsampling or depth")
    refused(call(r1, 1, c_of([K.image(ce, K.planes(w, h, sub, 10)[1], sub, 10)]), 1, None), "subsampling or depth")
    refused(call(r1, 1, c_of([K.image(ce, test, sub, 8, matrix=ce.YUV_BT709)]), 1, None), "matrix or range")
    refused(call(r1, 1, c_of([K.image(ce, test, sub, 8, range=ce.YUV_LIMITED)]), 1, None), "matrix or range")

    # what the ingest's own check refuses: its words, behind the call's name
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

    refused(call(r1, 1, broken(plane1=None), 1, None), "missing")
    refused(call(r1, 1, broken(subsampling=7), 1, None), "subsampling")
    refused(call(r1, 1, broken(layout=2), 1, None), "layout")
    refused(call(r1, 1, broken(matrix=9), 1, None), "matrix")
    refused(call(r1, 1, broken(range=5), 1, None), "range")
    refused(call(r1, 1, broken(upsample=4), 1, None), "upsampling")
    refused(call(r1, 1, broken(memory=3), 1, None), "memory")
    refused(call(r1, 1, broken(depth=9), 1, None), "depth")
    refused(call(r1, 1, broken(msb_aligned=1), 1, None), "msb_aligned")
    refused(call(r1, 1, broken(pitch0=w - 1), 1, None), "pitch")
    refused(call(r1, 1, broken(lut=8), 1, None), "colour table")
    r10, t10 = K.planes(w, h, sub, 10)
    odd = c_of([K.image(ce, t10, sub, 10)])
    odd[0].pitch[0] = 2 * w + 1
    refused(call(c_of([K.image(ce, r10, sub, 10)]), 1, odd, 1, None), "2-byte aligned")
    assert L.ce_yuv_plane_gmsd(None, w, h, r1, 1, t1, 1, None, out) == ce.CE_ERR_INVALID_ARG
    assert C.sizeof(ce.CePlaneGmsdScores) == 160
