"""PSNR-HVS / PSNR-HVS-M of a decoder's Y'CbCr planes on the device (ce_yuv_plane_hvs).  Everything the
device returns is an exact integer, so every integer of every pair must equal the numpy restatement
(tests/plane_hvs_restatement.py) and the doubles finished from them within 1e-14 relative (libm's log10 may differ): on the
shapes of tests/plane_hvs_cases.py, each one way for the kernel to go wrong, with host and device planes, planar and
semiplanar layouts, MSB-aligned samples, depths 8, 10 and 12 and odd pitches; shared references; a repeat; beside a launch and
beside ce_yuv_plane_fidelity; every refusal."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_hvs_cases as HK  # noqa: E402
import plane_hvs_restatement as H  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h,sub,depth,step,layout,msb", HK.SHAPES, ids=lambda v: str(v))
def test_every_shape_equals_the_restatement_on_host_and_device_planes(ce, gpu_ctx, w, h, sub, depth, step, layout, msb):
    """One planar reference on the host; the test image four times: on the host in the shape's layout with an odd pitch, on the
    device with another pitch at an aligned and at an unaligned base, and on the host in the other layout"""
    ref, test = HK.planes(w, h, sub, depth)
    want = HK.expected(w, h, sub, depth, step)
    bps = 1 if depth == 8 else 2
    other = K.PLANAR if layout == K.SEMIPLANAR else K.SEMIPLANAR
    keep, tests = [], [K.image(ce, test, sub, depth, layout, msb, pad=bps)]
    for offset in (0, bps):
        dev, buffers = K.on_device(ce, K.image(ce, test, sub, depth, layout, msb, pad=3 * bps), offset)
        keep.append(buffers), tests.append(dev)
    tests.append(K.image(ce, test, sub, depth, other, False, pad=0))
    got = gpu_ctx.plane_hvs([K.image(ce, ref, sub, depth)], tests, w, h, pair_ref=[0] * len(tests), step=step)
    for i, g in enumerate(got):
        HK.check(g, want, (w, h, sub, depth, step, i))
    assert got[0].hvs_sum[0] > 0 and got[0].n_blocks[0] == H.n_blocks_of(w, h, step)
    print(f"{w} x {h} sub {sub} depth {depth} step {step}: blocks {got[0].n_blocks} hvs {got[0].psnr_hvs!r} hvsm {got[0].psnr_hvsm!r}")


def test_a_chroma_plane_without_a_block_and_an_identical_pair(ce, gpu_ctx):
    ref, test = HK.planes(8, 8, H.SUB_420, 8)
    got = gpu_ctx.plane_hvs([K.image(ce, ref, H.SUB_420, 8)], [K.image(ce, test, H.SUB_420, 8), K.image(ce, ref, H.SUB_420, 8, K.SEMIPLANAR)],
                            8, 8, pair_ref=[0, 0])
    assert got[0].n_blocks == (1, 0, 0) and got[0].n_planes == 3 and got[0].hvs_q[1] == got[0].hvsm_q[2] == (0, 0)
    assert np.isnan(got[0].psnr_hvs[1]) and np.isnan(got[0].psnr_hvsm[2]) and np.isfinite(got[0].psnr_hvs[0])
    assert got[1].hvs_sum == got[1].hvsm_sum == (0, 0, 0) and got[1].psnr_hvs[0] == got[1].psnr_hvsm[0] == np.inf and np.isnan(got[1].psnr_hvs[1])
    # black against white: the anchor of the definition
    a, b = [np.zeros((8, 8), np.uint8)], [np.full((8, 8), 255, np.uint8)]
    bw = gpu_ctx.plane_hvs([K.image(ce, a, H.SUB_400, 8)], [K.image(ce, b, H.SUB_400, 8)], 8, 8)[0]
    assert bw.hvs_sum[0] == bw.hvsm_sum[0] == 11289420915398 and abs(bw.psnr_hvs[0] - -4.1281) < 5e-5 and bw.n_planes == 1


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_shared_references_a_repeat_and_the_other_calls_beside_it(ce, gpu_ctx):
    """Two semiplanar references on the host, three planar tests on the device, a pair table that is no identity; the call
    again; ce_yuv_plane_fidelity on the same images before and after; and a batch launch that is collected across the call"""
    w, h, sub, step = 93, 67, H.SUB_420, 7
    refs = [K.image(ce, HK.planes(w, h, sub, 8, s)[0], sub, 8, K.SEMIPLANAR, pad=5) for s in (0, 1)]
    seeds, table = (1, 0, 2), [1, 0, 1]
    keep, tests = [], []
    for s in seeds:
        dev, t = K.on_device(ce, K.image(ce, HK.planes(w, h, sub, 8, s)[1], sub, 8, pad=1))
        keep.append(t), tests.append(dev)
    wants = [HK.expected(w, h, sub, 8, step, s, r) for s, r in zip(seeds, table)]
    fidelity = K.key(gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table, levels=1))
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
        got = gpu_ctx.plane_hvs(refs, tests, w, h, pair_ref=table, step=step)
        again = b.collect(1)
        key = lambda s: (bits(s.dssim), bits(s.ssimulacra2), bits(s.butteraugli), bits(s.psnr), s.valid, s.status)  # noqa: E731
        assert [key(s) for s in again] == [key(s) for s in scores] and again[0].valid == 15
    finally:
        b.close()
    for i in range(3):
        HK.check(got[i], wants[i], i)
    assert gpu_ctx.plane_hvs(refs, tests, w, h, pair_ref=table, step=step) == got
    assert K.key(gpu_ctx.plane_fidelity(refs, tests, w, h, pair_ref=table, levels=1)) == fidelity
    # pairs 1 and 0 alone with the identity table and with none: a pair's result does not depend on who shares the call
    assert gpu_ctx.plane_hvs(refs, [tests[1], tests[0]], w, h, pair_ref=[0, 1], step=step) == [got[1], got[0]]
    assert gpu_ctx.plane_hvs(refs, [tests[1], tests[0]], w, h, step=step) == [got[1], got[0]]


def test_every_refusal_names_its_reason_and_leaves_the_context_usable(ce, gpu_ctx):
    w, h, sub = 40, 36, H.SUB_420
    ref, test = HK.planes(w, h, sub, 8)
    want = HK.expected(w, h, sub, 8, 8)
    L = ce.lib()
    keep = []

    def c_of(images):
        arr = (ce.CeYuvImage * len(images))()
        for i, img in enumerate(images):
            arr[i], k = img._c()
            keep.append(k)
        return arr

    good_r, good_t = K.image(ce, ref, sub, 8), K.image(ce, test, sub, 8, K.SEMIPLANAR)
    out = (ce.CePlaneHvsScores * 4)()

    def call(refs, n_refs, tests, n_pairs, table, step=8, width=w, height=h, out=out):
        t = None if table is None else (C.c_uint32 * len(table))(*table)
        return L.ce_yuv_plane_hvs(gpu_ctx._h, width, height, refs, n_refs, tests, n_pairs, t, step, out)

    def refused(rc, word):
        assert rc == ce.CE_ERR_INVALID_ARG and word in gpu_ctx._err() and "plane hvs" in gpu_ctx._err(), (rc, word, gpu_ctx._err())
        HK.check(gpu_ctx.plane_hvs([good_r], [good_t], w, h)[0], want, "after " + word)

    r1, t1, t2 = c_of([good_r]), c_of([good_t]), c_of([good_t, good_t])
    refused(call(None, 1, t1, 1, None), "null")
    refused(call(r1, 1, None, 1, None), "null")
    refused(call(r1, 1, t1, 1, None, out=None), "null")
    refused(call(r1, 1, t1, 0, None), "no references or no pairs")
    refused(call(r1, 0, t1, 1, [0]), "no references or no pairs")
    refused(call(r1, 1, t2, 2, [0, 1]), "names reference 1")
    refused(call(r1, 1, t2, 2, None), "pair table")
    for step in (0, 9, 16):
        refused(call(r1, 1, t1, 1, None, step), "step")
    refused(call(r1, 1, t1, 1, None, 8, 0, h), "empty")
    refused(call(r1, 1, t1, 1, None, 8, w, 0), "empty")
    refused(call(r1, 1, t1, 1, None, 8, 7, 36), "8 x 8")  # the images are checked at the call's size first, so give it planes
    refused(call(r1, 1, t1, 1, None, 8, 40, 6), "8 x 8")
    # images of one call that disagree, and pairs that do
    refused(call(r1, 1, c_of([K.image(ce, K.planes(w, h, H.SUB_444, 8)[1], H.SUB_444, 8)]), 1, None), "subsampling or depth")
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
        HK.check(gpu_ctx.plane_hvs([good_r], [good_t], w, h)[0], want, "after " + word)

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
    assert L.ce_yuv_plane_hvs(None, w, h, r1, 1, t1, 1, None, 8, out) == ce.CE_ERR_INVALID_ARG
    assert C.sizeof(ce.CePlaneHvsScores) == 176
