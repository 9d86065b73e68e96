"""HDR fidelity on the device (ce_batch_hdr_fidelity, ce_eval_pair_hdr_fidelity).  The definition is made
of integers and correctly rounded IEEE operations, so the device must equal the numpy restatement
(tests/hdr_fidelity_restatement.py) exactly: the three integers of every pair, and the three doubles finished from them to the
bit - on both load paths, with one and with several blocks a pair, at every depth and white, on PQ content and on the
wide-content classes (negatives, values above PQ's peak, subnormals), through the pair -> reference table, whatever slot a pair
sits in and however often it is asked."""
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import hdr_fidelity_cases as K  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def assert_equal(got, want, what):
    assert (got.pq_sse, got.itp_sum_q20, got.itp_max_q20) == (want["pq_sse"], want["itp_sum_q20"], want["itp_max_q20"]), what
    for name in ("pq_psnr", "delta_e_itp_mean", "delta_e_itp_max"):
        assert bits(getattr(got, name)) == bits(want[name]), (what, name, getattr(got, name), want[name])


def load(ce, ctx, w, h, pairs):
    """The pairs as one linear batch, a reference slot per distinct reference array."""
    refs = []
    for _, ref, _ in pairs:
        if not any(r is ref for r in refs):
            refs.append(ref)
    b = ctx.batch_linear(w, h, len(refs), len(pairs))
    for i, r in enumerate(refs):
        b.set_reference(i, r)
    for p, (_, ref, test) in enumerate(pairs):
        b.set_test(p, next(i for i, r in enumerate(refs) if r is ref), test)
    return b


@pytest.mark.parametrize("shape_index", range(len(K.shape_cases())), ids=["%dx%d" % c[:2] for c in K.shape_cases()])
def test_batch_equals_restatement_exactly(ce, gpu_ctx, shape_index):
    w, h, params, pairs = K.shape_cases()[shape_index]
    b = load(ce, gpu_ctx, w, h, pairs)
    try:
        for depth, white in params:
            got = b.hdr_fidelity(len(pairs), depth, white)
            want = K.expected(shape_index, depth, white)
            for p, (name, _, _) in enumerate(pairs):
                assert_equal(got[p], want[p], (w, h, depth, white, p, name))
            assert any(g.pq_sse > 0 and g.itp_max_q20 > 0 for g in got)
    finally:
        b.close()


def test_cicp_ingested_pair(ce, gpu_ctx):
    """BT.2020 PQ code values through set_*_cicp: the scores of what the device's ingest wrote equal the restatement's on the
    restated ingest, and PQ-PSNR is the integer PSNR of the codes to 1e-3 dB."""
    w, h, depth, white = 96, 64, 10, 203.0
    ref, test = K.pq_pair(w, h, depth, white, 31, noise=6)
    colour = ce.ColourDescription(ce.PRIMARIES_BT2020, ce.TRANSFER_PQ, depth, white)
    b = gpu_ctx.batch_linear(w, h, 1, 1)
    try:
        b.set_reference_cicp(0, ref, colour)
        b.set_test_cicp(0, 0, test, colour)
        got = b.hdr_fidelity(1, depth, white)[0]
    finally:
        b.close()
    assert_equal(got, F.fidelity(R.to_linear(ref, 9, 16, depth, white), R.to_linear(test, 9, 16, depth, white), depth, white), "cicp")
    d = ref.astype(np.int64) - test.astype(np.int64)
    plain = 10.0 * math.log10(1023.0 ** 2 / (float((d * d).sum()) / d.size))
    print(f"pq_psnr {got.pq_psnr!r}, integer PSNR of the codes {plain!r}")
    assert abs(got.pq_psnr - plain) <= 1e-3


def test_pair_ref_indirection_slots_and_repeats(ce, gpu_ctx):
    """3 references and 7 tests bound out of order; the same call twice; the pairs placed in other slots of another batch."""
    w, h, depth, white = 20, 13, 12, 203.0  # 260 pixels: the wide path, one block and a partly idle wave
    imgs = [K.pq_linear(w, h, 12, white, 40 + i) for i in range(7)]
    refs = [imgs[i][0] for i in range(3)]
    binding = [2, 0, 1, 1, 2, 0, 2]
    tests = [imgs[i][1] for i in range(7)]
    want = [F.fidelity(refs[binding[p]], tests[p], depth, white) for p in range(7)]
    b = gpu_ctx.batch_linear(w, h, 3, 7)
    try:
        for p in (5, 2, 6, 0, 3, 1, 4):  # tests first, out of order, then the references
            b.set_test(p, binding[p], tests[p])
        for i in (1, 2, 0):
            b.set_reference(i, refs[i])
        first = b.hdr_fidelity(7, depth, white)
        second = b.hdr_fidelity(7, depth, white)
        assert first == second
        for p in range(7):
            assert_equal(first[p], want[p], p)
        assert b.hdr_fidelity(3, depth, white) == first[:3]
        b.bind_pair(0, 1)  # rebinding alone reaches the device
        assert_equal(b.hdr_fidelity(1, depth, white)[0], F.fidelity(refs[1], tests[0], depth, white), "rebound")
    finally:
        b.close()
    order = [3, 6, 0, 5, 1, 4, 2]  # slot s of the second batch holds pair order[s], its references in other slots too
    b2 = gpu_ctx.batch_linear(w, h, 4, 9)
    try:
        for i in range(3):
            b2.set_reference(3 - i, refs[i])
        for s, p in enumerate(order):
            b2.set_test(s, 3 - binding[p], tests[p])
        moved = b2.hdr_fidelity(7, depth, white)
    finally:
        b2.close()
    assert [moved[s] for s in range(7)] == [first[p] for p in order]


def test_leaf_equals_batch_and_sanitises(ce, gpu_ctx):
    w, h, params, pairs = K.shape_cases()[2]  # 97 x 35
    depth, white = params[2]
    want = K.expected(2, depth, white)
    for p in (0, len(pairs) - 1):
        assert_equal(gpu_ctx.hdr_fidelity(pairs[p][1], pairs[p][2], w, h, depth, white), want[p], p)
    ref = pairs[-1][1].copy()
    ref[0, 0] = (np.nan, 5000.0, -5000.0)  # the ingest of a linear image: NaN -> 0, the clamp to +-1024
    clean = ref.copy()
    clean[0, 0] = (0.0, 1024.0, -1024.0)
    assert gpu_ctx.hdr_fidelity(ref, pairs[-1][2], w, h, depth, white) == gpu_ctx.hdr_fidelity(clean, pairs[-1][2], w, h, depth, white)


def test_refusals_leave_the_batch_usable(ce, gpu_ctx):
    w, h, params, pairs = K.shape_cases()[2]  # 97 x 35
    depth, white = params[0]
    b = load(ce, gpu_ctx, w, h, pairs[:2])
    try:
        before = b.hdr_fidelity(2, depth, white)
        out = (ce.CeHdrScores * 4)()
        L = ce.lib()
        for args in ((2, 8, white), (2, 14, white), (2, depth, 0.0), (2, depth, -203.0), (2, depth, math.inf), (2, depth, math.nan),
                     (0, depth, white), (3, depth, white)):
            assert L.ce_batch_hdr_fidelity(b._h, args[0], args[1], args[2], out) == ce.CE_ERR_INVALID_ARG, args
            assert gpu_ctx._err() != ""
        assert L.ce_batch_hdr_fidelity(b._h, 2, depth, white, None) == ce.CE_ERR_INVALID_ARG
        assert L.ce_batch_hdr_fidelity(None, 2, depth, white, out) == ce.CE_ERR_INVALID_ARG
        assert b.hdr_fidelity(2, depth, white) == before
        # a batch that is not linear
        plain = ce.Batch(gpu_ctx, w, h, 1, 1)
        deep = gpu_ctx.batch_deep(w, h, 1, 1, 10, 10)
        try:
            for other in (plain, deep):
                with pytest.raises(ce.CodecEvalError) as e:
                    other.hdr_fidelity(1, depth, white)
                assert e.value.status == ce.CE_ERR_INVALID_ARG and "linear" in str(e.value)
        finally:
            plain.close()
            deep.close()
        # the leaf: wrong lengths, null pointers, an empty image
        r, t = pairs[0][1], pairs[0][2]
        one = ce.CeHdrScores()
        assert L.ce_eval_pair_hdr_fidelity(gpu_ctx._h, r.ctypes.data, r.nbytes - 4, t.ctypes.data, t.nbytes, w, h, depth, white, one) == ce.CE_ERR_BAD_LENGTH
        assert L.ce_eval_pair_hdr_fidelity(gpu_ctx._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes + 12, w, h, depth, white, one) == ce.CE_ERR_BAD_LENGTH
        assert L.ce_eval_pair_hdr_fidelity(gpu_ctx._h, None, r.nbytes, t.ctypes.data, t.nbytes, w, h, depth, white, one) == ce.CE_ERR_INVALID_ARG
        assert L.ce_eval_pair_hdr_fidelity(gpu_ctx._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, 0, h, depth, white, one) == ce.CE_ERR_INVALID_ARG
        assert L.ce_eval_pair_hdr_fidelity(gpu_ctx._h, r.ctypes.data, r.nbytes, t.ctypes.data, t.nbytes, w, h, 11, white, one) == ce.CE_ERR_INVALID_ARG
        assert gpu_ctx.hdr_fidelity(r, t, w, h, depth, white) == before[0]
        # what a launch left to collect is untouched by a call made in between
        dssim = ce.MetricConfig(dssim=True)
        scores = b.run(2, dssim)
        b.launch(2, dssim)
        assert b.hdr_fidelity(2, depth, white) == before
        again = b.collect(2)
        assert [(bits(s.dssim), s.valid, s.status) for s in again] == [(bits(s.dssim), s.valid, s.status) for s in scores]
        assert all(s.valid == ce.METRIC_DSSIM for s in again)
    finally:
        b.close()
