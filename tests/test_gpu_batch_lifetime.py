"""A batch's device memory over its whole life (ce_owned.h, the working sets of ce_internal.h): everything a batch ever
allocates - slabs, staging, the three metrics' working sets and what later launches add on first use (SSIMULACRA2's reference
planes of the split path and its maps, Butteraugli's diffmaps and its half-resolution chain's scratch, the readouts' cell
buffers, a linear batch's HDR fidelity and Delta E ITP buffers) - goes back to the device when the batch is destroyed, and a
new batch of the same shape on the same context computes the same bits.

Drift: ten cycles of create, fill, launch twice, collect, read one map of each kind, destroy; the device's free bytes after
each destroy.  Freed memory may stay in the runtime's pools at some granularity, so the bound is not zero: from cycle 2 (cycle
1 also fills the context's tables, streams and helper threads) to cycle 10 free memory may drop by less than what ONE cycle
holds, measured in the same cycles as free-before-create minus free-after-launch.  The device reports free memory in 2 MiB
steps and a cycle holds 10 - 12 MiB here, so eight cycles that each keep an eighth of that show; the commit before the owners
measured 0 bytes of drift on both batch kinds under the same bound, and so does this one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_fidelity_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, REFS, PAIRS, CYCLES = 72, 40, 2, 3, 10
PAIR_REF = (0, 0, 1)  # two pairs on one reference: the second launch of a cycle takes SSIMULACRA2's split path
THRESHOLDS = [1 << 18, 1 << 20, 1 << 22]


def _images(workloads, linear):
    if linear:
        pairs = [K.pq_linear(W, H, 10, 203.0, 61 + r) for r in range(REFS)]
        refs = [p[0] for p in pairs]
        tests = [pairs[0][1], K.pq_linear(W, H, 10, 203.0, 61, noise=90)[1], pairs[1][1]]
        return refs, tests
    refs = [workloads.make_reference(W, H, 31 + r) for r in range(REFS)]
    return refs, [workloads.distort(refs[r], q) for r, q in zip(PAIR_REF, (35, 70, 50))]


def _score_bits(scores):
    return [tuple(int(np.float64(v).view(np.uint64)) for v in (s.dssim, s.ssimulacra2, s.butteraugli, s.psnr)) + (s.valid, s.status)
            for s in scores]


def _cycle(ce, ctx, refs, tests, linear):
    """One life of a batch: (everything it computed, as bits; bytes it held after its launches; free bytes after destroy)."""
    free_before = ctx.memory_info()[0]
    b = ce.Batch(ctx, W, H, REFS, PAIRS, linear=linear)
    try:
        for r, img in enumerate(refs):
            b.set_reference(r, img)
        for p, img in enumerate(tests):
            b.set_test(p, PAIR_REF[p], img)
        got = []
        for _ in range(2):  # the second launch finds the references kept: SSIMULACRA2 builds the split path's planes
            b.launch(PAIRS, ce.MetricConfig.all(), butteraugli_diffmap=True, ssimulacra2_maps=True)
            got.append(_score_bits(b.collect(PAIRS)))
        got.append(b.butteraugli_diffmaps(0, PAIRS, block=8).tobytes())
        maps, ssim = b.dssim_ssim_maps(1, 0, PAIRS, block=2)
        got += [maps.tobytes(), ssim.tobytes()]
        maps, norms = b.ssimulacra2_maps(1, 0, 1, 0, PAIRS, block=4)
        got += [maps.tobytes(), norms.tobytes()]
        if linear:
            got.append([(s.pq_sse, s.itp_sum_q20, s.itp_max_q20) for s in b.hdr_fidelity(PAIRS, 10, 203.0)])
            maps, over = b.delta_e_itp_maps(0, PAIRS, 10, 203.0, block=4, thresholds_q20=THRESHOLDS)
            got += [maps.tobytes(), over.tobytes()]
        held = free_before - ctx.memory_info()[0]
    finally:
        b.close()
    return got, held, ctx.memory_info()[0]


@pytest.fixture(scope="module", params=[False, True], ids=["rgb8", "linear"])
def lives(request, ce, workloads):
    """CYCLES lives of one batch shape on a context of their own: [(results, held, free after destroy)]."""
    linear = request.param
    refs, tests = _images(workloads, linear)
    with ce.Context(0) as ctx:
        return [_cycle(ce, ctx, refs, tests, linear) for _ in range(CYCLES)]


def test_destroy_returns_what_a_batch_held(lives):
    held = [h for _, h, _ in lives]
    free = [f for _, _, f in lives]
    drift = free[1] - free[CYCLES - 1]  # cycle 2 -> cycle 10
    print("held per cycle", held, "free after destroy", free, "drift", drift)
    one_cycle = min(held[1:])
    assert one_cycle > 0, "a cycle that holds nothing measures nothing"
    assert drift < one_cycle


def test_new_batch_after_destroy_computes_the_same_bits(lives):
    first = lives[0][0]
    for k, (got, _, _) in enumerate(lives[1:], start=2):
        assert got == first, "life %d of the batch differs from the first" % k
    assert first[0] == first[1], "the launch on the split path differs from the one before it"
