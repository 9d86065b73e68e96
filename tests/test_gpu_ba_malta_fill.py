"""The tile fill of Butteraugli's Malta kernel (codec-eval_amd/csrc/butteraugli.hip: k_ba_malta_l2_xy): the pre-scaling of a
position's X and Y samples as one pair, a thread's positions and in-image masks formed once for the three bands, a band's loads
requested together, and a block whose whole 72 x 40 region lies inside the image filling without predicates.  None of it may
change a bit: with the two device switches on (tests/test_gpu_butteraugli.py) the oracle's diffmap and score are the device's,
`==`, and its 3-norm within the tolerances of tests/test_gpu_ba_slot_order.py; a batch equals one-pair calls bit for bit.

A 64 x 32 tile with a halo of 4 has its region inside the image from 132 x 68 on (the tile at column 1, row 1).  Shapes: one tile
or less and four tiles with no interior one; either side of the first interior tile in each direction; a float4 group straddling
the right edge (w % 4 = 1, 2, 3) with the pitch beyond w; the same edges at the half-resolution level; the deep and linear
batches' operand ranges.  Every case has 2 references and 3 pairs (a padded work list, a reference serving two distorted images)
and runs with the diffmap flag (the instance that stores the map) and without it; every image with a half-resolution level also
runs the instance that writes the half-resolution map."""
import numpy as np
import pytest

import ba_diffmap_shim as S
import linear_input_shim as LS
from test_gpu_ba_slot_order import DEPTH, N_REFS, PNORM_REL, make_images, oracle_results

pytestmark = pytest.mark.gpu

N_PAIRS = 3
RGB8 = [(9, 9), (60, 30), (64, 32), (65, 33),  # one tile or less; four tiles, none interior
        (131, 68), (132, 68), (133, 68), (132, 67), (132, 69),  # either side of the first interior tile
        (133, 69), (134, 70), (135, 71),  # w % 4 = 1, 2, 3 with an interior tile
        (263, 135), (264, 136), (265, 137)]  # the same at the half-resolution level (132 x 68, 132 x 68, 133 x 69)
CASES = [("rgb8", w, h) for w, h in RGB8] + [(k, w, h) for k in ("deep", "linear") for w, h in ((132, 68), (133, 69))]


@pytest.fixture(scope="module")
def shims(tmp_path_factory, oracle):
    ba, lin = S.Shim(tmp_path_factory.mktemp("malta_fill_ba")), LS.Shim(tmp_path_factory.mktemp("malta_fill_lin"))
    ba.set_device_switches(True)
    lin.set_device_switches(True)
    yield ba, lin
    ba.set_device_switches(False)
    lin.set_device_switches(False)


def device_results(ce, ctx, kind, w, h, refs, tests, pair_ref, with_map):
    """(scores, 3-norms, maps or None) of one launch of a fresh batch holding these pairs."""
    n = len(tests)
    if kind == "deep":
        b = ctx.batch_deep(w, h, len(refs), n, DEPTH, DEPTH)
    elif kind == "linear":
        b = ctx.batch_linear(w, h, len(refs), n)
    else:
        b = ce.Batch(ctx, w, h, len(refs), n)
    try:
        for i, r in enumerate(refs):
            b.set_reference(i, r)
        for p, t in enumerate(tests):
            b.set_test(p, pair_ref[p], t)
        scores = b.run(n, ce.MetricConfig(butteraugli=True), 80.0, butteraugli_diffmap=with_map)
        assert all(s.status == 0 for s in scores)
        p3 = b.butteraugli_pnorm3(n)
        maps = b.butteraugli_diffmaps(0, n) if with_map else None
        return [s.butteraugli for s in scores], [float(v) for v in p3], maps
    finally:
        b.close()


@pytest.mark.parametrize("kind,w,h", CASES, ids=lambda v: str(v))
def test_fill_is_the_oracle_and_a_batch_is_its_pairs(ce, gpu_ctx, workloads, shims, kind, w, h):
    refs, tests = make_images(workloads, kind, w, h, N_PAIRS, 7000 + 3 * w + h)
    pair_ref = [p % N_REFS for p in range(N_PAIRS)]
    want = oracle_results(ce, shims, kind, refs, tests, w, h)
    bits = lambda v: np.float64(v).view(np.uint64)
    for with_map in (True, False):
        scores, p3, maps = device_results(ce, gpu_ctx, kind, w, h, refs, tests, pair_ref, with_map)
        if with_map:
            assert maps.shape == (N_PAIRS, h, w) and maps.dtype == np.float32
        for p in range(N_PAIRS):
            w_score, w_p3, w_map = want[p]
            where = (kind, w, h, with_map, p)
            if with_map:
                bad = np.argwhere(maps[p].view(np.uint32) != w_map.view(np.uint32))
                assert bad.size == 0, (where, len(bad), bad[:4].tolist())
            assert scores[p] == w_score, (where, scores[p], w_score)
            assert abs(p3[p] - w_p3) <= PNORM_REL[kind] * abs(w_p3), (where, p3[p], w_p3)
            # the pair alone, with its own reference only
            s1, q1, m1 = device_results(ce, gpu_ctx, kind, w, h, [refs[pair_ref[p]]], [tests[p]], [0], with_map)
            assert bits(s1[0]) == bits(scores[p]) and bits(q1[0]) == bits(p3[p]), (where, s1[0], scores[p], q1[0], p3[p])
            if with_map:
                assert np.array_equal(m1[0].view(np.uint32), maps[p].view(np.uint32)), where
