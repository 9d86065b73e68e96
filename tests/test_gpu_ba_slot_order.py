"""Butteraugli's per-slot kernels under both launch orders (codec-eval_amd/csrc/ba_slot_order.h): a launch with fewer than
ba_slot_order_min slots keeps a slot's tiles spread over the XCDs (tile order), a larger one keeps them on one (slot order)
unless the padding of its last group of 8 slots exceeds a sixteenth of them (at 64: 64 and 68 .. 72 slots, not 65 .. 67, 73).
Both must give the oracle's diffmap and score bit for bit with the two device switches on (tests/test_gpu_butteraugli.py).

Per shape one pool of pairs (2 references, unique distorted images) is scored by the oracle once; a case then runs the first n
pairs of the pool for n_pairs values that put the slot count of a launch at the crossover, one either side of it, and at
multiples of 8 +- 1 on both sides of it - for the first launch of a batch (z0 = 0: references + pairs) and for a second
launch of the same batch (the references' state is kept: z0 = the references, the distorted images' slots only).  The two large
shapes run small (512 x 512: 2 references x 4 tests; 768 x 512: 2 x 1) and once more with the same pairs repeated
until the launch is past the crossover: 8 and 12 column tiles are the two ways neighbouring tiles used to meet the XCDs."""
import os
import re

import numpy as np
import pytest

import ba_diffmap_shim as S
import linear_input_shim as LS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "codec-eval_amd", "csrc", "ba_slot_order.h")
M = int(re.search(r"ba_slot_order_min\s*=\s*(\d+)\s*;", open(HEADER).read()).group(1))  # the crossover, in slots per launch
N_REFS = 2
# first launch: n + 2 slots, second launch: n slots.  Both hit M - 1, M, M + 1 and, past the crossover, 71 .. 73 (72 = 9 x 8 at
# M = 64); under it 7, 8, 9 and 15, 16, 17
N_PAIRS = sorted({5, 6, 7, 8, 9, 13, 14, 15, 16, 17} | set(range(M - 3, M + 2)) | set(range(M + 5, M + 10)))
POOL = max(N_PAIRS)
# the 3-norm: the device adds the oracle's f64 terms tile by tile (1e-13, tests/test_gpu_butteraugli.py); an RGB8 pool's
# 3-norm is numpy's sum over the oracle's map (1e-12, tests/test_gpu_butteraugli_diffmap.py)
PNORM_REL = {"rgb8": 1e-12, "deep": 1e-13, "linear": 1e-13}
SMALL = [("rgb8", 63, 33), ("rgb8", 64, 64), ("rgb8", 65, 31), ("rgb8", 129, 70), ("deep", 65, 31), ("deep", 129, 70),
         ("linear", 63, 33), ("linear", 64, 64)]
DEPTH = 10


@pytest.fixture(scope="module")
def shims(tmp_path_factory, oracle):
    ba, lin = S.Shim(tmp_path_factory.mktemp("slot_order_ba")), LS.Shim(tmp_path_factory.mktemp("slot_order_lin"))
    ba.set_device_switches(True)
    lin.set_device_switches(True)
    yield ba, lin
    ba.set_device_switches(False)
    lin.set_device_switches(False)


def make_images(workloads, kind, w, h, n_tests, seed):
    """2 references and n_tests distorted images, every one different; pair p belongs to reference p % 2."""
    rng = np.random.default_rng(seed)
    if kind == "rgb8":
        refs = [workloads.make_reference(w, h, seed + i) for i in range(N_REFS)]
        tests = []
        for p in range(n_tests):
            t = np.asarray(workloads.distort(refs[p % N_REFS], 25 + (p * 13) % 70, p % 3 == 0), np.uint8).reshape(h, w, 3)
            tests.append(np.clip(t.astype(np.int16) + rng.integers(-1 - p % 4, 2 + p % 4, t.shape), 0, 255).astype(np.uint8))
        return refs, tests
    base = [np.clip(workloads.make_reference(w, h, seed + i).astype(np.float64) / 255.0 + rng.normal(0.0, 0.01, (h, w, 3)), 0.0, 1.0)
            for i in range(N_REFS)]
    noisy = [np.clip(base[p % N_REFS] + rng.normal(0.0, 0.004 * (1 + p % 7), (h, w, 3)), 0.0, 1.0) for p in range(n_tests)]
    if kind == "deep":
        q = lambda a: np.round(a * ((1 << DEPTH) - 1)).astype(np.uint16)
        return [q(a) for a in base], [q(a) for a in noisy]
    lin = lambda a: (a ** 2.2 * 4.0).astype(np.float32)  # linear light, up to four times diffuse white
    return [lin(a) for a in base], [lin(a) for a in noisy]


def oracle_results(ce, shims, kind, refs, tests, w, h):
    """(score, 3-norm, diffmap) per pair with the device switches on."""
    ba, lin = shims
    out = []
    table = ce.srgb_table(DEPTH, 0) if kind == "deep" else None
    for p, t in enumerate(tests):
        r = refs[p % N_REFS]
        if kind == "rgb8":  # one oracle run per pair: the score is the map's maximum, the 3-norm the map's (numpy's summation
            dm = ba.diffmap(r, t, w, h)  # order: 1e-12, tests/test_gpu_butteraugli_diffmap.py)
            out.append((float(dm.max()), S.pnorm3(dm), dm))
        elif kind == "deep":  # a deep batch is the oracle's stages on table(depth, rule 0)[sample]
            out.append(lin.butteraugli_map(table[r], table[t], w, h))
        else:
            out.append(lin.butteraugli_map(r, t, w, h))
    return out


def new_batch(ce, ctx, kind, w, h, n_pairs):
    if kind == "deep":
        return ctx.batch_deep(w, h, N_REFS, n_pairs, DEPTH, DEPTH)
    if kind == "linear":
        return ctx.batch_linear(w, h, N_REFS, n_pairs)
    return ce.Batch(ctx, w, h, N_REFS, n_pairs)


def run_and_check(ce, ctx, kind, w, h, refs, tests, pair_ref, want, where):
    """A fresh batch of these pairs, launched twice; want[p] is the oracle's result of pair p."""
    n = len(tests)
    b = new_batch(ce, ctx, kind, w, h, n)
    try:
        for i, r in enumerate(refs):
            b.set_reference(i, r)
        for p, t in enumerate(tests):
            b.set_test(p, pair_ref[p], t)
        for launch in (0, 1):  # 0: every slot (z0 = 0); 1: the references' state is kept, the distorted slots only (z0 = 2)
            scores = b.run(n, ce.MetricConfig(butteraugli=True), 80.0, butteraugli_diffmap=True)
            p3 = b.butteraugli_pnorm3(n)
            maps = b.butteraugli_diffmaps(0, n)
            assert maps.shape == (n, h, w) and maps.dtype == np.float32
            for p in range(n):
                w_score, w_p3, w_map = want[p]
                bad = np.argwhere(maps[p].view(np.uint32) != w_map.view(np.uint32))
                assert bad.size == 0, (where, n, launch, p, len(bad), bad[:4].tolist())
                assert scores[p].status == 0 and scores[p].butteraugli == w_score, (where, n, launch, p, scores[p].butteraugli, w_score)
                assert abs(float(p3[p]) - w_p3) <= PNORM_REL[kind] * abs(w_p3), (where, n, launch, p, float(p3[p]), w_p3)
    finally:
        b.close()


def test_crossover_is_covered():
    """The slot counts the cases reach, whatever value the header holds."""
    first, second = {n + N_REFS for n in N_PAIRS}, set(N_PAIRS)
    for launches in (first, second):
        assert {M - 1, M, M + 1} <= launches
        assert any(s % 8 == 0 and s > M and {s - 1, s + 1} <= launches for s in launches)  # slot order, padded either side
        assert any(s % 8 == 0 and s < M and {s - 1, s + 1} <= launches for s in launches)  # tile order


@pytest.mark.parametrize("kind,w,h", SMALL, ids=lambda v: str(v))
def test_small_shapes_both_orders_are_the_oracle(ce, gpu_ctx, workloads, shims, kind, w, h):
    refs, tests = make_images(workloads, kind, w, h, POOL, 4000 + w)
    want = oracle_results(ce, shims, kind, refs, tests, w, h)
    for n in N_PAIRS:
        run_and_check(ce, gpu_ctx, kind, w, h, refs, tests[:n], [p % N_REFS for p in range(n)], want, (kind, w, h))


@pytest.mark.parametrize("w,h,per_ref", [(512, 512, 4), (768, 512, 1)], ids=["512x512", "768x512"])
def test_large_shapes_both_orders_are_the_oracle(ce, gpu_ctx, workloads, shims, w, h, per_ref):
    """As stated (10 and 4 slots: tile order), then the same pairs repeated in a scrambled order until both launches are in slot
    order (M + 8 slots, then M + 6 distorted slots: a padded group)."""
    n_unique = N_REFS * per_ref
    refs, tests = make_images(workloads, "rgb8", w, h, n_unique, 5000 + w)
    want = oracle_results(ce, shims, "rgb8", refs, tests, w, h)
    run_and_check(ce, gpu_ctx, "rgb8", w, h, refs, tests, [p % N_REFS for p in range(n_unique)], want, (w, h, "as stated"))
    pick = [(5 * p + p // n_unique) % n_unique for p in range(M + 6)]
    run_and_check(ce, gpu_ctx, "rgb8", w, h, refs, [tests[u] for u in pick], [u % N_REFS for u in pick], [want[u] for u in pick],
                  (w, h, "repeated"))
