"""SSIMULACRA2's split path (ssim2.hip, ce_plan.h: ce_plan_ssim2_ref_blur): a launch with more pairs than references that finds
its references kept from an earlier launch keeps every reference's mu1 = blur(a) and s11 = blur(a*a) as final planes of the
batch (record CE_REF_SSIM2_BLUR) and the pair passes filter only the three streams that involve the distorted image.  Every
step of a scenario is therefore launched three times (ssim2_ref_blur_cases.launch3: unsplit, build + split, split) and the
three must agree.  The planes are the floats the unsplit passes compute, so
every comparison here is == on bit patterns: against one-pair calls (which keep the unsplit passes by the rule), against
the same batch in a child process with CE_SSIM2_REF_BLUR=0, and against fresh batches after everything that can leave the
planes stale - rebinding, references without pairs in the building launch, a launch over a prefix of the pairs, rewritten
references, the XYB roundtrip's other slab, a reference handle.  Batches and shapes: tests/ssim2_ref_blur_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reference_reuse_cases as R  # noqa: E402
import ssim2_ref_blur_cases as S  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD_SCRIPT = r"""
import importlib, json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import ssim2_ref_blur_cases as S
ce = importlib.import_module("codec-eval_amd")
wl = importlib.import_module("codec-eval_amd.workloads")
ctx = ce.Context(0)
print(json.dumps(S.child(ce, wl, ctx, sys.argv[1])))
""" % (ROOT, os.path.join(ROOT, "tests"))


@pytest.fixture(scope="module")
def knob0(tmp_path_factory):
    """Every batch of the cases in a child with CE_SSIM2_REF_BLUR=0 (read once per process): (scores, maps)."""
    npz = str(tmp_path_factory.mktemp("ssim2_ref_blur") / "maps.npz")
    env = dict(os.environ)
    env["CE_SSIM2_REF_BLUR"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD_SCRIPT, npz], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    scores = {k: [tuple(x) for x in v] for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}
    return scores, np.load(npz)


@pytest.fixture(scope="module")
def split_scores(ce, workloads, gpu_ctx):
    """The batches' scores in this process, computed once: six pairs on three references, three launches."""
    return {S.key(*b): S.batch_scores(ce, workloads, gpu_ctx, *b) for b in S.BATCHES}


def _f64_bits(v):
    return int(np.float64(v).view(np.uint64))


def _result_bits(m):
    return tuple(_f64_bits(v) for v in (m.dssim, m.ssimulacra2, m.butteraugli, m.psnr))


@pytest.mark.parametrize("kind,w,h", S.BATCHES)
def test_the_batch_equals_its_one_pair_calls(ce, workloads, gpu_ctx, split_scores, kind, w, h):
    got = split_scores[S.key(kind, w, h)]
    refs, tests = R.images(ce, workloads, kind, w, h, S.SEED)
    cfg = ce.MetricConfig.all()
    for k in range(R.N_PAIRS):
        if kind == "rgb8":
            m = gpu_ctx.calculate_metrics(refs[R.BIND[k]], tests[k], w, h, cfg)
            assert got[k][2:] == _result_bits(m), (k, got[k], m)
        else:  # one pair, one reference: a batch of its own
            b = gpu_ctx.batch_deep(w, h, 1, 1, 16, 16) if kind == "deep" else gpu_ctx.batch_linear(w, h, 1, 1)
            try:
                b.set_reference(0, refs[R.BIND[k]])
                b.set_test(0, 0, tests[k])
                assert R.launch(b, cfg, n_pairs=1) == [got[k]], k
            finally:
                b.close()


@pytest.mark.parametrize("kind,w,h", S.BATCHES)
def test_the_knob_changes_no_score(split_scores, knob0, kind, w, h):
    assert split_scores[S.key(kind, w, h)] == knob0[0][S.key(kind, w, h)]


@pytest.mark.parametrize("kind,w,h", S.BATCHES)
def test_new_tests_and_a_rebound_pair_reuse_the_planes(ce, workloads, gpu_ctx, kind, w, h):
    cfg = ce.MetricConfig.all()
    refs, tests = R.images(ce, workloads, kind, w, h, S.SEED + 10)
    refs8 = [workloads.make_reference(w, h, S.SEED + 10 + r) for r in range(R.N_REFS)]
    tests2 = [R.convert(ce, kind, workloads.distort(refs8[R.REBIND[k]], 28 + 9 * k)) for k in range(R.N_PAIRS)]
    first = R.op_fill(refs, tests)
    second = [R.op_set_test(k, R.REBIND[k], t) for k, t in enumerate(tests2)]
    b = R.make_batch(ce, gpu_ctx, kind, w, h)
    try:
        R.run_ops(ce, b, first)
        one = S.launch3(b, cfg)
        stats = b.ref_stats()
        assert one == R.fresh(ce, gpu_ctx, kind, w, h, first, cfg)
        R.run_ops(ce, b, second)
        two = S.launch3(b, cfg)
        assert b.ref_stats() == stats == (1, 1, 1)
        assert two == R.fresh(ce, gpu_ctx, kind, w, h, first + second, cfg) and two != one
    finally:
        b.close()


@pytest.mark.parametrize("kind,w,h", S.BATCHES)
def test_references_without_pairs_in_the_building_launch(ce, workloads, gpu_ctx, kind, w, h):
    """All six pairs on reference 2: the launch uses three references and builds the planes of all three; then the pairs
    move onto references 0 and 1 as well."""
    cfg = ce.MetricConfig.ssimulacra2_only()
    refs, tests = R.images(ce, workloads, kind, w, h, S.SEED + 20)
    first = [R.op_set_reference(i, r) for i, r in enumerate(refs)] + [R.op_set_test(k, 2, t) for k, t in enumerate(tests)]
    second = [R.op_bind(k, R.BIND[k]) for k in range(R.N_PAIRS)]
    b = R.make_batch(ce, gpu_ctx, kind, w, h)
    try:
        R.run_ops(ce, b, first)
        assert S.launch3(b, cfg) == R.fresh(ce, gpu_ctx, kind, w, h, first, cfg)
        R.run_ops(ce, b, second)
        assert S.launch3(b, cfg) == R.fresh(ce, gpu_ctx, kind, w, h, first + second, cfg)
        assert b.ref_stats() == (1, 0, 0)
    finally:
        b.close()


@pytest.mark.parametrize("kind,w,h", S.BATCHES)
def test_a_prefix_launch_does_not_cover_the_third_reference(ce, workloads, gpu_ctx, kind, w, h):
    """Pairs 0 and 1 use references 1 and 0 (one pair per reference: the unsplit passes, nothing built, however often); three
    pairs on the same two references build planes that cover two references; all six then need reference 2's planes too; the
    prefixes again afterwards are covered and take the split path."""
    cfg = ce.MetricConfig.ssimulacra2_only()
    refs, tests = R.images(ce, workloads, kind, w, h, S.SEED + 30)
    ops = R.op_fill(refs, tests)
    b = R.make_batch(ce, gpu_ctx, kind, w, h)
    try:
        R.run_ops(ce, b, ops)
        two = S.launch3(b, cfg, n_pairs=2)
        assert two == R.fresh(ce, gpu_ctx, kind, w, h, ops, cfg, n_pairs=2)
        three = S.launch3(b, cfg, n_pairs=3)
        assert three == R.fresh(ce, gpu_ctx, kind, w, h, ops, cfg, n_pairs=3) and three[:2] == two
        six = S.launch3(b, cfg)
        assert six == R.fresh(ce, gpu_ctx, kind, w, h, ops, cfg) and six[:3] == three
        assert S.launch3(b, cfg, n_pairs=2) == two and S.launch3(b, cfg, n_pairs=3) == three
    finally:
        b.close()


@pytest.mark.parametrize("kind,w,h", S.BATCHES)
def test_rewritten_references_rebuild_the_planes(ce, workloads, gpu_ctx, kind, w, h):
    cfg = ce.MetricConfig.ssimulacra2_only()
    refs, tests = R.images(ce, workloads, kind, w, h, S.SEED + 40)
    ops = R.op_fill(refs, tests)
    b = R.make_batch(ce, gpu_ctx, kind, w, h)
    try:
        R.run_ops(ce, b, ops)
        base = S.launch3(b, cfg)
        ops.append(R.op_set_reference(1, R.convert(ce, kind, workloads.make_reference(w, h, S.SEED + 48))))
        ops[-1](ce, b)
        set_ = S.launch3(b, cfg)
        assert b.ref_stats() == (2, 0, 0)
        assert set_ == R.fresh(ce, gpu_ctx, kind, w, h, ops, cfg) and set_ != base
        ops.append(R.op_slab_write(0, R.convert(ce, kind, workloads.make_reference(w, h, S.SEED + 49))))
        ops[-1](ce, b)
        slab = S.launch3(b, cfg)
        assert b.ref_stats() == (3, 0, 0)
        assert slab == R.fresh(ce, gpu_ctx, kind, w, h, ops, cfg) and slab != set_
    finally:
        b.close()


@pytest.mark.parametrize("w,h", S.SHAPES)
def test_maps_and_norms_equal_the_knob_off_child(ce, workloads, gpu_ctx, knob0, w, h):
    scores, maps = S.batch_maps(ce, workloads, gpu_ctx, w, h)
    assert scores == knob0[0]["maps-" + S.key("rgb8", w, h)]
    assert len(maps) == 2 * 9 * len(ce.ssimulacra2_scales(w, h))
    for i, a in enumerate(maps):
        want = knob0[1]["%s-%04d" % (S.key("rgb8", w, h), i)]
        assert a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes(), i


@pytest.mark.parametrize("w,h", S.SHAPES)
def test_the_xyb_roundtrip_on_off_on(ce, workloads, gpu_ctx, w, h):
    cfg = ce.MetricConfig.ssimulacra2_only()
    refs, tests = R.images(ce, workloads, "rgb8", w, h, S.SEED + 50)
    ops = R.op_fill(refs, tests)
    on = R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg.with_xyb_roundtrip())
    off = R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg)
    b = R.make_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, ops)
        assert S.launch3(b, cfg.with_xyb_roundtrip()) == on
        assert S.launch3(b, cfg) == off
        assert S.launch3(b, cfg.with_xyb_roundtrip()) == on
        assert b.ref_stats() == (3, 0, 0)
    finally:
        b.close()


@pytest.mark.parametrize("w,h", S.SHAPES)
def test_a_reference_handle_sweep(ce, workloads, gpu_ctx, w, h):
    cfg = ce.MetricConfig.all()
    ref = workloads.make_reference(w, h, S.SEED + 60)
    tests = [workloads.distort(ref, q) for q in (30, 55, 80)]
    want = [_result_bits(gpu_ctx.calculate_metrics(ref, t, w, h, cfg)) for t in tests]
    hd = ce.ReferenceHandle(gpu_ctx, ref, w, h)
    try:
        assert [_result_bits(hd.compare(t, cfg)) for t in tests] == want  # one at a time: the first compare builds, the others reuse
        assert [_result_bits(m) for m in hd.compare_many(tests, cfg)] == want  # ... and a grown handle builds again
        assert [_result_bits(hd.compare(t, cfg)) for t in tests[::-1]] == want[::-1]
    finally:
        hd.close()
