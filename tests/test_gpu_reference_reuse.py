"""A batch keeps what its metrics derive from the references alone from one launch to the next (csrc/ce_ref_state.h) and
rebuilds it when, and only when, a reference was written, more references are used than the state covers, or a parameter
the state depends on differs.  Every comparison is exact equality of all scores with a fresh batch that received the same
writes and one launch; every case also asserts Batch.ref_stats(), without which no case could tell reuse from a rebuild.
Shapes, layout and method: tests/reference_reuse_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reference_reuse_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = R.SHAPES


@pytest.mark.parametrize("w,h", SHAPES)
def test_relaunch_with_new_tests_and_a_rebound_pair_reuses_everything(ce, workloads, gpu_ctx, w, h):
    steps = R.case_relaunch(ce, workloads, gpu_ctx, w, h)
    for got, want, stats in steps:
        assert got == want and stats == [1, 1, 1]
    assert steps[0][0] != steps[1][0]  # the second launch did score the new tests


@pytest.mark.parametrize("w,h", SHAPES)
def test_replacing_one_reference_rebuilds_all_metrics(ce, workloads, gpu_ctx, w, h):
    cfg = ce.MetricConfig.all()
    refs, tests = R.images(ce, workloads, "rgb8", w, h, 310)
    ops = R.op_fill(refs, tests)
    b = R.make_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, ops)
        first = R.launch(b, cfg)
        assert b.ref_stats() == (1, 1, 1)
        ops.append(R.op_set_reference(1, workloads.make_reference(w, h, 319)))  # the middle reference
        ops[-1](ce, b)
        got = R.launch(b, cfg)
        assert b.ref_stats() == (2, 2, 2)
        assert got == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg) and got != first
    finally:
        b.close()


def _yuv(ce, rng, w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return ce.YuvImage(planes=(rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (ch, cw), np.uint8),
                               rng.integers(0, 256, (ch, cw), np.uint8)))


def _writer(ce, wl, gpu_ctx, kind, name, w, h, keep):
    """-> the operations that write reference 1 (`over`: and 2; `resample`: all three) by route `name`; batches they read go to `keep`"""
    rng = np.random.default_rng(w * 100 + h)
    new8 = wl.make_reference(w, h, 329)
    new = R.convert(ce, kind, new8)
    if name == "set_reference":
        return [R.op_set_reference(1, new)]
    if name == "fmt":
        rgba = np.concatenate([new8.reshape(h, w, 3), np.full((h, w, 1), 255, np.uint8)], axis=2)
        return [lambda ce_, b: b.set_reference_fmt(1, rgba, ce.PIXEL_RGBA8)]
    if name == "lut":
        return [lambda ce_, b: b.set_reference_lut(1, new8, ce.PIXEL_RGB8, None)]
    if name == "over":
        rgba = np.concatenate([new8.reshape(h, w, 3), rng.integers(0, 256, (h, w, 1), np.uint8)], axis=2)
        return [lambda ce_, b: b.set_reference_over(1, rgba, ce.PIXEL_RGBA8, [(255, 255, 255), (20, 40, 60)])]
    if name == "yuv":
        img = _yuv(ce, rng, w, h)
        return [lambda ce_, b: b.set_reference_yuv(1, img)]
    if name == "resample":  # the three references of a larger batch of this context, resampled into this one
        src = ce.Batch(gpu_ctx, w + 9, h + 5, R.MAX_REFS, 1)
        keep.append(src)
        for i in range(R.N_REFS):
            src.set_reference(i, wl.make_reference(w + 9, h + 5, 340 + i))
        return [lambda ce_, b: src.resample_into(b, 0, R.N_REFS)]
    if name == "slab":
        return [R.op_slab_write(1, new)]
    if name == "cicp":
        return [lambda ce_, b: b.set_reference_cicp(1, new8.reshape(h, w, 3), ce.ColourDescription.SRGB)]
    if name == "hlg":
        codes = rng.integers(0, 1024, (h, w, 3), np.uint16)
        return [lambda ce_, b: b.set_reference_hlg(1, codes, ce.HlgDescription.BT2100_HLG)]
    if name == "yuv_cicp":
        img = _yuv(ce, rng, w, h)
        return [lambda ce_, b: b.set_reference_yuv_cicp(1, img, ce.ColourDescription.SRGB)]
    if name == "yuv_hlg":
        img = _yuv(ce, rng, w, h)
        return [lambda ce_, b: b.set_reference_yuv_hlg(1, img, ce.HlgDescription.BT2100_HLG)]
    raise AssertionError(name)


WRITERS = ([("rgb8", n) for n in ("fmt", "lut", "yuv", "over", "resample", "slab", "references_changed")] + [("deep", "set_reference")] +
           [("linear", n) for n in ("set_reference", "cicp", "hlg", "yuv_cicp", "yuv_hlg")])


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind,name", WRITERS)
def test_every_reference_writer_invalidates(ce, workloads, gpu_ctx, kind, name, w, h):
    cfg = ce.MetricConfig.all()
    refs, tests = R.images(ce, workloads, kind, w, h, 320)
    ops = R.op_fill(refs, tests)
    keep = []
    b = R.make_batch(ce, gpu_ctx, kind, w, h)
    try:
        R.run_ops(ce, b, ops)
        kept = b.reference_slab  # before the first launch: a caller that holds on to the pointer
        first = R.launch(b, cfg)
        assert b.ref_stats() == (1, 1, 1)
        if name == "references_changed":
            new = R.convert(ce, kind, workloads.make_reference(w, h, 329))
            R.write_device(ce, kept + new.nbytes, new)  # through the kept pointer: the library cannot see this write ...
            b.references_changed()                      # ... so the caller says so
            write = [R.op_slab_write(1, new)]
        else:
            write = _writer(ce, workloads, gpu_ctx, kind, name, w, h, keep)
            R.run_ops(ce, b, write)
        got = R.launch(b, cfg)
        assert b.ref_stats() == (2, 2, 2)
        assert got == R.fresh(ce, gpu_ctx, kind, w, h, ops + write, cfg) and got != first
    finally:
        b.close()
        for s in keep:
            s.close()


@pytest.mark.parametrize("w,h", SHAPES)
def test_parameters_rebuild_what_depends_on_them(ce, workloads, gpu_ctx, w, h):
    cfg = ce.MetricConfig.all()
    refs, tests = R.images(ce, workloads, "rgb8", w, h, 330)
    ops = R.op_fill(refs, tests)
    b = R.make_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, ops)
        base = R.launch(b, cfg)
        assert b.ref_stats() == (1, 1, 1)
        # another intensity target: Butteraugli alone, and again on the way back (one record, one target)
        bright = R.launch(b, cfg, intensity=250.0)
        assert b.ref_stats() == (1, 1, 2)
        assert bright == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg, intensity=250.0) and bright != base
        assert R.launch(b, cfg) == base and b.ref_stats() == (1, 1, 3)
        # the XYB roundtrip switches the slab the metrics read: on and off rebuild all three
        rt = R.launch(b, cfg.with_xyb_roundtrip())
        assert b.ref_stats() == (2, 2, 4)
        assert rt == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg.with_xyb_roundtrip()) and rt != base
        assert R.launch(b, cfg.with_xyb_roundtrip()) == rt and b.ref_stats() == (2, 2, 4)
        assert R.launch(b, cfg) == base and b.ref_stats() == (3, 3, 5)
        assert base == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg)
    finally:
        b.close()


@pytest.mark.parametrize("w,h", SHAPES)
def test_a_metric_builds_on_its_first_run_and_a_scale_limit_rebuilds_ssimulacra2(ce, workloads, gpu_ctx, w, h):
    cfg, only = ce.MetricConfig.all(), ce.MetricConfig.ssimulacra2_only()
    refs, tests = R.images(ce, workloads, "rgb8", w, h, 340)
    ops = R.op_fill(refs, tests)
    b = R.make_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, ops)
        alone = R.launch(b, only)
        assert b.ref_stats() == (1, 0, 0)
        assert alone == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, only)
        assert R.launch(b, cfg) == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg) and b.ref_stats() == (1, 1, 1)
        assert R.launch(b, only) == alone and b.ref_stats() == (1, 1, 1)
        b.debug_limit_scales(1)  # a pyramid of another depth is another state
        R.launch(b, only)
        assert b.ref_stats() == (2, 1, 1)
        b.debug_limit_scales(6)
        assert R.launch(b, only) == alone and b.ref_stats() == (3, 1, 1)
    finally:
        b.close()


@pytest.mark.parametrize("w,h", SHAPES)
def test_more_references_than_covered_rebuild_and_fewer_reuse(ce, workloads, gpu_ctx, w, h):
    cfg = ce.MetricConfig.all()
    refs, tests = R.images(ce, workloads, "rgb8", w, h, 350)
    ops = R.op_fill(refs, tests)
    b = R.make_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, ops)
        two = R.launch(b, cfg, n_pairs=2)  # pairs 0 and 1: references 1 and 0
        assert b.ref_stats() == (1, 1, 1)
        assert two == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg, n_pairs=2)
        six = R.launch(b, cfg)  # reference 2 as well: past what the state covers
        assert b.ref_stats() == (2, 2, 2)
        assert six == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg) and six[:2] == two
        assert R.launch(b, cfg, n_pairs=2) == two and b.ref_stats() == (2, 2, 2)
    finally:
        b.close()


def _read_maps(ce, w, h):
    def read(b):
        out = [b.butteraugli_diffmaps(0, R.N_PAIRS)]
        for level in range(len(ce.dssim_levels(w, h))):
            maps, ssim = b.dssim_ssim_maps(level, 0, R.N_PAIRS)
            out += [maps, ssim]
        for scale in range(len(ce.ssimulacra2_scales(w, h))):
            for channel in range(3):
                for kind in range(3):
                    maps, norms = b.ssimulacra2_maps(scale, channel, kind, 0, R.N_PAIRS)
                    out += [maps, norms]
        return [np.ascontiguousarray(a).view(np.uint8).copy() for a in out]
    return read


@pytest.mark.parametrize("w,h", SHAPES)
def test_maps_of_a_reused_launch_equal_a_fresh_batch(ce, workloads, gpu_ctx, w, h):
    cfg = ce.MetricConfig.all()
    refs, tests = R.images(ce, workloads, "rgb8", w, h, 360)
    ops = R.op_fill(refs, tests)
    read = _read_maps(ce, w, h)
    b = R.make_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, ops)
        R.launch(b, cfg)
        got = R.launch(b, cfg, butteraugli_diffmap=True, ssimulacra2_maps=True)
        assert b.ref_stats() == (1, 1, 1)
        maps = read(b)
        want, want_maps = R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg, read=read, butteraugli_diffmap=True, ssimulacra2_maps=True)
        assert got == want
        assert len(maps) == len(want_maps) > 20 and all(np.array_equal(a, c) for a, c in zip(maps, want_maps))
    finally:
        b.close()


@pytest.mark.parametrize("w,h", SHAPES)
def test_a_reference_written_between_launch_and_collect(ce, workloads, gpu_ctx, w, h):
    """The first launch scores the old reference, the second the new one: the upload waits for the launch that still reads
    the slab, and the state that now outlives a launch is dropped by the write, not by the collect."""
    cfg = ce.MetricConfig.all()
    refs, tests = R.images(ce, workloads, "rgb8", w, h, 370)
    ops = R.op_fill(refs, tests)
    other = R.op_set_reference(1, workloads.make_reference(w, h, 379))
    b = R.make_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, ops)
        b.launch(R.N_PAIRS, cfg)
        other(ce, b)
        old = R.bits(b.collect(R.N_PAIRS))
        new = R.launch(b, cfg)
        assert b.ref_stats() == (2, 2, 2)
        assert old == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops, cfg)
        assert new == R.fresh(ce, gpu_ctx, "rgb8", w, h, ops + [other], cfg) and new != old
    finally:
        b.close()


KNOB_SCRIPT = r"""
import importlib, json, sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import reference_reuse_cases as R
ce = importlib.import_module("codec-eval_amd")
wl = importlib.import_module("codec-eval_amd.workloads")
ctx = ce.Context(0)
print(json.dumps([R.case_relaunch(ce, wl, ctx, w, h) for (w, h) in R.SHAPES]))
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_the_knob_rebuilds_on_every_launch_and_changes_no_score(ce, workloads, gpu_ctx):
    """CE_KEEP_REFERENCE_STATE=0 (read once per process, so in a child): the counters grow by one per launch, the scores of
    the relaunch case are those of this process."""
    env = dict(os.environ)
    env["CE_KEEP_REFERENCE_STATE"] = "0"
    r = subprocess.run([sys.executable, "-c", KNOB_SCRIPT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    for (w, h), steps in zip(SHAPES, child):
        here = R.case_relaunch(ce, workloads, gpu_ctx, w, h)
        assert [s[2] for s in steps] == [[1, 1, 1], [2, 2, 2]] and [s[2] for s in here] == [[1, 1, 1], [1, 1, 1]]
        for (got, want, _), (mine, _, _) in zip(steps, here):
            assert [tuple(x) for x in got] == [tuple(x) for x in want] == mine


def test_pooled_batches_score_each_call_against_its_own_references(ce, workloads):
    """Two ce_eval_batch calls on one context, same shapes, other references: the pooled batches are reused and invalidate
    on upload, so each call equals its one-pair calls."""
    cfg = ce.MetricConfig.all()
    with ce.Context(0) as ctx:
        for seed in (380, 390):
            items = []
            for (w, h) in SHAPES:
                refs = [workloads.make_reference(w, h, seed + r) for r in range(R.N_REFS)]
                items += [(refs[R.BIND[k]], workloads.distort(refs[R.BIND[k]], 35 + 11 * k), w, h) for k in range(R.N_PAIRS)]
            got = [ce.MetricResult.from_c(s) for s in ctx.eval_batch(items, cfg)]
            assert all(m.dssim is not None and m.ssimulacra2 is not None and m.butteraugli is not None and m.psnr is not None for m in got)
            assert got == [ctx.calculate_metrics(r, t, w, h, cfg) for r, t, w, h in items]


@pytest.mark.parametrize("w,h", SHAPES)
def test_the_walk_length_hook_rebuilds_dssim(ce, workloads, gpu_ctx, w, h):
    cfg = ce.MetricConfig.all()
    refs, tests = R.images(ce, workloads, "rgb8", w, h, 400)
    ops = R.op_fill(refs, tests)
    b = R.make_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, ops)
        base = R.launch(b, cfg)
        b.debug_dssim_walk_rows(4)
        assert R.launch(b, cfg) == base and b.ref_stats() == (1, 2, 1)  # the walk length schedules, it does not change a value
        b.debug_dssim_walk_rows(0)
        assert R.launch(b, cfg) == base and b.ref_stats() == (1, 3, 1)
    finally:
        b.close()
