"""What tests/test_gpu_ssim2_ref_blur.py and its CE_SSIM2_REF_BLUR=0 child process share: the batches - three references in
four slots, six pairs bound as reference_reuse_cases.BIND, so a launch has more pairs than references - and what is read
from them.  A batch takes the split path (ssim2.hip: the references' mu1 / s11 as final planes) from the second launch on
the same references on (ce_plan.h: ce_plan_ssim2_ref_blur), so every step of a scenario is launched three times, launch3:
unsplit passes, build + split, split on the kept planes.  Everything returned is compared with ==: scores as bit patterns
(reference_reuse_cases.bits), maps and norms as bytes."""
import numpy as np

import reference_reuse_cases as R

# 8 x 8: one scale, fewer rows than two DMA groups.  130 x 67: crosses the 64-column strip and the 32-row block edges, h no
# multiple of 4.  260 x 258: six scales.
SHAPES = [(8, 8), (72, 40), (130, 67), (260, 258)]
BATCHES = [("rgb8", w, h) for (w, h) in SHAPES] + [("deep", 130, 67), ("linear", 130, 67)]
SEED = 500


def key(kind, w, h):
    return "%s-%dx%d" % (kind, w, h)


def launch3(b, cfg, n_pairs=R.N_PAIRS, **kw):
    """Three launches of the same pairs - the first on rebuilt references runs the unsplit passes, the second builds the planes
    and takes the split path, the third finds them - must agree bit for bit; -> their scores."""
    got = [R.launch(b, cfg, n_pairs, **kw) for _ in range(3)]
    assert got[0] == got[1] == got[2], got
    return got[0]


def batch_scores(ce, wl, ctx, kind, w, h):
    """All metrics of the six pairs of a new batch, launched three times."""
    refs, tests = R.images(ce, wl, kind, w, h, SEED)
    b = R.make_batch(ce, ctx, kind, w, h)
    try:
        R.run_ops(ce, b, R.op_fill(refs, tests))
        return launch3(b, ce.MetricConfig.all())
    finally:
        b.close()


def batch_maps(ce, wl, ctx, w, h):
    """-> (scores, [every (scale, channel, kind) map of the six pairs and its norms]) of an RGB8 batch's third launch with
    ssimulacra2_maps."""
    refs, tests = R.images(ce, wl, "rgb8", w, h, SEED + 7)

    def read(b):
        out = []
        for scale in range(len(ce.ssimulacra2_scales(w, h))):
            for channel in range(3):
                for kind in range(3):
                    maps, norms = b.ssimulacra2_maps(scale, channel, kind, 0, R.N_PAIRS)
                    out += [np.ascontiguousarray(maps), np.ascontiguousarray(norms)]
        return out

    b = R.make_batch(ce, ctx, "rgb8", w, h)
    try:
        R.run_ops(ce, b, R.op_fill(refs, tests))
        return launch3(b, ce.MetricConfig.ssimulacra2_only(), ssimulacra2_maps=True), read(b)
    finally:
        b.close()


def child(ce, wl, ctx, npz_path):
    """The child's whole job: scores of every batch as JSON-able lists, every map into one .npz."""
    scores, arrays = {}, {}
    for kind, w, h in BATCHES:
        scores[key(kind, w, h)] = batch_scores(ce, wl, ctx, kind, w, h)
    for w, h in SHAPES:
        s, maps = batch_maps(ce, wl, ctx, w, h)
        scores["maps-" + key("rgb8", w, h)] = s
        for i, a in enumerate(maps):
            arrays["%s-%04d" % (key("rgb8", w, h), i)] = a
    np.savez(npz_path, **arrays)
    return scores
