"""What tests/test_gpu_ba_lf_term.py and its CE_BA_LF_TERM=0 child process share: the batches, the launches each one is taken
through and what is read after every launch.  A launch that finds its references' state kept forms the LF term of
CombineChannelsToDiffmap in the LF column blur (butteraugli.hip: EPI_LF_TERM; ce_plan.h: ce_plan_ba_lf_term_in_blur), every
other launch in Malta's epilogue, so a batch is launched twice (old path, new path), one reference is then written again
(state dropped: old path) and it is launched twice more.  Everything returned is compared with == on bit patterns."""
import numpy as np

# 64 x 32 tiles in both kernels: a tile and one either side of it, two tiles by two with an odd half-resolution level
# (130 x 70 -> 65 x 35), and the smallest image Butteraugli scores (8 x 8, one resolution level; below it a batch returns
# CE_ERR_TOO_SMALL and runs none of the metric's kernels, as the oracle refuses it: a one-pixel image can only be refused)
SHAPES = [(8, 8), (63, 31), (64, 32), (65, 33), (130, 70)]
N_REFS = 3
BIND = [2, 1, 2, 0, 2, 1, 2]  # pair -> reference: 1, 2 and 4 pairs, no reference's pairs contiguous, reference 0 not first
# 64 distorted slots (the second launch is in slot order, ba_slot_order.h): the seven pairs over and over, scrambled
MANY = [(5 * p + p // 7) % 7 for p in range(64)]
MANY_SHAPE = (65, 33)
OTHER = [("deep", 65, 33), ("linear", 65, 33)]  # depth 10, as tests/test_gpu_ba_slot_order.py makes them
HANDLE_SHAPE = (65, 33)
DEPTH = 10
SEED = 9100


def key(kind, w, h, n):
    return "%s-%dx%d-%d" % (kind, w, h, n)


def images(wl, kind, w, h):
    """-> (3 references, 7 distorted images, every one different; pair p belongs to reference BIND[p])."""
    seed = SEED + 3 * w + h
    rng = np.random.default_rng(seed)
    if kind == "rgb8":
        refs = [np.asarray(wl.make_reference(w, h, seed + i), np.uint8).reshape(h, w, 3) for i in range(N_REFS)]
        tests = []
        for p, r in enumerate(BIND):
            t = np.asarray(wl.distort(refs[r], 25 + (p * 13) % 70, p % 3 == 0), np.uint8).reshape(h, w, 3)
            tests.append(np.clip(t.astype(np.int16) + rng.integers(-1 - p % 4, 2 + p % 4, t.shape), 0, 255).astype(np.uint8))
        return refs, tests
    base = [np.clip(np.asarray(wl.make_reference(w, h, seed + i), np.float64).reshape(h, w, 3) / 255.0 + rng.normal(0.0, 0.01, (h, w, 3)),
                    0.0, 1.0) for i in range(N_REFS)]
    noisy = [np.clip(base[r] + rng.normal(0.0, 0.004 * (1 + p % 7), (h, w, 3)), 0.0, 1.0) for p, r in enumerate(BIND)]
    if kind == "deep":
        q = lambda a: np.round(a * ((1 << DEPTH) - 1)).astype(np.uint16)
        return [q(a) for a in base], [q(a) for a in noisy]
    lin = lambda a: (a ** 2.2 * 4.0).astype(np.float32)  # linear light, up to four times diffuse white
    return [lin(a) for a in base], [lin(a) for a in noisy]


def new_batch(ce, ctx, kind, w, h, n_pairs):
    if kind == "deep":
        return ctx.batch_deep(w, h, N_REFS, n_pairs, DEPTH, DEPTH)
    if kind == "linear":
        return ctx.batch_linear(w, h, N_REFS, n_pairs)
    return ce.Batch(ctx, w, h, N_REFS, n_pairs)


def read(ce, b, n):
    """One launch with the diffmap flag -> (score bits [n], 3-norm bits [n], the maps [n, h, w])."""
    scores = b.run(n, ce.MetricConfig(butteraugli=True), 80.0, butteraugli_diffmap=True)
    assert all(s.status == 0 for s in scores)
    return (np.array([s.butteraugli for s in scores], np.float64).view(np.uint64),
            np.asarray(b.butteraugli_pnorm3(n), np.float64).view(np.uint64), np.ascontiguousarray(b.butteraugli_diffmaps(0, n)))


def launches(ce, ctx, kind, w, h, refs, tests, pick=None):
    """A fresh batch of the pairs `pick` (default: the seven), launched twice, reference 1 written again, launched twice more.
    -> the four launches' read()s and the launches that had rebuilt the references' state after each."""
    pick = list(range(len(BIND))) if pick is None else pick
    n = len(pick)
    b = new_batch(ce, ctx, kind, w, h, n)
    try:
        for i, r in enumerate(refs):
            b.set_reference(i, r)
        for p, u in enumerate(pick):
            b.set_test(p, BIND[u], tests[u])
        out, builds = [], []
        for launch in range(4):
            if launch == 2:
                b.set_reference(1, refs[1])
            out.append(read(ce, b, n))
            builds.append(b.ref_stats()[2])
        return out, builds
    finally:
        b.close()


def handle(ce, wl, ctx):
    """A reference handle's compare called twice per distorted image (the first compare builds the reference's state)."""
    w, h = HANDLE_SHAPE
    refs, tests = images(wl, "rgb8", w, h)
    hd = ce.ReferenceHandle(ctx, refs[2], w, h, butteraugli_diffmap=True)
    try:
        scores, maps = [], []
        for t in (tests[0], tests[0], tests[2]):
            scores.append(hd.compare(t, ce.MetricConfig(butteraugli=True)).butteraugli)
            maps.append(np.ascontiguousarray(hd.butteraugli_diffmaps(0, 1)))
        return np.array(scores, np.float64).view(np.uint64), np.concatenate(maps)
    finally:
        hd.close()


def everything(ce, wl, ctx):
    """Every batch of the file -> {name: array}; the child's whole job, and the parent's other half of each comparison."""
    out = {}

    def put(k, res):
        for launch, (s, p3, maps) in enumerate(res[0]):
            out["%s-L%d-score" % (k, launch)], out["%s-L%d-p3" % (k, launch)], out["%s-L%d-map" % (k, launch)] = s, p3, maps
        out[k + "-builds"] = np.array(res[1])

    for w, h in SHAPES:
        refs, tests = images(wl, "rgb8", w, h)
        put(key("rgb8", w, h, len(BIND)), launches(ce, ctx, "rgb8", w, h, refs, tests))
    w, h = MANY_SHAPE
    refs, tests = images(wl, "rgb8", w, h)
    put(key("rgb8", w, h, len(MANY)), launches(ce, ctx, "rgb8", w, h, refs, tests, MANY))
    for kind, w, h in OTHER:
        refs, tests = images(wl, kind, w, h)
        put(key(kind, w, h, len(BIND)), launches(ce, ctx, kind, w, h, refs, tests))
    out["handle-score"], out["handle-map"] = handle(ce, wl, ctx)
    return out
