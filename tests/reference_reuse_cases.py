"""What tests/test_gpu_reference_reuse.py and the child process of its knob case share: small grids with three references
in a batch of four slots and six pairs bound unevenly and interleaved, the ways a reference can be written, and the method -
a batch is taken through writes and launches, and every launch is compared, bit for bit, with a FRESH batch that received
the same writes in the same order and one launch.  A score comparison cannot tell a reused plane from a rebuilt one, so
every step also reports Batch.ref_stats()."""
import ctypes as C

import numpy as np

# 72 x 40: one Malta tile plus halo, two DSSIM strips.  130 x 67: odd, crosses the 64-column strip and the 32-row tile
# edges, three SSIMULACRA2 scales.  The smallest sizes at which slot indexing behind skipped reference slots can go wrong.
SHAPES = [(72, 40), (130, 67)]
MAX_REFS, N_REFS, N_PAIRS = 4, 3, 6
BIND = [1, 0, 0, 2, 0, 2]    # pair -> reference: pair_first is no identity, reference 0 is not the first one used
REBIND = [1, 0, 2, 2, 0, 2]  # ... with pair 2 moved to another reference


def bits(scores):
    """Scores as comparable integers: status, valid, and the bit patterns of the four values."""
    return [(s.status, s.valid) + tuple(int(np.float64(v).view(np.uint64)) for v in (s.dssim, s.ssimulacra2, s.butteraugli, s.psnr))
            for s in scores]


def make_batch(ce, ctx, kind, w, h):
    if kind == "linear":
        return ctx.batch_linear(w, h, MAX_REFS, N_PAIRS)
    if kind == "deep":
        return ctx.batch_deep(w, h, MAX_REFS, N_PAIRS, 16, 16)
    return ce.Batch(ctx, w, h, MAX_REFS, N_PAIRS)


def images(ce, wl, kind, w, h, seed):
    """-> (references [N_REFS], tests [N_PAIRS] bound by BIND) in the batch kind's own sample type."""
    refs8 = [wl.make_reference(w, h, seed + r) for r in range(N_REFS)]
    tests8 = [wl.distort(refs8[BIND[k]], 35 + 11 * k) for k in range(N_PAIRS)]
    return [convert(ce, kind, a) for a in refs8], [convert(ce, kind, a) for a in tests8]


def convert(ce, kind, rgb8):
    a = np.ascontiguousarray(rgb8).reshape(-1, 3)
    if kind == "deep":
        return (a.astype(np.uint32) * 257 + np.arange(a.shape[0], dtype=np.uint32)[:, None] % 5).clip(0, 65535).astype(np.uint16)  # off the 8-bit grid
    if kind == "linear":
        return ce.srgb_table(8, 0)[a].astype(np.float32)
    return a


# ---- operations on a batch: a scenario is a list of them with launches in between, the fresh batch gets them all at once ----

def op_set_reference(i, img):
    return lambda ce, b: b.set_reference(i, img)


def op_set_test(k, r, img):
    return lambda ce, b: b.set_test(k, r, img)


def op_bind(k, r):
    return lambda ce, b: b.bind_pair(k, r)


def op_fill(refs, tests, bind=BIND):
    return [op_set_reference(i, r) for i, r in enumerate(refs)] + [op_set_test(k, bind[k], t) for k, t in enumerate(tests)]


def write_device(ce, address, array):
    """Host bytes -> device memory once the device is idle: the write a caller with pixels in HBM would do itself."""
    a = np.ascontiguousarray(array)
    assert ce.lib().hipDeviceSynchronize() == 0
    assert ce.lib().hipMemcpy(C.c_void_p(address), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0


def op_slab_write(i, img):
    """Reference i through the slab pointer, fetched for this write (the fetch says that references change)."""
    return lambda ce, b: write_device(ce, b.reference_slab + i * np.ascontiguousarray(img).nbytes, img)


def run_ops(ce, b, ops):
    for op in ops:
        op(ce, b)


def launch(b, cfg, n_pairs=N_PAIRS, intensity=None, **kw):
    if intensity is None:
        b.launch(n_pairs, cfg, **kw)
    else:
        b.launch(n_pairs, cfg, intensity, **kw)
    return bits(b.collect(n_pairs))


def fresh(ce, ctx, kind, w, h, ops, cfg, n_pairs=N_PAIRS, intensity=None, read=None, **kw):
    """The scores (read: also read(batch)) of a new batch that gets `ops` and one launch."""
    b = make_batch(ce, ctx, kind, w, h)
    try:
        run_ops(ce, b, ops)
        s = launch(b, cfg, n_pairs, intensity, **kw)
        assert b.ref_stats() == tuple(int(x) for x in (cfg.ssimulacra2, cfg.dssim, cfg.butteraugli))
        return (s, read(b)) if read else s
    finally:
        b.close()


def case_relaunch(ce, wl, ctx, w, h):
    """Case 1 - launch all metrics, replace all six tests and rebind one pair, launch again.
    -> [(scores of the batch, scores of the fresh batch, ref_stats)] per launch."""
    cfg = ce.MetricConfig.all()
    refs, tests = images(ce, wl, "rgb8", w, h, 300)
    tests2 = [wl.distort(wl.make_reference(w, h, 300 + REBIND[k]), 28 + 9 * k).reshape(-1, 3) for k in range(N_PAIRS)]
    first = op_fill(refs, tests)
    second = [op_set_test(k, REBIND[k], t) for k, t in enumerate(tests2)]
    out = []
    b = make_batch(ce, ctx, "rgb8", w, h)
    try:
        run_ops(ce, b, first)
        out.append((launch(b, cfg), fresh(ce, ctx, "rgb8", w, h, first, cfg), list(b.ref_stats())))
        run_ops(ce, b, second)
        out.append((launch(b, cfg), fresh(ce, ctx, "rgb8", w, h, first + second, cfg), list(b.ref_stats())))
    finally:
        b.close()
    return out
