"""Deep batches against the oracle on real deep content (tests/deep_content.py; DESIGN.md section 11, "Parity on real deep
content").

A deep batch of depths (rd, td) is, by definition, the oracle's stages run on table(depth, rule)[min(v, maxv)].  The two
anchors of tests/test_gpu_deep_input.py read 256 entries of a table and content whose two bytes are equal; here one deep batch
per shape and pairing carries every class of deep content as its pairs, several references bound out of order, and
- the slabs, read back, hold the clamped samples exactly for uploads as RGB16, RGBA16 and - on a depth-8 side - RGB8 and
  RGBA8, on slots that are not 16-byte aligned (the edge shapes: k_ingest_deep's sample-by-sample route) and on aligned ones;
- every per-pixel map and score is held to the composed reference with the checks and bounds of
  tests/test_gpu_wide_content.py - Butteraugli's diffmap and score bit for bit with the two device switches on, DSSIM's maps
  bit for bit, SSIMULACRA2's SSIM-error maps bit for bit and its artifact / detail-lost maps within EDGE_REL with the same
  zeros - at 80 nits, and at 250 for one pairing per shape;
- PSNR is the host's expression of the exact integer SSE at equal depths and absent at unequal ones;
- a launch read twice is byte-identical, a replaced distorted image changes its own pair only, and the one-pair call
  returns the batch's scores.
"""
import math

import numpy as np
import pytest

import deep_content as DC
import deep_input_shim as D
import linear_input_shim as LS
import test_gpu_wide_content as WG
from test_gpu_deep_input import hip_runtime
from test_gpu_wide_content import check_butteraugli, check_dssim, check_ssim2, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shims(tmp_path_factory, oracle):
    assert WG.DEVICE_SWITCHES == ("ba_malta_f32", "ba_l2_early")  # what LS.Shim.set_device_switches turns on
    return D.Shim(tmp_path_factory.mktemp("deep_content_deep_shim")), LS.Shim(tmp_path_factory.mktemp("deep_content_linear_shim"))


@pytest.fixture(scope="module")
def content():
    cache = {}

    def get(b):
        if b not in cache:
            cache[b] = DC.cases(*b)
        return cache[b]
    return get


@pytest.fixture(scope="module")
def reference(shims, content):
    """DC.expected per batch, computed once: DSSIM and SSIMULACRA2 do not depend on the intensity target."""
    fixed = {}

    def get(b, intensity):
        ref = DC.expected(shims, content(b), *b, intensity, fixed.get(b))
        fixed[b] = (ref.dssim, ref.ssim2, ref.ssim2_default)
        return ref
    return get


@pytest.fixture(scope="module", autouse=True)
def own_worst():
    """The worst gaps that the shared checks note, for this file alone."""
    kept = dict(WG.worst)
    WG.worst.clear()
    yield
    WG.worst.clear()
    WG.worst.update(kept)


def read_u16(batch, which, n):
    out = np.empty(n, np.uint16)
    batch.ctx.synchronize()
    assert hip_runtime().hipMemcpy(out.ctypes.data, batch.test_slab if which else batch.reference_slab, out.nbytes, 2) == 0  # device to host
    return out


def as_format(ce, a, depth, fmt, rng):
    """The image as uploaded in `fmt`: (pixels, CE_PIXEL_*).  The 8-bit formats hold the clamped samples."""
    alpha_shape = a.shape[:2] + (1,)
    if fmt == "rgb16":
        return a, ce.PIXEL_RGB16
    if fmt == "rgba16":
        return np.concatenate([a, rng.integers(0, 65536, alpha_shape).astype(np.uint16)], axis=-1), ce.PIXEL_RGBA16
    a8 = DC.clamp(a, depth).astype(np.uint8)
    if fmt == "rgb8":
        return a8, ce.PIXEL_RGB8
    return np.concatenate([a8, rng.integers(0, 256, alpha_shape).astype(np.uint8)], axis=-1), ce.PIXEL_RGBA8


def batch_id(b):
    return "%dx%d-%d/%d" % b[:4] + ("" if len(b) == 4 else "@%g" % b[4])


@pytest.mark.parametrize("b", DC.BATCHES, ids=batch_id)
def test_slabs_hold_the_clamped_samples(ce, gpu_ctx, content, b):
    """After a first launch, which orders the uploads, both slabs equal the clamped samples for every format a side takes."""
    w, h, rd, td = b
    cs = content(b)
    refs, tests, pair_ref = DC.grid(cs)
    want_r = np.concatenate([DC.clamp(r, rd).reshape(-1) for r in refs])
    want_t = np.concatenate([DC.clamp(t, td).reshape(-1) for t in tests])
    formats = {depth: ["rgb16", "rgba16"] + (["rgb8", "rgba8"] if depth == 8 else []) for depth in (rd, td)}
    rng = np.random.default_rng(5)
    cfg = ce.MetricConfig(dssim=True, ssimulacra2=False, butteraugli=False, psnr=False)
    batch = gpu_ctx.batch_deep(w, h, len(refs), len(tests), rd, td)
    try:
        for k in range(max(len(f) for f in formats.values())):
            fr, ft = formats[rd][k % len(formats[rd])], formats[td][k % len(formats[td])]
            for i, r in enumerate(refs):
                batch.set_reference_fmt(i, *as_format(ce, r, rd, fr, rng))
            for p, t in enumerate(tests):
                batch.set_test_fmt(p, pair_ref[p], *as_format(ce, t, td, ft, rng))
            batch.run(len(tests), cfg)
            got_r, got_t = read_u16(batch, 0, want_r.size), read_u16(batch, 1, want_t.size)
            for side, got, want in (("references " + fr, got_r, want_r), ("tests " + ft, got_t, want_t)):
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (side, b, "slots", sorted(set((bad // (w * h * 3)).tolist())), "first sample", int(bad[0] % (w * h * 3)),
                                       got[bad[:4]].tolist(), want[bad[:4]].tolist())
            # the slabs are zeroed between formats, so that a setter that wrote nothing cannot pass on the bytes before it
            zero = np.zeros((h, w, 3), np.uint16)
            for i in range(len(refs)):
                batch.set_reference(i, zero)
            for p in range(len(tests)):
                batch.set_test(p, pair_ref[p], zero)
            batch.run(len(tests), cfg)
            assert not read_u16(batch, 0, want_r.size).any() and not read_u16(batch, 1, want_t.size).any()
    finally:
        batch.close()


def fill(batch, refs, tests, pair_ref):
    for i, r in enumerate(refs):
        batch.set_reference(i, r)
    for p, (t, ri) in enumerate(zip(tests, pair_ref)):
        batch.set_test(p, ri, t)


def read_everything(ce, batch, n, w, h, intensity):
    """tests/test_gpu_wide_content.py's read_everything, with PSNR as a sixth entry of every pair's scores."""
    scores = batch.run(n, ce.MetricConfig.all(), intensity, butteraugli_diffmap=True, ssimulacra2_maps=True)
    out = {"scores": [(s.dssim, s.ssimulacra2, s.butteraugli, s.valid, s.status, s.psnr) for s in scores], "pnorm3": batch.butteraugli_pnorm3(n),
           "diffmap": batch.butteraugli_diffmaps(0, n)}
    for lvl in range(len(ce.dssim_levels(w, h))):
        out[f"ds_{lvl}"], out[f"ds_ssim_{lvl}"] = batch.dssim_ssim_maps(lvl, 0, n)
    for s in range(len(ce.ssimulacra2_scales(w, h))):
        for c in range(3):
            for k in range(3):
                out[f"s2_{s}_{c}_{k}"], out[f"s2_norm_{s}_{c}_{k}"] = batch.ssimulacra2_maps(s, c, k, 0, n)
    return out


def pair_of(got, p):
    """Everything a launch returned for pair p, as bytes."""
    return {k: (tuple(np.float64(x).tobytes() for x in v[p]) if k == "scores" else np.asarray(v[p]).tobytes()) for k, v in got.items()}


def check_pair(ce, oracle, shims, name, got, p, ref, q, w, h, rd, td, samples):
    """Pair p of a launch against entry q of a Reference; samples = the pair's (ref, test) as uploaded."""
    n_levels, n_scales = len(ce.dssim_levels(w, h)), len(ce.ssimulacra2_scales(w, h))
    one = DC.Reference([ref.ba[q]], [ref.ba_default[q]], [ref.dssim[q]], [ref.ssim2[q]], [ref.ssim2_default[q]])
    view = {k: {0: v[p]} for k, v in got.items()}  # the shared checks index [p]
    dssim, ssim2, ba, valid, status, psnr = got["scores"][p]
    assert status == 0 and valid == (15 if rd == td else 7), (name, valid, status)  # unequal depths: no PSNR, the rest runs
    check_butteraugli(name, view, 0, one)
    check_dssim(name, view, 0, one.dssim[0], n_levels)
    check_ssim2(name, oracle, view, 0, one.ssim2[0], one.ssim2_default[0], n_scales)
    if rd == td:
        host = D.psnr_from_sse(shims[0].sse(DC.clamp(samples[0], rd), DC.clamp(samples[1], td)), w, h, rd)
        assert psnr == host, (name, psnr, host)
    if name.startswith("identical"):
        assert (dssim, ssim2, ba) == (0.0, 100.0, 0.0), (name, got["scores"][p])
        assert rd != td or psnr == math.inf, (name, psnr)


@pytest.mark.parametrize("run", DC.RUNS, ids=batch_id)
def test_every_map_and_score_equals_the_oracle(ce, gpu_ctx, oracle, shims, content, reference, run):
    w, h, rd, td, intensity = run
    b = run[:4]
    cs = content(b)
    refs, tests, pair_ref = DC.grid(cs)
    n = len(tests)
    ref = reference(b, intensity)
    p_new, new_case = DC.replacement(cs, w, h, rd, td)
    ref_new = DC.expected(shims, [new_case], w, h, rd, td, intensity)
    assert ce.dssim_levels(w, h) == LS.dssim_levels(w, h) and ce.ssimulacra2_scales(w, h) == LS.ssim2_scales(w, h)
    batch = gpu_ctx.batch_deep(w, h, len(refs), n, rd, td)
    try:
        fill(batch, refs, tests, pair_ref)
        got = read_everything(ce, batch, n, w, h, intensity)
        again = read_everything(ce, batch, n, w, h, intensity)
        batch.set_test(p_new, pair_ref[p_new], new_case[2])  # its reference slot, and the state kept for it, stay
        after = read_everything(ce, batch, n, w, h, intensity)
    finally:
        batch.close()
    WG.identical(got, again)
    for p, (name, r, t) in enumerate(cs):
        label = f"{name} {w}x{h} {rd}/{td} @{intensity:g}"
        check_pair(ce, oracle, shims, label, got, p, ref, p, w, h, rd, td, (r, t))
        if p != p_new:
            assert pair_of(after, p) == pair_of(got, p), (label, "changed by another pair's upload")
    check_pair(ce, oracle, shims, f"{new_case[0]} {w}x{h} {rd}/{td} @{intensity:g}", after, p_new, ref_new, 0, w, h, rd, td, new_case[1:])
    assert pair_of(after, p_new) != pair_of(got, p_new)
    # over-range samples score and map as their clamped copy
    names = [c[0] for c in cs]
    if "extremes_over" in names:
        a, c = names.index("extremes_over"), names.index("extremes")
        same_bits(got["diffmap"][a], got["diffmap"][c], (names[a], "diffmap against the clamped copy's"))
        assert pair_of(got, a) == pair_of(got, c)
    # the one-pair call, on the samples as uploaded
    cfg = ce.MetricConfig.all()
    for p in (names.index("bytes"), len(cs) - 1 if "extremes_over" not in names else names.index("extremes_over")):
        leaf = gpu_ctx.eval_pair_deep(cs[p][1], rd, cs[p][2], td, w, h, cfg, intensity)
        dssim, ssim2, ba, _, _, psnr = got["scores"][p]
        assert (leaf.dssim, leaf.ssimulacra2, leaf.butteraugli, leaf.psnr) == (dssim, ssim2, ba, psnr if rd == td else None), (names[p], leaf)
    print({k: f"{v:.3e}" for k, v in WG.worst.items()})

