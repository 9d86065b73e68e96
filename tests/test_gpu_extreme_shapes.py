"""Every call on the two axes that reach the launch code's limits (shapes, layout and bounds:
tests/extreme_shape_cases.py).

Long thin images: a side past 65535 - coordinates, tile rows and strip indices that no longer fit 16 bits - through a resident
batch of one reference and two tests, launched twice (the second launch finds its references kept: the LF term formed in the
blur, the split SSIMULACRA2 blur, slot grids that start behind the references), and once more through the one-pair leaves.
Many pairs: a batch of 65540 pairs of 8 x 8 images, scored by the calls that take any number of pairs in launches of at most
65535, and refused by the main metrics - before any kernel, whatever ran before - once references plus pairs pass 65535.
Height: the two launches whose grid holds a plane's rows in y refuse an image too tall and score the tallest that fits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_diffmap_shim as BS  # noqa: E402
import ciede2000_cases as CK  # noqa: E402
import dssim_map_shim as DS  # noqa: E402
import ssim2_map_shim as S2  # noqa: E402
from test_gpu_image_heuristics import _check as check_heuristics  # noqa: E402
from test_gpu_ssimulacra2_maps import _check_scale as check_ssim2_scale  # noqa: E402
import ciede2000_restatement as CR  # noqa: E402
import deep_input_shim as D  # noqa: E402
import delta_e_itp_map_restatement as IM  # noqa: E402
import extreme_shape_cases as X  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402
import msssim_cases as MK  # noqa: E402
import msssim_map_restatement as MM  # noqa: E402
import msssim_restatement as M  # noqa: E402
import reference_reuse_cases as R  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- long thin images ------------------------------------------------------------------------------------------------------------

def _thin_batch(ce, ctx, w, h):
    ref, tests = X.thin_images(w, h)
    b = ce.Batch(ctx, w, h, 1, len(tests))
    b.set_reference(0, ref)
    for k, t in enumerate(tests):
        b.set_test(k, 0, t)
    return b, ref, tests


@pytest.mark.parametrize("w,h", X.THIN_ALL, ids=lambda v: str(v))
def test_long_thin_images_score_as_the_oracle_in_a_batch_relaunched_and_through_the_leaves(gpu_ctx, oracle, ce, w, h):
    want = X.thin_oracle(oracle, w, h, "dsb")
    cfg = ce.MetricConfig.all()
    b, ref, tests = _thin_batch(ce, gpu_ctx, w, h)
    try:
        first = R.launch(b, cfg, len(tests))
        assert b.ref_stats() == (1, 1, 1)
        p3 = b.butteraugli_pnorm3(len(tests))
        scores = b.collect(len(tests))
        for k, s in enumerate(scores):
            what = (w, h, X.QUALITIES[k])
            assert s.status == 0 and s.valid == ce.METRIC_DSSIM | ce.METRIC_SSIMULACRA2 | ce.METRIC_BUTTERAUGLI | ce.METRIC_PSNR, what
            print(f"{what}: psnr {s.psnr!r} dssim {s.dssim!r} / {want[k]['dssim']!r} ssimulacra2 {s.ssimulacra2!r} / "
                  f"{want[k]['ssimulacra2']!r} butteraugli {s.butteraugli!r} / {want[k]['butteraugli_device'][0]!r}")
            X.check_psnr(s.psnr, want[k]["psnr"], what)
            X.check_dssim(s.dssim, want[k]["dssim"], what)
            X.check_ssim2(s.ssimulacra2, b.debug_averages(k), want[k]["ssimulacra2"], want[k]["averages"], what)
            X.check_butteraugli(s.butteraugli, float(p3[k]), want[k]["butteraugli_device"], want[k]["butteraugli"], what)
        # the second launch finds its references kept and gives the same bits
        assert R.launch(b, cfg, len(tests)) == first and b.ref_stats() == (1, 1, 1)
        assert b.butteraugli_pnorm3(len(tests)).tobytes() == p3.tobytes()
    finally:
        b.close()
    for k, t in enumerate(tests):
        what = (w, h, X.QUALITIES[k], "leaf")
        X.check_psnr(gpu_ctx.calculate_psnr(ref, t, w, h), want[k]["psnr"], what)
        X.check_dssim(gpu_ctx.calculate_dssim(ref, t, w, h), want[k]["dssim"], what)
        got = gpu_ctx.calculate_ssimulacra2(ref, t, w, h)
        assert abs(got - want[k]["ssimulacra2"]) <= 1e-4 * max(abs(want[k]["ssimulacra2"]), 1.0), (what, got)
        X.check_butteraugli(gpu_ctx.calculate_butteraugli(ref, t, w, h), None, want[k]["butteraugli_device"], want[k]["butteraugli"], what)
    assert gpu_ctx.calculate_dssim(ref, ref, w, h) == 0.0


@pytest.mark.parametrize("w,h", X.THIN_DSSIM, ids=lambda v: str(v))
def test_one_pixel_wide_images_through_dssim_and_psnr(gpu_ctx, oracle, ce, w, h):
    want = X.thin_oracle(oracle, w, h, "d")
    cfg = ce.MetricConfig(dssim=True, psnr=True)
    b, ref, tests = _thin_batch(ce, gpu_ctx, w, h)
    try:
        first = R.launch(b, cfg, len(tests))
        assert b.ref_stats() == (0, 1, 0)
        for k, s in enumerate(b.collect(len(tests))):
            assert s.status == 0 and s.valid == ce.METRIC_DSSIM | ce.METRIC_PSNR
            X.check_psnr(s.psnr, want[k]["psnr"], (w, h, k))
            X.check_dssim(s.dssim, want[k]["dssim"], (w, h, k))
        assert R.launch(b, cfg, len(tests)) == first and b.ref_stats() == (0, 1, 0)
    finally:
        b.close()
    for k, t in enumerate(tests):
        X.check_psnr(gpu_ctx.calculate_psnr(ref, t, w, h), want[k]["psnr"], (w, h, k, "leaf"))
        X.check_dssim(gpu_ctx.calculate_dssim(ref, t, w, h), want[k]["dssim"], (w, h, k, "leaf"))
    assert gpu_ctx.calculate_dssim(ref, ref, w, h) == 0.0


@pytest.mark.parametrize("w,h,levels", [s + (1,) for s in X.THIN_SSIM] + [s + (5,) for s in X.THIN_MS_SSIM], ids=lambda v: str(v))
def test_long_thin_images_through_ssim_and_ms_ssim(gpu_ctx, ce, w, h, levels):
    b, ref, tests = _thin_batch(ce, gpu_ctx, w, h)
    try:
        got = b.ms_ssim(len(tests), levels)
        assert [(a.ssim_q, a.cs_q, a.n) for a in b.ms_ssim(len(tests), levels)] == [(g.ssim_q, g.cs_q, g.n) for g in got]
    finally:
        b.close()
    for k, t in enumerate(tests):
        want = M.msssim(ref, t, 8, levels)
        MK.check_integers(got[k], want, (w, h, levels, k))
        MK.check_integers(gpu_ctx.ms_ssim(ref, t, w, h, levels), want, (w, h, levels, k, "leaf"))
        assert got[k].n[0] == (w - 10) * (h - 10)


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    return (BS.Shim(tmp_path_factory.mktemp("ba_shim")), DS.Shim(tmp_path_factory.mktemp("dssim_shim")),
            S2.Shim(tmp_path_factory.mktemp("ssim2_map_shim")))


CELLS = (8, 64)  # with B = 1, the map itself: a cell as wide as the image, and wider


@pytest.mark.parametrize("w,h", X.THIN_ALL[:2], ids=lambda v: str(v))
def test_long_thin_maps_are_the_oracle_maps(gpu_ctx, ce, shims, w, h):
    """The Butteraugli diffmap, DSSIM's SSIM map of every level and SSIMULACRA2's nine maps of every scale, of a launch that
    found its references kept; each held as its own test holds it (test_gpu_butteraugli_diffmap.py: ==;
    test_gpu_dssim_ssim_maps.py: == and 1e-12 on a level's score; test_gpu_ssimulacra2_maps.py: == on the error map, EDGE_REL on
    artifact and detail-lost), and the cell readouts at B = 8 and 64 as the cell maxima / minima of the full maps."""
    ba, ds, s2 = shims
    cfg = ce.MetricConfig.all()
    b, ref, tests = _thin_batch(ce, gpu_ctx, w, h)
    n = len(tests)
    try:
        plain = R.launch(b, cfg, n)
        assert R.launch(b, cfg, n, butteraugli_diffmap=True, ssimulacra2_maps=True) == plain and b.ref_stats() == (1, 1, 1)
        scores = b.collect(n)
        p3 = b.butteraugli_pnorm3(n)
        dm = b.butteraugli_diffmaps(0, n)
        dm_cells = {B: b.butteraugli_diffmaps(0, n, B) for B in CELLS}
        levels = ce.dssim_levels(w, h)
        ds_maps = [b.dssim_ssim_maps(l, 0, n) for l in range(len(levels))]
        ds_cells = {(l, B): b.dssim_ssim_maps(l, 0, n, B) for l in range(len(levels)) for B in CELLS}
        scales = ce.ssimulacra2_scales(w, h)
        s2_maps = {(s, c, k): b.ssimulacra2_maps(s, c, k, 0, n) for s in range(len(scales)) for c in range(3) for k in range(3)}
        s2_cells = {(s, c, k, B): b.ssimulacra2_maps(s, c, k, 0, n, B) for s in range(len(scales)) for c in range(3) for k in range(3)
                    for B in CELLS}
    finally:
        b.close()
    assert [(m.shape[2], m.shape[1]) for m, _ in ds_maps] == levels == ds.levels(w, h)
    ba.set_device_switches(True)
    try:
        want_dm = [ba.diffmap(ref, t, w, h) for t in tests]
    finally:
        ba.set_device_switches(False)
    for i, t in enumerate(tests):
        where = (w, h, X.QUALITIES[i])
        assert dm[i].shape == (h, w) and np.array_equal(dm[i].view(np.uint32), want_dm[i].view(np.uint32)), where
        assert float(dm[i].max()) == scores[i].butteraugli and abs(BS.pnorm3(dm[i]) - p3[i]) <= 1e-12 * p3[i], where
        for B in CELLS:
            assert dm_cells[B][i].tobytes() == BS.block_max(dm[i], B).tobytes(), where + (B,)
        want_d, want = ds.maps(ref, t, w, h)
        for l, (wm, ws) in enumerate(want):
            got, ssim = ds_maps[l][0][i], ds_maps[l][1][i]
            assert np.array_equal(got.view(np.uint32), wm.view(np.uint32)) and abs(ssim - ws) <= 1e-12, where + (l,)
            for B in CELLS:
                assert ds_cells[(l, B)][0][i].tobytes() == DS.block_min(got, B).tobytes(), where + (l, B)
        X.check_dssim(scores[i].dssim, want_d, where)
        want_s2 = s2.maps(ref, t, w, h)
        assert len(want_s2) == len(scales)
        for s in range(len(scales)):
            dev = np.stack([np.stack([s2_maps[(s, c, k)][0][i] for k in range(3)]) for c in range(3)])
            check_ssim2_scale(dev, want_s2[s], where + (s,))
            for c in range(3):
                for k in range(3):
                    for B in CELLS:
                        assert s2_cells[(s, c, k, B)][0][i].tobytes() == S2.cell_max(dev[c, k], B).tobytes(), where + (s, c, k, B)


@pytest.mark.parametrize("w,h", X.THIN_SSIM, ids=lambda v: str(v))
def test_long_thin_ssim_map_is_the_restatement(gpu_ctx, ce, w, h):
    """The SSIM map at level 0 of one level - 8 pixels across hold no 11-tap window, so on the shapes that do; test_gpu_msssim_map.py: ==."""
    thresholds = [0, MM.Q32 // 100, MM.Q32 // 10, MM.U32_MAX]
    b, ref, tests = _thin_batch(ce, gpu_ctx, w, h)
    n = len(tests)
    try:
        got = {(what, B): b.ms_ssim_maps(0, n, 1, 0, what, B, thresholds) for what in ("ssim", "cs") for B in (1,) + CELLS}
    finally:
        b.close()
    for what in ("ssim", "cs"):
        for i, t in enumerate(tests):
            m = MM.full_map(ref, t, 8, 1, 0, what)
            assert m.shape == (3, h - 10, w - 10)
            for B in (1,) + CELLS:
                maps, over = got[(what, B)]
                assert np.array_equal(maps[i], MM.cells(m, B)) and np.array_equal(over[i], MM.over(m, thresholds)), (w, h, what, i, B)
            leaf, leaf_over = gpu_ctx.ms_ssim_map(ref, t, w, h, 1, 0, what, 1, thresholds)
            assert np.array_equal(leaf[0], m) and np.array_equal(leaf_over[0], MM.over(m, thresholds))


@pytest.mark.parametrize("w,h", X.THIN_ALL[:2], ids=lambda v: str(v))
def test_long_thin_image_heuristics(gpu_ctx, ce, w, h):
    b, ref, tests = _thin_batch(ce, gpu_ctx, w, h)
    try:
        check_heuristics(b.image_heuristics(0, 1)[0], ref, w, h, (w, h, "reference"))
        for i, got in enumerate(b.image_heuristics(0, len(tests), tests=True)):
            check_heuristics(got, tests[i], w, h, (w, h, i))
    finally:
        b.close()
    check_heuristics(gpu_ctx.image_heuristics(ref, w, h), ref, w, h, (w, h, "leaf"))


# ---- many pairs ------------------------------------------------------------------------------------------------------------------

def _many_batch(ce, ctx, kind, w, h):
    refs8, tests8 = X.many_images(w, h)
    refs, tests = [R.convert(ce, kind, a) for a in refs8], [R.convert(ce, kind, a) for a in tests8]
    if kind == "linear":
        b = ctx.batch_linear(w, h, X.MAX_REFS, X.MAX_PAIRS)
    elif kind == "deep":
        b = ctx.batch_deep(w, h, X.MAX_REFS, X.MAX_PAIRS, 16, 16)
    else:
        b = ce.Batch(ctx, w, h, X.MAX_REFS, X.MAX_PAIRS)
    X.fill_many(ce, b, refs, tests)
    return b, refs, tests, refs8, tests8


def _pair(refs, tests, p):
    return refs[p % X.MAX_REFS], tests[p % X.K_TESTS]


def _main_metrics_at_and_past_the_slots(ce, b, cfg, rewrite):
    """FITS pairs score, every pair as its twin; every count past the slots is refused with the limit in the message, as a first
    launch after a reference write and with the references kept, and leaves the batch as it was.  -> the score rows of FITS."""
    want_stats = tuple(int(x) for x in (cfg.ssimulacra2, cfg.dssim, cfg.butteraugli))
    b.launch(X.FITS, cfg)
    rows = X.score_rows(b.collect(X.FITS))
    p3 = b.butteraugli_pnorm3(X.FITS)
    assert b.ref_stats() == want_stats
    X.assert_twins(rows, "scores")
    X.assert_twins(p3, "3-norm")
    for n in X.PAST:
        slots = f"{X.MAX_REFS} references + {n} pairs = {X.MAX_REFS + n} image slots"
        # with the references kept: refused, and the next launch rebuilds nothing and gives the same bits
        X.refused(ce, lambda: b.launch(n, cfg), slots, f"at most {X.SLOTS_MAX} slots")
        b.launch(X.FITS, cfg)
        assert b.ref_stats() == want_stats
        assert np.array_equal(X.score_rows(b.collect(X.FITS)), rows) and b.butteraugli_pnorm3(X.FITS).tobytes() == p3.tobytes()
        # as a first launch after a reference write: the same refusal; the write costs the next launch one rebuild
        rewrite()
        X.refused(ce, lambda: b.launch(n, cfg), slots, f"at most {X.SLOTS_MAX} slots")
        b.launch(X.FITS, cfg)
        want_stats = tuple(s + 1 for s in want_stats)
        assert b.ref_stats() == want_stats
        assert np.array_equal(X.score_rows(b.collect(X.FITS)), rows)
    # the rule counts slots, not pairs: one reference and 65534 pairs fit
    return rows, p3


def test_many_pairs_rgb8(gpu_ctx, oracle, ce):
    w = h = 8
    cfg = ce.MetricConfig.all()
    b, refs, tests, _, _ = _many_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        rows, p3 = _main_metrics_at_and_past_the_slots(ce, b, cfg, lambda: b.set_reference(1, refs[1]))
        # the first 21 pairs against the oracle, as the long thin images are
        assert oracle.variants_all_default()
        b.launch(X.TWINS, cfg)
        scores = b.collect(X.TWINS)
        assert np.array_equal(X.score_rows(scores), rows[:X.TWINS])
        avgs = [b.debug_averages(p) for p in range(X.TWINS)]
        CK.use(ce)
        cie = b.ciede2000(X.FITS, CK.THRESHOLDS)
        X.assert_twin_items(cie, ("sum_q20", "max_q20", "n", "n_above"), "ciede2000")
        for p in range(X.TWINS):
            r, t = _pair(refs, tests, p)
            s = scores[p]
            X.check_psnr(s.psnr, oracle.psnr(r, t, w, h), p)
            X.check_dssim(s.dssim, oracle.dssim(r, t, w, h), p)
            want, want_avg = oracle.ssimulacra2_detail(r, t, w, h, 1)
            X.check_ssim2(s.ssimulacra2, avgs[p], want, want_avg, p)
            base = oracle.butteraugli(r, t, w, h)
            for v in X.DEVICE_SWITCHES:
                oracle.set_variant(v, 1)
            try:
                same = oracle.butteraugli(r, t, w, h)
            finally:
                for v in X.DEVICE_SWITCHES:
                    oracle.set_variant(v, 0)
            X.check_butteraugli(s.butteraugli, float(p3[p]), same, base, p)
            CK.check(cie[p], CR.scores(CK.q_of(r, t, (0, 0)), CK.THRESHOLDS), p)
        # PSNR and CIEDE2000 take any number of pairs, in launches of at most 65535
        only = ce.MetricConfig(psnr=True)
        for n in X.PAST:
            b.launch(n, only)
            got = X.score_rows(b.collect(n))
            X.assert_twins(got, ("psnr", n))
            assert np.array_equal(got[:X.TWINS, 5], rows[:X.TWINS, 5]) and (got[:, 1] == ce.METRIC_PSNR).all()
            more = b.ciede2000(n, CK.THRESHOLDS)
            assert more[:X.TWINS] == cie[:X.TWINS]
            X.assert_twin_items(more, ("sum_q20", "max_q20", "n", "n_above"), ("ciede2000", n))
        assert b.ref_stats() == (4, 4, 4)  # none of that touched the references' state
        # slots, not pairs: bound to reference 0 alone, 65534 pairs fit and 65535 do not
        for p in range(1, 65535, 1):
            if p % X.MAX_REFS:
                b.bind_pair(p, 0)
        X.refused(ce, lambda: b.launch(65535, cfg), "1 references + 65535 pairs = 65536 image slots")
        b.launch(65534, cfg)
        one_ref = X.score_rows(b.collect(65534))
        assert b.ref_stats() == (4, 4, 4)  # fewer references than the state covers
        same_pair = np.arange(65534) % X.MAX_REFS == 0
        assert np.array_equal(one_ref[same_pair], rows[np.arange(65534)[same_pair] % X.TWINS])
    finally:
        b.close()


def test_many_pairs_deep(gpu_ctx, ce):
    """A 16 / 16 batch: k_psnr_sse_u16 and k_ciede2000<true> past a grid's y; the main metrics at the slots and refused past them."""
    w = h = 8
    b, refs, tests, _, _ = _many_batch(ce, gpu_ctx, "deep", w, h)
    try:
        rows, _ = _main_metrics_at_and_past_the_slots(ce, b, ce.MetricConfig.all(), lambda: b.set_reference(1, refs[1]))
        CK.use(ce)
        only = ce.MetricConfig(psnr=True)
        want_psnr = [D.psnr_from_sse(int(((_pair(refs, tests, p)[0].astype(np.int64) - _pair(refs, tests, p)[1].astype(np.int64)) ** 2).sum()),
                                     w, h, 16) for p in range(X.TWINS)]
        want_cie = [CR.scores(CK.q_of(*_pair(refs, tests, p), (16, 16)), CK.THRESHOLDS) for p in range(X.TWINS)]
        for n in (X.FITS,) + X.PAST:
            b.launch(n, only)
            got = b.collect(n)
            assert [s.psnr for s in got[:X.TWINS]] == want_psnr
            X.assert_twins(X.score_rows(got), ("psnr", n))
            cie = b.ciede2000(n, CK.THRESHOLDS)
            for p in range(X.TWINS):
                CK.check(cie[p], want_cie[p], (n, p))
            X.assert_twin_items(cie, ("sum_q20", "max_q20", "n", "n_above"), ("ciede2000", n))
        assert np.array_equal(rows[:X.TWINS, 5], np.array(want_psnr, np.float64).view(np.uint64))
    finally:
        b.close()


def test_many_pairs_linear(gpu_ctx, ce):
    """A linear batch: k_hdr_fidelity and k_delta_e_itp_map past a grid's y, the maps of the last ten pairs."""
    w = h = 8
    depth, white = 12, 203.0
    b, refs, tests, _, _ = _many_batch(ce, gpu_ctx, "linear", w, h)
    try:
        _main_metrics_at_and_past_the_slots(ce, b, ce.MetricConfig(dssim=True, ssimulacra2=True, butteraugli=True),
                                            lambda: b.set_reference(1, refs[1]))
        shape = lambda a: np.asarray(a, np.float32).reshape(h, w, 3)  # noqa: E731
        want = [F.fidelity(*_pair(refs, tests, p), depth, white) for p in range(X.TWINS)]
        maps = [IM.full_map(shape(_pair(refs, tests, p)[0]), shape(_pair(refs, tests, p)[1]), depth, white) for p in range(X.TWINS)]
        for n in (X.FITS,) + X.PAST:
            got = b.hdr_fidelity(n, depth, white)
            for p in range(X.TWINS):
                assert (got[p].pq_sse, got[p].itp_sum_q20, got[p].itp_max_q20) == (want[p]["pq_sse"], want[p]["itp_sum_q20"], want[p]["itp_max_q20"]), (n, p)
                assert (got[p].pq_psnr, got[p].delta_e_itp_mean, got[p].delta_e_itp_max) == (want[p]["pq_psnr"], want[p]["delta_e_itp_mean"], want[p]["delta_e_itp_max"])
            X.assert_twin_items(got, ("pq_sse", "itp_sum_q20", "itp_max_q20"), ("hdr_fidelity", n))
        first, count = X.TAIL
        for block in (1, 8):
            got, over = b.delta_e_itp_maps(first, count, depth, white, block, IM.THRESHOLDS)
            for i in range(count):
                m = maps[(first + i) % X.TWINS]
                assert np.array_equal(got[i], IM.block_max(m, block)), (block, i)
                assert np.array_equal(over[i], IM.over(m, IM.THRESHOLDS)), (block, i)
        # every pair's counts, in two launches: the whole batch through the map kernel
        _, over = b.delta_e_itp_maps(0, X.MAX_PAIRS, depth, white, 1, IM.THRESHOLDS, maps=False)
        X.assert_twins(over, "delta_e_itp counts")
        assert np.array_equal(over[:X.TWINS], np.stack([IM.over(m, IM.THRESHOLDS) for m in maps]))
    finally:
        b.close()


def test_many_pairs_ssim(gpu_ctx, ce):
    """An 11 x 11 RGB8 batch: SSIM at one level - one valid position - and its map, of any number of pairs."""
    w = h = 11
    b, refs, tests, _, _ = _many_batch(ce, gpu_ctx, "rgb8", w, h)
    try:
        shape = lambda a: np.asarray(a).reshape(h, w, 3)  # noqa: E731
        want = [M.msssim(shape(_pair(refs, tests, p)[0]), shape(_pair(refs, tests, p)[1]), 8, 1) for p in range(X.TWINS)]
        for n in (X.FITS,) + X.PAST:
            got = b.ms_ssim(n, 1)
            for p in range(X.TWINS):
                MK.check_integers(got[p], want[p], (n, p))
            X.assert_twin_items(got, ("ssim_q", "cs_q", "n", "n_levels"), ("ssim", n))
        first, count = X.TAIL
        thresholds = [0, MM.Q32 // 100, MM.Q32 // 10, MM.U32_MAX]
        for what in ("ssim", "cs"):
            got, over = b.ms_ssim_maps(first, count, 1, 0, what, 1, thresholds)
            assert got.shape == (count, 3, 1, 1)
            for i in range(count):
                r, t = _pair(refs, tests, first + i)
                m = MM.full_map(shape(r), shape(t), 8, 1, 0, what)
                assert np.array_equal(got[i], m) and np.array_equal(over[i], MM.over(m, thresholds)), (what, i)
        _, over = b.ms_ssim_maps(0, X.MAX_PAIRS, 1, 0, "ssim", 1, thresholds, maps=False)
        X.assert_twins(over, "ssim map counts")
    finally:
        b.close()


def test_eval_batch_of_70000_items_equals_its_one_pair_calls(ce):
    """ce_eval_batch plans its chunks under the launch's slots (ce_plan.h: ce_plan_bucket): 70 000 items of 8 x 8 on three
    distinct references, item i the twin of item i % 21, each equal to its one-pair call."""
    w = h = 8
    refs, tests = X.many_images(w, h)
    cfg = ce.MetricConfig.all()
    n = 70000
    with ce.Context(0) as ctx:
        items = [(refs[p % X.MAX_REFS], tests[p % X.K_TESTS], w, h) for p in range(n)]
        got = X.score_rows(ctx.eval_batch(items, cfg))
        X.assert_twins(got, "eval_batch")
        for p in range(X.TWINS):
            r, t, _, _ = items[p]
            m = ctx.calculate_metrics(r, t, w, h, cfg)
            want = np.array([m.dssim, m.ssimulacra2, m.butteraugli, m.psnr], np.float64).view(np.uint64)
            assert got[p, 0] == 0 and np.array_equal(got[p, 2:], want), (p, got[p], want)


# ---- height ----------------------------------------------------------------------------------------------------------------------

def _tall(w, h, seed):
    ref = X.wl.make_reference(w, h, seed)
    return ref, X.wl.distort(ref, 60)


def test_butteraugli_refuses_an_image_too_tall_and_scores_the_tallest_that_fits(gpu_ctx, oracle, ce):
    w = 8
    h = X.BA_HEIGHT_MAX
    ref, t = _tall(w, h, 7201)
    base = oracle.butteraugli(ref, t, w, h)
    for v in X.DEVICE_SWITCHES:
        oracle.set_variant(v, 1)
    try:
        same = oracle.butteraugli(ref, t, w, h)
    finally:
        for v in X.DEVICE_SWITCHES:
            oracle.set_variant(v, 0)
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference(0, ref)
        b.set_test(0, 0, t)
        s = b.run(1, ce.MetricConfig(butteraugli=True))[0]
        X.check_butteraugli(s.butteraugli, float(b.butteraugli_pnorm3(1)[0]), same, base, (w, h))
    finally:
        b.close()
    h = 262148
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        img = np.zeros((h, w, 3), np.uint8)
        b.set_reference(0, img)
        b.set_test(0, 0, img)
        X.refused(ce, lambda: b.launch(1, ce.MetricConfig.all()), f"height {h}", f"Butteraugli takes at most {X.BA_HEIGHT_MAX} rows")
        assert b.ref_stats() == (0, 0, 0)
        s = b.run(1, ce.MetricConfig(dssim=True, ssimulacra2=True, psnr=True))[0]  # the others take it
        assert s.status == 0 and s.dssim == 0.0 and s.ssimulacra2 == 100.0 and b.ref_stats() == (1, 1, 0)
    finally:
        b.close()


def test_ssimulacra2_refuses_an_image_too_tall_and_scores_the_tallest_that_fits(gpu_ctx, oracle, ce):
    w = 8
    h = X.SSIM2_HEIGHT_MAX
    ref, t = _tall(w, h, 7202)
    want, want_avg = oracle.ssimulacra2_detail(ref, t, w, h, 1)
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        b.set_reference(0, ref)
        b.set_test(0, 0, t)
        s = b.run(1, ce.MetricConfig.ssimulacra2_only())[0]
        X.check_ssim2(s.ssimulacra2, b.debug_averages(0), want, want_avg, (w, h))
    finally:
        b.close()
    h = 524288
    b = ce.Batch(gpu_ctx, w, h, 1, 1)
    try:
        img = np.zeros((h, w, 3), np.uint8)
        b.set_reference(0, img)
        b.set_test(0, 0, img)
        X.refused(ce, lambda: b.launch(1, ce.MetricConfig.ssimulacra2_only()), f"height {h}", f"SSIMULACRA2 takes at most {X.SSIM2_HEIGHT_MAX} rows")
        assert b.ref_stats() == (0, 0, 0)
        s = b.run(1, ce.MetricConfig(dssim=True, psnr=True))[0]
        assert s.status == 0 and s.dssim == 0.0 and b.ref_stats() == (0, 1, 0)
    finally:
        b.close()
