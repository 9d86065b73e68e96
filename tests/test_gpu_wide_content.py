"""Linear batches against the oracle over their whole operand range (tests/wide_content.py; DESIGN.md section 15, "Operand ranges").

A linear batch takes any float in +-1024, negatives and subnormals included, at any intensity target; the metric kernels'
hand-expanded divisions were written for 8-bit sRGB.  Here every class of wide content goes through gpu_ctx.batch_linear - one
batch per shape with all classes as its pairs, several references - at intensity targets 80, 203 and 10000, and every
per-pixel map and score is held to tests/linear_input_shim.py (the oracle's own stages from float planes on) with the bounds
the 8-bit map tests hold: Butteraugli's diffmap and score bit for bit with the two device switches on, DSSIM's maps bit for
bit, SSIMULACRA2's SSIM-error maps bit for bit and its artifact / detail-lost maps within EDGE_REL with the same zeros.
Non-finite values must sit at the same pixels with the same class (NaN, +inf, -inf) on both sides; on this content the
reference has none (tests/test_wide_content_cpu.py).

EDGE_REL (2^-20, established on 8-bit content) holds here as it is: the device's artifact / detail-lost values deviate
from the reference's f64 value, rounded to f32, by at most 2.4e-7 relative on this set (measured on an MI355X; the test prints
it).  The reference's own spread between that f64 value and the same expression (1 + |e2|) / (1 + |e1|) - 1 evaluated in f32
is printed beside it and is no yardstick: the f32 form cancels, up to 127 relative on logramp - which is why the device
forms (|e2| - |e1|) / (1 + |e1|) instead (ssim2.hip).
"""
import collections
import math

import numpy as np
import pytest

import ba_diffmap_shim as BA
import dssim_map_shim as DS
import linear_input_shim as LS
import ssim2_map_shim as S2
import wide_content as WC
from test_gpu_butteraugli import DEVICE_SWITCHES, REL_TOL
from test_gpu_linear_input import FLOORS, read_slab
from test_gpu_ssimulacra2_maps import EDGE_REL

pytestmark = pytest.mark.gpu

PNORM_REL = 1e-13  # tests/test_gpu_butteraugli.py: the 3-norm with the device switches on
DSSIM_SCALE_ABS, DSSIM_FROM_SCALES_REL, DSSIM_REL, DSSIM_FLOOR = 1e-12, 1e-12, 1e-9, 1e-6  # tests/test_gpu_dssim_ssim_maps.py: _check_against_shim
SSIM2_SCORE_REL = 1e-6  # tests/test_gpu_soak.py, floor 1.0
SETS = {"working": (WC.W, WC.H, WC.working_set), "odd": (WC.ODD_W, WC.ODD_H, WC.odd_set)}
Reference = collections.namedtuple("Reference", "ba ba_default dssim ssim2 ssim2_default")
worst = collections.defaultdict(float)


@pytest.fixture(scope="module")
def shim(tmp_path_factory, oracle):
    assert DEVICE_SWITCHES == ("ba_malta_f32", "ba_l2_early")  # what LS.Shim.set_device_switches turns on
    return LS.Shim(tmp_path_factory.mktemp("wide_content_shim"))


@pytest.fixture(scope="module")
def content():
    return {key: gen() for key, (_, _, gen) in SETS.items()}


@pytest.fixture(scope="module")
def reference(shim, content):
    """The shim's results per set, computed once: DSSIM and SSIMULACRA2 do not depend on the intensity target."""
    fixed, per_intensity = {}, {}

    def get(key, intensity):
        w, h, _ = SETS[key]
        cases = content[key]
        if key not in fixed:
            fixed[key] = ([shim.dssim_maps(r, t, w, h) for _, r, t in cases], [shim.ssim2_maps(r, t, w, h) for _, r, t in cases],
                          [shim.ssimulacra2(r, t, w, h, 1) for _, r, t in cases])
        if (key, intensity) not in per_intensity:
            default = [shim.butteraugli(r, t, w, h, intensity) for _, r, t in cases]
            shim.set_device_switches(True)
            try:
                on = [shim.butteraugli_map(r, t, w, h, intensity) for _, r, t in cases]
            finally:
                shim.set_device_switches(False)
            per_intensity[(key, intensity)] = (on, default)
        on, default = per_intensity[(key, intensity)]
        return Reference(on, default, *fixed[key])
    return get


def klass(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 3, 0)))


def same_bits(got, want, where):
    """Bit for bit where the reference is finite; the same class of non-finite value at the same pixels elsewhere."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, where
    kg, kw = klass(got), klass(want)
    assert np.array_equal(kg, kw), (where, "non-finite", int((kg != kw).sum()), np.argwhere(kg != kw)[:4].tolist())
    fin = kw == 0
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & fin)
    assert bad.size == 0, (where, len(bad), bad[:4].tolist(), [float(got[tuple(i)]) for i in bad[:4]], [float(want[tuple(i)]) for i in bad[:4]])


def same_value(got, want, tol, where):
    """|got - want| <= tol where the reference is finite, else the same class."""
    if math.isfinite(want):
        assert math.isfinite(got) and abs(got - want) <= tol, (where, got, want, tol)
    else:
        assert int(klass(got)) == int(klass(want)), (where, got, want)


def fill_and_prove(ce, b, refs, tests, pair_ref, config):
    """Uploads, then - behind a first launch, which orders the uploads - the slabs read back: the device holds the bytes the
    test built, before the run that is scored."""
    for i, r in enumerate(refs):
        b.set_reference(i, r)
    for p, (t, ri) in enumerate(zip(tests, pair_ref)):
        b.set_test(p, ri, t)
    b.run(len(tests), config)
    n = refs[0].size
    assert np.array_equal(read_slab(b, 0, len(refs) * n).view(np.uint32), np.concatenate([r.reshape(-1) for r in refs]).view(np.uint32))
    assert np.array_equal(read_slab(b, 1, len(tests) * n).view(np.uint32), np.concatenate([t.reshape(-1) for t in tests]).view(np.uint32))


def read_everything(ce, b, n, w, h, intensity):
    scores = b.run(n, ce.MetricConfig.all(), intensity, butteraugli_diffmap=True, ssimulacra2_maps=True)
    out = {"scores": [(s.dssim, s.ssimulacra2, s.butteraugli, s.valid, s.status) for s in scores], "pnorm3": b.butteraugli_pnorm3(n),
           "diffmap": b.butteraugli_diffmaps(0, n)}
    for lvl in range(len(ce.dssim_levels(w, h))):
        out[f"ds_{lvl}"], out[f"ds_ssim_{lvl}"] = b.dssim_ssim_maps(lvl, 0, n)
    for s in range(len(ce.ssimulacra2_scales(w, h))):
        for c in range(3):
            for k in range(3):
                out[f"s2_{s}_{c}_{k}"], out[f"s2_norm_{s}_{c}_{k}"] = b.ssimulacra2_maps(s, c, k, 0, n)
    return out


def identical(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "scores":
            assert [tuple(np.float64(v).tobytes() for v in s) for s in a[k]] == [tuple(np.float64(v).tobytes() for v in s) for s in b[k]], k
        else:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def note(key, value):
    if math.isfinite(value):
        worst[key] = max(worst[key], value)


def check_butteraugli(name, got, p, ref):
    score, p3, dm = ref.ba[p]
    dev_score, dev_p3 = got["scores"][p][2], float(got["pnorm3"][p])
    same_bits(got["diffmap"][p], dm, (name, "diffmap"))
    if math.isfinite(score):
        assert dev_score == score, (name, dev_score, score)
    else:
        assert int(klass(dev_score)) == int(klass(score)), (name, dev_score, score)
    same_value(dev_p3, p3, PNORM_REL * abs(p3), (name, "3-norm"))
    d_score, d_p3 = ref.ba_default[p]
    floor = FLOORS["butteraugli"]
    gap = abs(dev_score - d_score) / max(abs(d_score), floor)
    note("butteraugli vs the default oracle", gap)
    print(f"{name}: butteraugli device {dev_score!r} default oracle {d_score!r} gap {gap:.3e}")
    same_value(dev_score, d_score, REL_TOL * max(abs(d_score), floor), (name, "default oracle"))
    same_value(dev_p3, d_p3, REL_TOL * max(abs(d_p3), floor), (name, "default oracle 3-norm"))
    assert abs(BA.pnorm3(dm) - p3) <= 1e-12 * max(p3, 1e-300) or not math.isfinite(p3)  # the shim's map is the map of its own score


def check_dssim(name, got, p, want, n_levels):
    want_d, levels = want
    assert len(levels) == n_levels, name
    ssims = []
    for l, (wm, ws) in enumerate(levels):
        same_bits(got[f"ds_{l}"][p], wm, (name, "dssim level", l))
        dev = float(got[f"ds_ssim_{l}"][p])
        same_value(dev, ws, DSSIM_SCALE_ABS, (name, "dssim per-scale score", l))
        ssims.append(dev)
    score = got["scores"][p][0]
    if all(math.isfinite(s) for s in ssims):
        assert abs(DS.dssim_from_scores(ssims) - score) <= DSSIM_FROM_SCALES_REL * max(abs(score), 1e-300), (name, score, ssims)
    same_value(score, want_d, DSSIM_REL * max(abs(want_d), DSSIM_FLOOR), (name, "dssim"))
    note("dssim", abs(score - want_d) / max(abs(want_d), DSSIM_FLOOR))


def check_ssim2(name, oracle, got, p, want, want_default, n_scales):
    assert len(want) == n_scales, name
    for s, (d, e, f) in enumerate(want):
        for c in range(3):
            same_bits(got[f"s2_{s}_{c}_0"][p], d[c], (name, "ssim2 d", s, c))
            for k in (1, 2):
                dev, ref, ref32 = got[f"s2_{s}_{c}_{k}"][p], e[c, k - 1], f[c, k - 1]
                where = (name, "ssim2 edge", s, c, k)
                assert np.array_equal(klass(dev), klass(ref)), where
                fin = np.isfinite(ref)
                assert np.array_equal((dev > 0) & fin, (ref > 0) & fin), (where, int(np.sum(((dev > 0) != (ref > 0)) & fin)))
                assert np.all(dev[fin] >= 0), where
                nz = (ref > 0) & fin
                if np.any(nz):
                    r32 = ref[nz].astype(np.float32).astype(np.float64)
                    ok = r32 > 0
                    dev_rel = float(np.max(np.abs(dev[nz].astype(np.float64)[ok] - r32[ok]) / r32[ok])) if np.any(ok) else 0.0
                    own = float(np.max(np.abs(ref32[nz].astype(np.float64)[ok] - r32[ok]) / r32[ok])) if np.any(ok) else 0.0
                    note("edge maps, device vs the reference's f64 value", dev_rel)
                    note("edge maps, the reference's own f32 vs f64", own)
                    assert dev_rel <= EDGE_REL, (where, dev_rel, own)
    score = got["scores"][p][1]
    pooled = oracle.ssimulacra2_score(S2.features([(d, e) for d, e, _ in want]))  # the maps above, pooled as the score pools them
    same_value(score, pooled, SSIM2_SCORE_REL * max(1.0, abs(pooled)), (name, "ssimulacra2 from the shim's maps"))
    gap = abs(score - want_default) / max(abs(want_default), FLOORS["ssimulacra2"])
    note("ssimulacra2 vs the default oracle", gap)
    print(f"{name}: ssimulacra2 device {score!r} pooled shim maps {pooled!r} default oracle {want_default!r} gap {gap:.3e}")
    same_value(score, want_default, REL_TOL * max(abs(want_default), FLOORS["ssimulacra2"]), (name, "ssimulacra2 default oracle"))


@pytest.mark.parametrize("intensity", WC.INTENSITIES)
@pytest.mark.parametrize("key", sorted(SETS))
def test_every_map_and_score_equals_the_oracle(ce, gpu_ctx, oracle, shim, content, reference, key, intensity):
    w, h, _ = SETS[key]
    cases = content[key]
    refs, tests, pair_ref = WC.grid(cases)
    n = len(tests)
    ref = reference(key, intensity)
    b = gpu_ctx.batch_linear(w, h, len(refs), n)
    try:
        fill_and_prove(ce, b, refs, tests, pair_ref, ce.MetricConfig(dssim=True, ssimulacra2=False, butteraugli=False, psnr=False))
        got = read_everything(ce, b, n, w, h, intensity)
        again = read_everything(ce, b, n, w, h, intensity)
    finally:
        b.close()
    identical(got, again)
    n_levels, n_scales = len(ce.dssim_levels(w, h)), len(ce.ssimulacra2_scales(w, h))
    assert ce.dssim_levels(w, h) == LS.dssim_levels(w, h) and ce.ssimulacra2_scales(w, h) == LS.ssim2_scales(w, h)
    for p, (name, _, _) in enumerate(cases):
        name = f"{name} {w}x{h} @{intensity:g}"
        assert got["scores"][p][3:] == (7, 0), (name, got["scores"][p])  # the three perceptual metrics, no PSNR, no error
        check_butteraugli(name, got, p, ref)
        check_dssim(name, got, p, ref.dssim[p], n_levels)
        check_ssim2(name, oracle, got, p, ref.ssim2[p], ref.ssim2_default[p], n_scales)
        if name.startswith(WC.IDENTICAL):
            assert got["scores"][p][:3] == (0.0, 100.0, 0.0), (name, got["scores"][p])
    print({k: f"{v:.3e}" for k, v in worst.items()})


def test_lab_crossing_dssim(ce, gpu_ctx, shim):
    """Every float32 around the zero of cbrt_poly's first denominator, in grey and in one channel at a time: DSSIM only."""
    w, h = WC.CROSS_W, WC.CROSS_H
    cases = WC.lab_crossing(shim.cbrt_den)
    refs, tests, pair_ref = WC.grid(cases)
    n = len(tests)
    cfg = ce.MetricConfig(dssim=True, ssimulacra2=False, butteraugli=False, psnr=False)
    levels = ce.dssim_levels(w, h)
    assert levels == LS.dssim_levels(w, h)

    def read(b):
        scores = b.run(n, cfg)
        out = {"scores": [(s.dssim, 0.0, 0.0, s.valid, s.status) for s in scores]}
        for lvl in range(len(levels)):
            out[f"ds_{lvl}"], out[f"ds_ssim_{lvl}"] = b.dssim_ssim_maps(lvl, 0, n)
        return out

    b = gpu_ctx.batch_linear(w, h, len(refs), n)
    try:
        fill_and_prove(ce, b, refs, tests, pair_ref, cfg)
        got = read(b)
        again = read(b)
    finally:
        b.close()
    identical(got, again)
    for p, (name, r, t) in enumerate(cases):
        assert got["scores"][p][3:] == (1, 0), (name, got["scores"][p])
        want = shim.dssim_maps(r, t, w, h)
        bad = sum(int((~np.isfinite(m)).sum()) for m, _ in want[1])
        print(f"{name}: dssim device {got['scores'][p][0]!r} shim {want[0]!r}, non-finite reference pixels {bad}")
        check_dssim(name, got, p, want, len(levels))
