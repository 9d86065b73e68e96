"""What the reference does on wide content (tests/wide_content.py; DESIGN.md section 15, "Operand ranges"): the oracle's own stages from float
planes on (tests/linear_input_shim.py) stay finite on every legal sample of a linear batch, the content really drives the
operands of the hand-expanded divisions out of the ranges 8-bit input keeps them in, and the two arithmetic switches the
device runs with are worth no more there than on 8-bit content.  No GPU."""
import json
import math
import os
import re

import numpy as np
import pytest

import cicp_restatement as R
import linear_input_shim as LS
import wide_content as WC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SWITCHES = {"ba_malta_f32": LS.BA_MALTA_F32, "ba_l2_early": LS.BA_L2_EARLY}  # tests/test_gpu_butteraugli.py: DEVICE_SWITCHES
ADOPTION_BAR = 1e-6  # the ledger's bar for a switch the device adopts (tests/test_crate_pin.py)
BA_FLOOR = 1e-3  # tests/golden/sensitivity.py: FLOOR


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return LS.Shim(tmp_path_factory.mktemp("wide_content_shim"))


@pytest.fixture(scope="module")
def crossing(shim):
    return WC.lab_crossing(shim.cbrt_den)


def all_sets():
    return [(WC.W, WC.H, WC.working_set()), (WC.ODD_W, WC.ODD_H, WC.odd_set())]


def test_content_is_legal_and_as_described():
    names = set()
    for w, h, cases in all_sets():
        for name, ref, test in cases:
            names.add(name)
            for a in (ref, test):
                assert a.dtype == np.float32 and a.shape == (h, w, 3)
                assert np.array_equal(R.sanitise(a).view(np.uint32), a.view(np.uint32)), name  # what a linear batch keeps bit for bit
    assert {"logramp_x1.05", "logramp_noise", "checker", "spikes", "neg_noise", "hdr_noise", "lab_threshold", "saturated_+1024_-1024",
            "saturated_0_0", WC.IDENTICAL} == names
    ramp = WC.logramp_ref(WC.W, WC.H)
    assert ramp.max() == 1024.0 and ramp.min() == -1024.0 and np.abs(ramp[ramp != 0]).min() == WC.SMALLEST_SUBNORMAL
    assert (ramp[0] > 0).all() and (ramp[WC.H // 3] < 0).all() and (np.sign(ramp[-1, :, 0]) == -np.sign(ramp[-1, :, 1])).all()
    lab = WC.lab_threshold(WC.W, WC.H)[0][1]
    grey = lab[:WC.H // 5, :, 0].astype(np.float64)
    zero = lab[4 * (WC.H // 5):]
    assert grey.min() < WC.LAB_EPSILON < grey.max() and (zero < 0).any() and (zero > 0).any()
    assert ((np.abs(zero) < 1.17549435e-38) & (zero < 0)).any() and ((np.abs(zero) < 1.17549435e-38) & (zero > 0)).any()  # subnormals on either side of 0
    refs, tests, pair_ref = WC.grid(WC.working_set())
    assert len(refs) < len(tests) and max(pair_ref) == len(refs) - 1  # several references, one of them shared


def run_set(shim, w, h, cases, intensity, report):
    """(a) on one set at one intensity; -> {name: butteraugli score}"""
    scores = {}
    for name, ref, test in cases:
        ba, p3, dm = shim.butteraugli_map(ref, test, w, h, intensity)
        ds, levels = shim.dssim_maps(ref, test, w, h)
        s2 = shim.ssimulacra2(ref, test, w, h, 1)
        maps = shim.ssim2_maps(ref, test, w, h)
        report.append(f"{name} {w}x{h} @{intensity:g}: butteraugli {ba!r} 3-norm {p3!r} dssim {ds!r} ssimulacra2 {s2!r}")
        assert all(math.isfinite(v) for v in (ba, p3, ds, s2)), (name, intensity, ba, p3, ds, s2)
        assert np.isfinite(dm).all(), (name, intensity)
        for m, s in levels:
            assert np.isfinite(m).all() and math.isfinite(s), (name, intensity)
        for d, e, f in maps:
            assert np.isfinite(d).all() and np.isfinite(e).all() and np.isfinite(f).all(), (name, intensity)
        if name == WC.IDENTICAL:
            assert (s2, ba, ds) == (100.0, 0.0, 0.0), (s2, ba, ds)
        scores[name] = ba
    return scores


@pytest.fixture(scope="module")
def swept(shim, crossing):
    """Every case of both shapes at every intensity through all three metrics, then lab_crossing through DSSIM, with the
    probe recording: -> (probe of the 96 x 64 / 97 x 35 sets, probe with lab_crossing added, the crossing's maps, report)."""
    report = []
    shim.probe_reset()
    for w, h, cases in all_sets():
        for it in WC.INTENSITIES:
            run_set(shim, w, h, cases, it, report)
    before = shim.probe()
    cross = [(name, shim.dssim_maps(ref, test, WC.CROSS_W, WC.CROSS_H)) for name, ref, test in crossing]
    print("\n".join(report))
    return before, shim.probe(), cross


def unit_range_probe(shim):
    """The probe over content an RGB8 or deep batch can hold - table values in [0, 1]: golden inputs, uniform random codes
    and a black / white checker, at the three intensity targets."""
    table = R.transfer_table(13, 8)
    gold = np.load(os.path.join(GOLD, "inputs.npz"))
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (64, 96, 3)).astype(np.uint8)
    y, x = np.mgrid[0:64, 0:96]
    bw = np.repeat(np.where((x + y) % 2 == 0, 255, 0).astype(np.uint8)[..., None], 3, axis=-1)
    pairs = [(gold[n + ".ref"], gold[n + ".test"]) for n in ("nat64_q40", "nat97x131_q75_420", "min8x8_q50")]
    pairs += [(noise, noise[::-1].copy()), (bw, 255 - bw), (np.zeros_like(bw), bw)]
    shim.probe_reset()
    for ref, test in pairs:
        h, w = ref.shape[:2]
        r, t = table[ref], table[test]
        shim.dssim(r, t, w, h)
        for it in WC.INTENSITIES:
            shim.butteraugli(r, t, w, h, it)
    return shim.probe()


def test_b0_unit_range_content_keeps_the_ranges_the_kernels_were_written_for(shim):
    """What the comments at the division sites state for RGB8 and deep batches, measured the same way."""
    p = unit_range_probe(shim)
    print(format_probe(p))
    c1, c2, lg, gp, m0, m1 = (p[s] for s in LS.DIV_SITES)
    for c in (c1, c2):
        assert 2.0 ** -8 < c["num_min"] and c["num_max"] < 8.0 and 0.016 <= c["den_min"] and c["den_max"] < 8.0 and int(c["signs"]) == 5
    assert 1.0 < gp["den_min"] and gp["den_max"] < 2.0 ** 14 and 21.0 < gp["num_min"] and gp["num_max"] < 150.0  # the opsin bias keeps p off its clamp
    for m in (m0, m1):
        assert 5.0 <= m["den_min"] and m["den_max"] < 2.0 ** 28 and 1.0 < m["num_min"] and m["num_max"] < 4.1e7
    for site, r in p.items():
        assert 2.0 ** -40 < min(r["num_min"], r["den_min"], r["quot_min"]) and max(r["num_max"], r["den_max"], r["quot_max"]) < 2.0 ** 40, site


def test_a_reference_is_finite_everywhere_but_at_the_lab_crossing(swept):
    _, _, cross = swept  # the fixture asserted finiteness of everything else
    for name, (ds, levels) in cross:
        total = sum(m.size for m, _ in levels)
        bad = sum(int((~np.isfinite(m)).sum()) for m, _ in levels)
        print(f"{name}: dssim {ds!r}, non-finite map pixels {bad} of {total} ({[int((~np.isfinite(m)).sum()) for m, _ in levels]} per level)")
        assert bad <= 0.01 * total, (name, bad, total)  # a condition on the content: the window is chosen to meet it


def format_probe(p):
    rows = ["site | |num| | |den| | |quot| | signs num/den | zero num/den | subnormal num/den/quot | non-finite quot"]
    for site, r in p.items():
        sg = int(r["signs"])
        signs = ("+" if sg & 1 else "") + ("-" if sg & 2 else "") + " / " + ("+" if sg & 4 else "") + ("-" if sg & 8 else "")
        rows.append(f"{site} | {r['num_min']:.3g} .. {r['num_max']:.3g} | {r['den_min']:.3g} .. {r['den_max']:.3g} | "
                    f"{r['quot_min']:.3g} .. {r['quot_max']:.3g} | {signs} | {r['num_zero']:.0f} / {r['den_zero']:.0f} | "
                    f"{r['num_subnormal']:.0f} / {r['den_subnormal']:.0f} / {r['quot_subnormal']:.0f} | {r['quot_nonfinite']:.0f}")
    return "\n".join(rows)


def binade(v, up):
    """v rounded outward to a power of two, as its exponent."""
    return math.ceil(math.log2(v)) if up else math.floor(math.log2(v))


def test_b_the_content_leaves_the_8bit_operand_ranges(swept, crossing):
    before, p, _ = swept
    print(format_probe(p))
    envelope = {}
    for site, r in p.items():
        envelope[site] = (binade(min(r["num_min"], r["den_min"]), False), binade(max(r["num_max"], r["den_max"]), True))
    print("operand envelope in whole binades (2^lo .. 2^hi):", envelope)
    c1, c2, lg, gp, m0, m1 = (p[s] for s in LS.DIV_SITES)
    # the content itself: |x| of cbrt_poly above 1000 (fy of a grey +1024 is 1024)
    fy = max(float(np.max(ref.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722]))) for _, ref, _ in WC.working_set())
    assert fy > 1000.0
    # cbrt_poly, 8-bit: "numerators and denominators in (0.005, 3.5)", every denominator positive
    assert c1["num_max"] > 2.0 ** 70 and c1["den_max"] > 2.0 ** 50 and c2["den_max"] > 2.0 ** 50
    assert 0.0 < c2["den_min"] < 2.0 ** -16 and c2["den_zero"] == 0  # the second step's own two zeros (lab_crossing_step2_*)
    # lab_crossing holds EVERY float32 around the zero of the first denominator, so this is the smallest magnitude that
    # denominator takes at all: it steps over zero (no x makes it 0), down from >= 0.016 = 2^-6 on 8-bit input
    assert 0.0 < c1["den_min"] <= 2.0 ** -20 and c1["den_zero"] == 0
    assert int(c1["signs"]) & 8 and int(c2["signs"]) & 8 and int(c1["signs"]) & 2
    assert before[LS.DIV_SITES[0]]["den_min"] > 2.0 ** -10  # ... which is lab_crossing's doing
    assert c1["quot_max"] > 2.0 ** 20
    # gamma(p) / p, 8-bit: "p >= 1e-4, gamma in [21, ~150]"
    assert gp["num_max"] > 150.0 and gp["den_max"] > 2.0 ** 20 and gp["den_min"] == float(np.float32(1e-4)) and gp["quot_min"] < 2.0 ** -10
    assert int(gp["signs"]) == 5  # both positive: the clamp holds
    # Malta, 8-bit: "b = norm1 + |..| in [5, 2^28]"
    for m in (m0, m1):
        assert m["den_max"] > 2.0 ** 28 and m["quot_min"] < 2.0 ** -28 and int(m["signs"]) == 5
    # fast_log2f's quotient does not depend on the content's range: the mantissa reduction keeps yq in one binade pair
    assert 0.5 <= lg["den_min"] and lg["den_max"] < 2.0 and lg["num_max"] < 1.0
    # nothing reaches the ends of the format, where the expansion without range scaling would differ from a / b
    for site, r in p.items():
        assert r["num_subnormal"] == 0 and r["den_subnormal"] == 0 and r["quot_subnormal"] == 0, site
        assert r["den_max"] < 2.0 ** 126 and r["num_max"] < 2.0 ** 126 and r["quot_max"] < 2.0 ** 126, site
    # the device's division sweep covers what was measured (include/ce_metrics_debug.h: ce_debug_div_sweep)
    lo = min(e[0] for e in envelope.values())
    hi = max(e[1] for e in envelope.values())
    sweep_lo, sweep_hi = sweep_exponents()
    print(f"k_div_sweep draws operands from [2^{sweep_lo}, 2^{sweep_hi})")
    assert sweep_lo <= min(lo, -40) and max(hi, 40) <= sweep_hi, (lo, hi)  # and the range it has always covered


def sweep_exponents():
    """[2^lo, 2^hi): the operand range of the device's division sweep, from the kernel's own constants."""
    text = open(os.path.join(os.path.dirname(GOLD), os.pardir, "codec-eval_amd", "csrc", "butteraugli.hip")).read()
    first = int(re.search(r"DIV_SWEEP_EXP_FIRST = (\d+)u", text).group(1))
    span = int(re.search(r"DIV_SWEEP_EXP_SPAN = (\d+)u", text).group(1))
    return first - 127, first - 127 + span


def test_c_the_device_switches_are_worth_nothing_here(shim):
    """Each of the two switches alone, on every case at every intensity: below the adoption bar, and the rows are the
    ledger's (tests/golden/sensitivity.json, cases "wide:*")."""
    ledger = json.load(open(os.path.join(GOLD, "sensitivity.json")))
    worst = {k: 0.0 for k in SWITCHES}
    for w, h, cases in all_sets():
        for it in WC.INTENSITIES:
            base = {name: shim.butteraugli(ref, test, w, h, it)[0] for name, ref, test in cases}
            for key, idx in SWITCHES.items():
                shim.set_variant(idx, 1)
                try:
                    got = {name: shim.butteraugli(ref, test, w, h, it)[0] for name, ref, test in cases}
                finally:
                    shim.set_variant(idx, 0)
                for name in base:
                    rel = abs(got[name] - base[name]) / max(abs(base[name]), BA_FLOOR)
                    worst[key] = max(worst[key], rel)
                    assert rel <= ADOPTION_BAR, (key, name, w, h, it, base[name], got[name])
                    row = ledger[key]["cases"][f"wide:{name}:{w}x{h}@{it:g}"]
                    assert row["default"] == base[name] and row["variant"] == got[name], (key, name, row)
            shim.set_device_switches(True)  # and both together, as the device runs
            try:
                for name, ref, test in cases:
                    got = shim.butteraugli(ref, test, w, h, it)[0]
                    assert abs(got - base[name]) <= ADOPTION_BAR * max(abs(base[name]), BA_FLOOR), (name, w, h, it, base[name], got)
            finally:
                shim.set_device_switches(False)
    print("worst relative move on wide content:", worst)
    for key in SWITCHES:
        assert ledger[key]["max_rel"] >= worst[key]
