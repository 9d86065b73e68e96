"""CPU checks of the image heuristics (crates/codec-compare/src/image_heuristics.rs): the numpy restatement against
answers derived by hand, the CSV writer and build-predictor's reader, the ABI of ce_image_heuristics, and the argument
checks that need no device."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import heuristics_restatement as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = importlib.import_module("codec-eval_amd.reports")
F = np.float32


def _solid(w, h, rgb):
    return np.broadcast_to(np.array(rgb, np.uint8), (h, w, 3)).copy()


def _gray(v):
    return H.gray_of(np.array([[[v, v, v]]], np.uint8))[0, 0]


@pytest.mark.parametrize("mode", H.MODES)
def test_flat_image(mode):
    # gray(0, 122, 249) is exactly 100.0, so every sum of it is exact in f32 too: the sequential block and image means
    # are exactly 100 and the variances exactly 0 (a gray with more mantissa bits leaves the sequential means a rounding
    # off, and the variances a little above 0, in the reference as in the restatement)
    assert H.gray_of(np.array([[[0, 122, 249]]], np.uint8))[0, 0] == F(100.0)
    o = H.compute(_solid(16, 16, (0, 122, 249)), 16, 16, mode)
    assert o["luminance_variance"] == 0 and o["luminance_std"] == 0 and o["color_variance"] == 0
    assert o["flat_block_pct"] == 100 and o["low_var_block_pct"] == 100 and o["block_variance_mean"] == 0
    assert o["mid_var_block_pct"] == o["high_var_block_pct"] == o["detail_block_pct"] == o["analyze_detail_block_pct"] == 0
    assert o["low_freq_energy"] == 1 and o["high_freq_energy"] == 0 and o["freq_ratio"] == 0
    assert o["edge_strength_max"] == 0 and o["edge_density"] == 0 and o["local_contrast_mean"] == 0
    assert o["horizontal_complexity"] == o["vertical_complexity"] == o["diagonal_complexity"] == 0
    assert o["mean_luminance"] == F(100.0) and o["block_variance_std"] == 0
    assert o["saturation_mean"] == 1 and o["saturation_std"] == 0
    assert (o["width"], o["height"], o["pixels"]) == (16, 16, 256)


def test_vertical_step():
    """Columns 0-7 black, 8-15 at gray G = gray(200, 200, 200): only columns 7 and 8 see the step."""
    w, h = 16, 12
    img = np.zeros((h, w, 3), np.uint8)
    img[:, 8:] = 200
    G = _gray(200)
    o = H.compute(img, w, h)
    inner = F((w - 2) * (h - 2))
    two_cols = F(2 * (h - 2) * float(G))  # exact in f64: 20 copies of one f32
    assert o["edge_strength_max"] == G
    assert o["edge_density"] == F(2 * (h - 2)) / inner
    assert o["edge_strength_mean"] == two_cols / inner
    assert o["horizontal_complexity"] == o["diagonal_complexity"] == o["local_contrast_mean"] == two_cols / inner
    assert o["vertical_complexity"] == 0
    assert o["high_freq_energy"] == F(h) / F((w - 1) * h)
    assert o["low_freq_energy"] == F((w - 2) * h) / F((w - 1) * h)
    assert o["freq_ratio"] == o["high_freq_energy"] / o["low_freq_energy"]
    assert o["flat_block_pct"] == 100 and o["block_variance_mean"] == 0  # the step is on a block edge


def test_one_pixel_checkerboard():
    w = h = 16
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.where(((xx + yy) & 1)[..., None] == 1, np.uint8(255), np.uint8(0)).repeat(3, axis=2)
    G = _gray(255)
    o = H.compute(img, w, h)
    # every neighbour two apart (and diagonal) has the same colour: no gradient, no edge, no complexity
    assert o["edge_strength_max"] == 0 and o["edge_density"] == 0
    assert o["horizontal_complexity"] == o["vertical_complexity"] == o["diagonal_complexity"] == 0
    # every adjacent pair differs by G: all transitions high, none low, so freq_ratio is high_freq_energy itself
    assert o["high_freq_energy"] == 1 and o["low_freq_energy"] == 0 and o["freq_ratio"] == 1
    assert o["local_contrast_mean"] == G and o["local_contrast_std"] == 0
    # a block is 32 x G and 32 x 0: variance (G / 2)^2, far above 5000
    assert np.isclose(o["block_variance_mean"], (float(G) / 2) ** 2, rtol=1e-6)
    assert o["detail_block_pct"] == 100 and o["analyze_detail_block_pct"] == 100 and o["flat_block_pct"] == 0


def test_saturation_of_pure_and_black_colours():
    """Columns of pure red, black (max = 0: the else branch), white and pure dark blue: 1, 0, 0, 1."""
    img = np.zeros((8, 8, 3), np.uint8)
    img[:, 0:2] = (255, 0, 0)
    img[:, 4:6] = (255, 255, 255)
    img[:, 6:8] = (0, 0, 128)
    with np.errstate(all="raise"):
        for mode in H.MODES:
            o = H.compute(img, 8, 8, mode)
            assert o["saturation_mean"] == F(0.5) and o["saturation_std"] == F(0.5)


def test_seven_by_seven_has_no_blocks():
    o = H.compute(np.random.default_rng(1).integers(0, 256, (7, 7, 3), dtype=np.uint8), 7, 7)
    for f in ("flat_block_pct", "low_var_block_pct", "mid_var_block_pct", "high_var_block_pct", "detail_block_pct",
              "analyze_detail_block_pct", "block_variance_mean", "block_variance_std"):
        assert o[f] == 0, f
    assert H.block_variances(H.gray_of(np.zeros((7, 9, 3), np.uint8))).size == 0
    with pytest.raises(ValueError):
        H.compute(np.zeros((2, 7, 3), np.uint8), 7, 2)


def test_accumulation_modes():
    """seq_f32 is one f32 accumulator in order (2^24 + 1 + 1 stays 2^24); f64 rounds the sum once."""
    t = np.array([2.0 ** 24, 1.0, 1.0], np.float32)
    assert H._sum(t, "seq_f32") == F(2.0 ** 24)
    assert H._sum(t, "f64") == F(2.0 ** 24 + 2)
    img = np.random.default_rng(2).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    a, s = H.compute(img, 96, 64, "f64"), H.compute(img, 96, 64, "seq_f32")
    assert all(a[f] == s[f] for f in H.TIER_A)


# ---- CSV ----------------------------------------------------------------------------------------------------------
HEADER = ("image,width,height,pixels,mean_luminance,luminance_variance,luminance_std,edge_strength_mean,edge_strength_max,"
          "edge_density,flat_block_pct,low_var_block_pct,mid_var_block_pct,high_var_block_pct,detail_block_pct,"
          "block_variance_mean,block_variance_std,color_variance,saturation_mean,saturation_std,high_freq_energy,"
          "low_freq_energy,freq_ratio,local_contrast_mean,local_contrast_std,horizontal_complexity,vertical_complexity,"
          "diagonal_complexity")


def _row(image, **kw):
    import codec_eval_amd as ce

    vals = {f: 0.0 for f in ce.HEURISTICS_FIELDS}
    vals.update(width=3, height=4, pixels=12)
    vals.update({k: float(F(v)) if isinstance(v, float) else v for k, v in kw.items()})
    return ce.ImageHeuristics(image, **vals)


def test_heuristics_csv_is_the_references_bytes():
    # Exact binary ties at {:.2}: 0.125 -> 0.12, 0.375 -> 0.38 (to even), the rule reports._fixed already assumes for
    # Rust's float formatting.  There is no Rust toolchain to confirm it against here.
    # The other values: f32(1.005) = 1.00499999523..., f32(1234.5678) = 1234.5677490234375, f32(0.41576192) =
    # 0.41576191782...; 0.03125 is a tie at {:.4}.
    rows = [_row("a.png", mean_luminance=0.125, luminance_variance=0.375, luminance_std=2.5, edge_strength_mean=1.005,
                 edge_strength_max=255.0, edge_density=0.03125, flat_block_pct=100.0, saturation_mean=0.41576192,
                 freq_ratio=float("nan"), diagonal_complexity=1234.5678),
            _row("b c.jpg", width=768, height=512, pixels=393216, high_freq_energy=0.0625, low_freq_energy=0.9375)]
    got = R.heuristics_csv(rows)
    assert got == (
        HEADER + "\n"
        "a.png,3,4,12,0.12,0.38,2.50,1.00,255.00,0.0312,100.00,0.00,0.00,0.00,0.00,0.00,0.00,0.00,0.4158,0.0000,0.0000,"
        "0.0000,NaN,0.00,0.00,0.00,0.00,1234.57\n"
        "b c.jpg,768,512,393216,0.00,0.00,0.00,0.00,0.00,0.0000,0.00,0.00,0.00,0.00,0.00,0.00,0.00,0.00,0.0000,0.0000,"
        "0.0625,0.9375,0.0000,0.00,0.00,0.00,0.00,0.00\n")
    assert R.HEURISTICS_CSV_HEADER == HEADER.split(",")


def test_cpp_heuristics_csv_matches_the_python_one(tmp_path):
    exe = str(tmp_path / "test_heuristics_csv")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "codec-eval_amd", "host"),
                           os.path.join(ROOT, "tests", "cpp", "test_heuristics_csv.cpp"), "-o", exe])
    rows = [_row("a.png", mean_luminance=0.125, luminance_variance=0.375, luminance_std=2.5, edge_strength_mean=1.005,
                 edge_strength_max=255.0, edge_density=0.03125, flat_block_pct=100.0, saturation_mean=0.41576192,
                 freq_ratio=float("nan"), diagonal_complexity=1234.5678),
            _row("b c.jpg", width=768, height=512, pixels=393216, high_freq_energy=0.0625, low_freq_energy=0.9375)]
    assert subprocess.check_output([exe], text=True) == R.heuristics_csv(rows)


def test_read_heuristics_csv_takes_build_predictors_columns(tmp_path):
    rows = [_row("x.png", luminance_std=6.0, edge_strength_mean=7.0, edge_density=0.25, flat_block_pct=10.0,
                 detail_block_pct=14.0, block_variance_mean=15.0, saturation_mean=0.5, high_freq_energy=0.125,
                 freq_ratio=0.375, local_contrast_mean=23.0, luminance_variance=99.0, mid_var_block_pct=98.0),
            _row("y.png", luminance_std=1.0),
            _row("x.png", luminance_std=2.0)]  # a later row of the same image replaces the earlier one (HashMap::insert)
    text = R.heuristics_csv(rows[:2])
    got = R.read_heuristics_csv(text)
    x = got["x.png"]
    assert (x.luminance_std, x.edge_strength_mean, x.edge_density, x.flat_block_pct, x.detail_block_pct, x.block_variance_mean,
            x.saturation_mean, x.high_freq_energy, x.freq_ratio, x.local_contrast_mean) == (
        6.0, 7.0, 0.25, 10.0, 14.0, 15.0, 0.5, 0.125, 0.375, 23.0)
    p = tmp_path / "h.csv"
    p.write_text(R.heuristics_csv(rows))
    got = R.read_heuristics_csv(str(p))
    assert sorted(got) == ["x.png", "y.png"] and got["x.png"].luminance_std == 2.0
    # unparsable cells are 0.0 (`parse().unwrap_or(0.0)`)
    bad = HEADER + "\n" + ",".join(["z.png"] + ["oops"] * 27) + "\n"
    z = R.read_heuristics_csv(bad)["z.png"]
    assert z.luminance_std == 0.0 and z.freq_ratio == 0.0


# ---- ABI ----------------------------------------------------------------------------------------------------------
def _header_fields():
    text = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
    body = re.search(r"typedef struct ce_image_heuristics \{(.*?)\} ce_image_heuristics;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.split(r"[ \*]", f.strip())[-1] for f in body.split(";") if f.strip()]


def test_struct_field_order_matches_everywhere():
    import codec_eval_amd as ce

    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "codec-eval-hip", "src", "sys.rs")).read()
    rust = re.findall(r"pub ([a-z0-9_]+):", re.search(r"pub struct ce_image_heuristics \{(.*?)\}", sys_rs, flags=re.S).group(1))
    fields = _header_fields()
    assert fields == rust == list(ce.HEURISTICS_FIELDS) == [f for f, _ in ce.CeImageHeuristics._fields_]
    # the reference's field order (image_heuristics.rs:22-63) is the CSV's column order after the name
    assert fields[:-1] == R.HEURISTICS_CSV_HEADER[1:]
    assert fields[-1] == "analyze_detail_block_pct"


def test_struct_layout_as_a_c_compiler_sees_it(tmp_path):
    import codec_eval_amd as ce

    fields = _header_fields()
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ce_metrics.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(ce_image_heuristics));\n' +
                   "".join(f'printf("%zu\\n", offsetof(ce_image_heuristics, {f}));\n' for f in fields) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == ctypes.sizeof(ce.CeImageHeuristics) == 128
    assert got[1:] == [getattr(ce.CeImageHeuristics, f).offset for f in fields]


def test_argument_checks_without_a_device(ce):
    out = ce.CeImageHeuristics()
    a = np.zeros(9 * 9 * 3, np.uint8)
    L = ce.lib()
    assert L.ce_image_heuristics_rgb8(None, a.ctypes.data, a.size, 9, 9, ctypes.byref(out)) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_image_heuristics(None, ce.BATCH_REFERENCES, 0, 1, ctypes.byref(out)) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ref_image_heuristics(None, ctypes.byref(out)) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ref_image_heuristics(None, None) == ce.CE_ERR_INVALID_ARG
