"""The tensor ingest's definition (include/ce_metrics.h, section "tensors") on the host: tests/tensor_restatement.py against
live CPU torch - torch.round(x.float().clamp(0, 1) * m) for NEAREST_EVEN, floor for TRUNCATE - on every float16 and every
bfloat16 bit pattern at every slot depth and on float32 at every tie and around both ends; hand-derived values; the package's
quantise_tensor against the restatement; the ctypes struct against the header's layout."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tensor_restatement as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = (8, 10, 12, 16)
ALL16 = np.arange(65536, dtype=np.uint32).astype(np.uint16)


def torch_rule(x32: torch.Tensor, depth: int, rule: int) -> np.ndarray:
    p = x32.clamp(0, 1) * float((1 << depth) - 1)
    with np.errstate(invalid="ignore"):  # NaN rows are compared by the caller, not through this cast
        return (torch.round(p) if rule == T.NEAREST_EVEN else torch.floor(p)).numpy().astype(np.int64)


@pytest.mark.parametrize("dtype,tdtype", [(T.F16, torch.float16), (T.BF16, torch.bfloat16)])
def test_every_16_bit_pattern_equals_torch(dtype, tdtype):
    x = torch.from_numpy(ALL16.view(np.int16).copy()).view(tdtype)
    x32 = x.float()
    nan = torch.isnan(x32).numpy()
    # the widening is torch's .float(), bit for bit (bf16: on NaN payloads too; f16 conversions may quiet a signalling NaN)
    same = T.widen(ALL16, dtype).view(np.uint32) == x32.numpy().view(np.uint32)
    assert same.all() if dtype == T.BF16 else same[~nan].all()
    assert nan.sum() == {T.F16: 2046, T.BF16: 254}[dtype]
    for depth in DEPTHS:
        for rule in (T.NEAREST_EVEN, T.TRUNCATE):
            got = T.quantise(ALL16, dtype, depth, rule).astype(np.int64)
            assert np.array_equal(got[~nan], torch_rule(x32, depth, rule)[~nan]), (depth, rule)
            assert not got[nan].any(), "NaN quantises to 0"


@pytest.mark.parametrize("depth", (8, 10))
def test_f32_at_every_tie_and_at_the_ends_equals_torch(depth):
    m = (1 << depth) - 1
    ties = ((np.arange(m, dtype=np.float64) + 0.5) / m).astype(np.float32)
    one = np.float32(1)
    ends = np.array([0.0, -0.0, 1.0, np.nextafter(one, np.float32(2)), 1.5, 3e38, np.inf, -np.inf, 1e-45, -1e-45, 1.1754942e-38, -1.0,
                     np.nextafter(one, np.float32(0)), 0.5 / m, np.nextafter(np.float32(0.5 / m), one)], np.float32)
    x = np.concatenate([ties, np.nextafter(ties, np.float32(-1)), np.nextafter(ties, np.float32(2)), ends]).astype(np.float32)
    for rule in (T.NEAREST_EVEN, T.TRUNCATE):
        assert np.array_equal(T.quantise(x, T.F32, depth, rule).astype(np.int64), torch_rule(torch.from_numpy(x), depth, rule)), rule
    assert not T.quantise(np.array([np.nan, -np.nan], np.float32), T.F32, depth).any()
    assert T.quantise(np.array([-0.0], np.float32), T.F32, depth)[0] == 0 and T.quantise(np.array([np.inf], np.float32), T.F32, depth)[0] == m


def test_hand_derived_values():
    q = lambda v, rule=T.NEAREST_EVEN, depth=8: int(T.quantise(np.array([v], np.float32), T.F32, depth, rule)[0])
    assert q(0.5) == 128  # 0.5 * 255 = 127.5 exactly: the tie goes to the even 128
    assert q(0.5, T.TRUNCATE) == 127
    # 2.5 / 255 is not a float32: what decides is the f32 product of the rounded quotient with 255, computed here in exact
    # arithmetic (a float32 times 255 fits a double), rounded once to f32 as the definition's one multiply is
    x = np.float32(2.5 / 255)
    p = np.float32(np.float64(x) * 255.0)
    assert q(x) == (2 if p <= np.float32(2.5) else 3) and q(x) in (2, 3)
    assert q(x, T.TRUNCATE) == 2
    assert q(1.5 / 255) in (1, 2) and q(3.5 / 255) in (3, 4)
    assert q(1.0) == 255 and q(1.0, depth=16) == 65535 and q(2.0) == 255 and q(-1.0) == 0
    assert q(0.999, T.TRUNCATE) == 254 and q(0.999) == 255
    # bf16: the bits shifted left; 0x3F00 is 0.5, 0x3F80 is 1.0
    assert T.quantise(np.array([0x3F00, 0x3F80, 0x7FC0, 0x8000], np.uint16), T.BF16, 8).tolist() == [128, 255, 0, 0]
    # f16: 0x3800 is 0.5, 0x3C00 is 1.0, 0x0001 the smallest subnormal
    assert T.quantise(np.array([0x3800, 0x3C00, 0x7E00, 0x0001], np.uint16), T.F16, 10).tolist() == [512, 1023, 0, 0]
    # integer dtypes and the linear clamp
    assert T.to_slot(np.array([0, 1023, 1024, 65535], np.uint16), T.U16, "u16", 10).tolist() == [0, 1023, 1023, 1023]
    assert T.to_slot(np.array([0, 255], np.uint8), T.U8, "u16", 8).dtype == np.uint16
    lin = T.linear(np.array([np.nan, 2000.0, -2000.0, -0.0, 0.25], np.float32), T.F32)
    assert lin.view(np.uint32).tolist() == np.array([0.0, 1024.0, -1024.0, -0.0, 0.25], np.float32).view(np.uint32).tolist()


def test_quantise_tensor_equals_the_restatement(ce):
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-0.2, 1.2, 4096), (np.arange(255) + 0.5) / 255, [np.nan, np.inf, -0.0, 1.0]]).astype(np.float32)
    for depth in DEPTHS:
        for rule in (ce.QUANT_NEAREST_EVEN, ce.QUANT_TRUNCATE):
            want = T.quantise(x, T.F32, depth, rule)
            got = ce.quantise_tensor(x, depth, rule)
            assert got.dtype == want.dtype and np.array_equal(got, want)
            assert np.array_equal(ce.quantise_tensor(ALL16, depth, rule, dtype=ce.DTYPE_BF16), T.quantise(ALL16, T.BF16, depth, rule))
            assert np.array_equal(ce.quantise_tensor(ALL16.view(np.float16), depth, rule), T.quantise(ALL16, T.F16, depth, rule))
            assert np.array_equal(ce.quantise_tensor(ALL16, depth, rule, dtype=ce.DTYPE_F16), T.quantise(ALL16, T.F16, depth, rule))
    t = torch.from_numpy(ALL16.view(np.int16).copy()).view(torch.bfloat16)
    assert np.array_equal(ce.quantise_tensor(t, 10), T.quantise(ALL16, T.BF16, 10))
    assert (ce.DTYPE_U8, ce.DTYPE_U16, ce.DTYPE_F16, ce.DTYPE_BF16, ce.DTYPE_F32) == (T.U8, T.U16, T.F16, T.BF16, T.F32)
    assert (ce.QUANT_NEAREST_EVEN, ce.QUANT_TRUNCATE) == (T.NEAREST_EVEN, T.TRUNCATE)


def test_from_array_reads_layouts_views_and_torch_tensors(ce):
    a = np.zeros((2, 3, 6, 10), np.float32)
    t = ce.TensorImage.from_array(a, "NCHW")
    assert (t.strides, t.count, t.height, t.width, t.dtype, t.memory) == ((180, 60, 10, 1), 2, 6, 10, ce.DTYPE_F32, ce.MEM_HOST)
    t = ce.TensorImage.from_array(a[0, :, 1:5, 2:9], "CHW", quantise=ce.QUANT_TRUNCATE)
    assert (t.strides, t.count, t.height, t.width, t.quantise) == ((0, 60, 10, 1), 1, 4, 7, ce.QUANT_TRUNCATE)
    assert t.data == a.ctypes.data + (10 + 2) * 4
    rgba = np.zeros((6, 10, 4), np.uint8)
    assert ce.TensorImage.from_array(rgba, "HWC").strides == (0, 1, 40, 4)
    assert ce.TensorImage.from_array(np.zeros((6, 10, 1), np.uint16), "HWC").strides == (0, 0, 10, 1)
    x = torch.zeros((2, 3, 6, 10), dtype=torch.bfloat16)
    t = ce.TensorImage.from_array(x.to(memory_format=torch.channels_last), "NCHW")
    assert (t.strides, t.dtype, t.memory, t.data) == ((180, 1, 30, 3), ce.DTYPE_BF16, ce.MEM_HOST, t.keep.data_ptr())
    assert ce.TensorImage.from_array(x[0].expand(3, 6, 10)[:1].expand(3, 6, 10), "CHW").strides[1] == 0
    assert ce.TensorImage.from_array(torch.zeros((3, 4, 4), dtype=torch.float16), "CHW").dtype == ce.DTYPE_F16
    with pytest.raises(TypeError):
        ce.TensorImage.from_array(np.zeros((3, 4, 4), np.int32), "CHW")
    with pytest.raises(ValueError):
        ce.TensorImage.from_array(np.zeros((2, 4, 4), np.uint8), "CHW")
    assert "torch" not in ce.__dict__, "the package does not import torch"


def test_struct_matches_the_header(ce, tmp_path):
    fields = [f for f, _ in ce.CeTensorImage._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ce_metrics.h"\nint main(void){printf("%zu\\n", sizeof(ce_tensor_image));\n' +
                   "".join(f'printf("%zu\\n", offsetof(ce_tensor_image, {f}));\n' for f in fields) +
                   'printf("%d %d %d %d %d %d %d\\n", CE_DTYPE_U8, CE_DTYPE_U16, CE_DTYPE_F16, CE_DTYPE_BF16, CE_DTYPE_F32, CE_QUANT_NEAREST_EVEN, CE_QUANT_TRUNCATE);\n'
                   "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    import ctypes as C
    assert int(out[0]) == C.sizeof(ce.CeTensorImage) == 56
    assert [int(v) for v in out[1:1 + len(fields)]] == [getattr(ce.CeTensorImage, f).offset for f in fields]
    assert out[1 + len(fields)].split() == [str(v) for v in (ce.DTYPE_U8, ce.DTYPE_U16, ce.DTYPE_F16, ce.DTYPE_BF16, ce.DTYPE_F32, ce.QUANT_NEAREST_EVEN,
                                                               ce.QUANT_TRUNCATE)]
    assert fields == ["data", "stride_n", "stride_c", "stride_y", "stride_x", "dtype", "memory", "quantise"]
