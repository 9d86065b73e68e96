"""The tensor ingest of include/ce_metrics.h (section "tensors") restated in numpy: the contract the device, the host build
of the kernel and codec_eval_amd.quantise_tensor are held to, bit for bit.

Elements are given as they lie in memory: uint8 / uint16 arrays for the integer dtypes, uint16 BIT PATTERNS for f16 and
bf16 (numpy has no bfloat16), float32 for f32.  Every step is one numpy operation on float32 arrays, so nothing is
evaluated in a wider type on the way."""
import numpy as np

U8, U16, F16, BF16, F32 = 0, 1, 2, 3, 4
NEAREST_EVEN, TRUNCATE = 0, 1
LINEAR_MAX = np.float32(1024.0)
ELEM_BYTES = {U8: 1, U16: 2, F16: 2, BF16: 2, F32: 4}
STORAGE = {U8: np.uint8, U16: np.uint16, F16: np.uint16, BF16: np.uint16, F32: np.float32}


def widen(x, dtype):
    """f32(x), exactly: f16 by numpy's conversion, bf16 as its 16 bits shifted left, f32 as it is"""
    x = np.asarray(x)
    if dtype == F32:
        return x.astype(np.float32, copy=False)
    if dtype == F16:
        return x.astype(np.uint16).view(np.float16).astype(np.float32)
    if dtype == BF16:
        return (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
    raise ValueError("not a float dtype")


def quantise(x, dtype, depth, rule=NEAREST_EVEN):
    """a float dtype into an integer slot of `depth` bits: clamp, one f32 multiply, rint (ties to even) or floor"""
    v = widen(x, dtype)
    m = np.float32((1 << depth) - 1)
    with np.errstate(invalid="ignore"):
        c = np.where(v > np.float32(0), np.minimum(v, np.float32(1)), np.float32(0)).astype(np.float32)  # NaN, -0 -> +0
    p = (c * m).astype(np.float32)
    q = np.rint(p) if rule == NEAREST_EVEN else np.floor(p)
    return q.astype(np.uint8 if depth == 8 else np.uint16)


def linear(x, dtype):
    """a float dtype into a slot of a linear batch: the clamp of a linear image"""
    v = widen(x, dtype)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), np.float32(0), np.clip(v, -LINEAR_MAX, LINEAR_MAX)).astype(np.float32)


def to_slot(x, dtype, slot, depth=8, rule=NEAREST_EVEN):
    """elements -> samples of a slot: "u8" (an RGB8 batch), "u16" (a deep side of `depth`) or "lin" """
    x = np.asarray(x)
    if slot == "lin":
        if dtype in (U8, U16):
            raise ValueError("integer dtypes do not enter a linear batch")
        return linear(x, dtype)
    out_dt = np.uint8 if slot == "u8" else np.uint16
    d = 8 if slot == "u8" else depth
    if dtype == U8:
        if d != 8:
            raise ValueError("u8 needs depth 8")
        return x.astype(out_dt)
    if dtype == U16:
        if slot == "u8":
            raise ValueError("u16 needs a deep side")
        return np.minimum(x, np.uint16((1 << d) - 1)).astype(np.uint16)
    return quantise(x, dtype, d, rule).astype(out_dt)


def gather(mem, base, strides, count, h, w):
    """[count][h][w][3] elements of the flat element array `mem`: element (n, c, y, x) at base + n sn + c sc + y sy + x sx"""
    sn, sc, sy, sx = strides
    n, y, x, c = np.meshgrid(np.arange(count), np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return mem[base + n * sn + c * sc + y * sy + x * sx]


def sample_elements(rng, dtype, extent, lin=False):
    """`extent` test elements as they lie in memory (bit patterns for f16 / bf16): values around [0, 1] with the 8-bit ties, the ends
    and the specials among them; lin: some far beyond the clamp of a linear image"""
    if dtype == U8:
        return rng.integers(0, 256, extent).astype(np.uint8)
    if dtype == U16:
        return rng.integers(0, 65536, extent).astype(np.uint16)
    v = rng.uniform(-0.25, 1.25, extent).astype(np.float32)
    k = rng.integers(0, 255, extent)
    v = np.where(rng.random(extent) < 0.2, ((k + 0.5) / 255.0).astype(np.float32), v)
    if lin:
        v = np.where(rng.random(extent) < 0.3, v * np.float32(3000.0), v)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1e-45, 0.5], np.float32)
    pick = rng.random(extent) < 0.1
    v = np.where(pick, special[rng.integers(0, special.size, extent)], v).astype(np.float32)
    if dtype == F32:
        return v
    if dtype == F16:
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16)
    return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
