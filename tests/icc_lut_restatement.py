"""LUT-based ICC profiles applied without a CMS (include/ce_metrics.h: ce_icc_lut_*) restated in numpy /
Python floats, with a test-only writer of `mAB `, `mft2` and `mft1` tags.

What the host builds - input tables, CLUT nodes, matrix, curve descriptors, the PCS matrix - is computed per entry in Python
floats (IEEE f64, the host libm's pow for the input side) in the order the header states and rounded once to float32; the
per-pixel part is numpy float32 (float64 inside a power curve), whose products and sums are each rounded separately, as the
device's are.  The power of a post-CLUT curve is hlg_restatement.hlg_pow, the fixed sequence the device runs.  The reader is
written against the ICC.1 layout on its own (struct.unpack of valid profiles only), not against the library's parser."""
import functools
import math
import struct

import numpy as np

import hlg_restatement as H
import icc_restatement as R

TRILINEAR, TETRAHEDRAL = 0, 1
F32 = np.float32
XYZ_SCALE = 1.0 + 32767.0 / 32768.0
D50 = (0xF6D6 / 65536.0, 1.0, 0xD32D / 65536.0)
# the canonical sRGB profile's colorants as a row-major matrix (rows X Y Z)
SRGB_A = [[R.SRGB_COLORANTS[c][r] / 65536.0 for c in range(3)] for r in range(3)]
P3_A = [[R.P3_COLORANTS[c][r] / 65536.0 for c in range(3)] for r in range(3)]


# ---- the writer ------------------------------------------------------------------------------------------------------------------

def _pad4(b: bytes) -> bytes:
    return b + b"\0" * ((-len(b)) % 4)


def _curves(c) -> bytes:
    c = (c,) * 3 if isinstance(c, bytes) else c
    return b"".join(_pad4(x) for x in c)


def clut_bytes(grid, values, precision: int) -> bytes:
    """values: [g0, g1, g2, 3] in [0, 1] -> samples, the first axis slowest"""
    v = np.asarray(values, np.float64).reshape(tuple(grid) + (3,))
    q = np.rint(np.clip(v, 0.0, 1.0) * (65535.0 if precision == 2 else 255.0)).astype(np.int64).reshape(-1)
    return struct.pack(f">{q.size}{'H' if precision == 2 else 'B'}", *q.tolist())


def mab_tag(b, a=None, clut=None, m=None, matrix=None, channels=(3, 3)) -> bytes:
    """b, a, m: one curve element for all channels or three; clut: (grid, values, precision); matrix: 12 floats"""
    body, offs = b"", {}

    def put(name, data):
        nonlocal body
        offs[name] = 32 + len(body)
        body += _pad4(data)

    put("b", _curves(b))
    if clut is not None:
        grid, values, precision = clut
        put("clut", bytes(grid) + b"\0" * 13 + bytes([precision]) + b"\0" * 3 + clut_bytes(grid, values, precision))
    if m is not None:
        put("m", _curves(m))
    if matrix is not None:
        put("matrix", struct.pack(">12i", *(int(round(x * 65536.0)) for x in matrix)))
    if a is not None:
        put("a", _curves(a))
    head = b"mAB \0\0\0\0" + bytes(channels) + b"\0\0" + struct.pack(">5I", offs["b"], offs.get("matrix", 0), offs.get("m", 0), offs.get("clut", 0), offs.get("a", 0))
    return head + body


def mft_tag(wide: bool, in_tables, grid: int, values, out_tables, matrix=(1, 0, 0, 0, 1, 0, 0, 0, 1), channels=(3, 3)) -> bytes:
    """in_tables / out_tables: [3][n] integer samples (u16 for mft2, u8 for mft1); values [g, g, g, 3] in [0, 1]"""
    head = (b"mft2" if wide else b"mft1") + b"\0\0\0\0" + bytes(channels) + bytes([grid, 0]) + struct.pack(">9i", *(int(round(x * 65536.0)) for x in matrix))
    code = "H" if wide else "B"
    if wide:
        head += struct.pack(">HH", len(in_tables[0]), len(out_tables[0]))
    flat = lambda t: struct.pack(f">{3 * len(t[0])}{code}", *[int(v) for ch in t for v in ch])
    return head + flat(in_tables) + clut_bytes((grid,) * 3, values, 2 if wide else 1) + flat(out_tables)


def lut_profile(tag: bytes, pcs: bytes = b"XYZ ", version: int = 4, name: str = "lut", sig: bytes = b"A2B0", extra=(), **kw) -> bytes:
    tags = [(b"desc", R._desc_tag(version, name)), (b"cprt", R._text_tag(version, "no copyright")), (b"wtpt", R.xyz_tag((0xF6D6, 0x10000, 0xD32D))), (sig, tag)]
    return R.write_profile(tags + list(extra), version, pcs=pcs, **kw)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------

def _mat_to_pcs(a3):
    """a row-major RGB -> XYZ matrix as the 12 numbers of an mAB matrix that lands on PCS-encoded XYZ"""
    return [v / XYZ_SCALE for row in a3 for v in row] + [0.0, 0.0, 0.0]


def _lab(xyz):
    f = [(t ** (1.0 / 3.0)) if t > (6.0 / 29.0) ** 3 else t * (841.0 / 108.0) + 4.0 / 29.0 for t in (max(xyz[i], 0.0) / D50[i] for i in range(3))]
    return 116.0 * f[1] - 16.0, 500.0 * (f[0] - f[1]), 200.0 * (f[1] - f[2])


def _grid_rgb(grid):
    ax = [np.linspace(0.0, 1.0, g) for g in grid]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def _lab_clut(grid, legacy: bool):
    """Lab of linear P3 light at the nodes, in the v4 or the legacy 16-bit encoding, as [0, 1] values"""
    rgb = _grid_rgb(grid)
    out = np.empty_like(rgb)
    for idx in np.ndindex(*grid):
        L, a, b = _lab([sum(P3_A[r][c] * rgb[idx][c] for c in range(3)) for r in range(3)])
        out[idx] = (L * 652.8 / 65535.0, (a + 128.0) * 256.0 / 65535.0, (b + 128.0) * 256.0 / 65535.0) if legacy else (L / 100.0, (a + 128.0) / 255.0, (b + 128.0) / 255.0)
    return out


def _xyz_clut(grid):
    """PCS-encoded XYZ of linear P3 light at the nodes"""
    rgb = _grid_rgb(grid)
    return np.einsum("rc,...c->...r", np.array(P3_A), rgb) / XYZ_SCALE


# the XYB colour space of JPEG XL as jpegli's XYB JPEGs code it (public constants of libjxl): the opsin absorbance matrix,
# its bias, and the offsets and scales that bring X, Y, B - Y into [0, 1]
OPSIN = ((0.30, 0.622, 0.078), (0.23, 0.692, 0.078), (0.24342268924547819, 0.20476744424496821, 0.55180986650955360))
OPSIN_BIAS = 0.0037930732552754493
XYB_OFFSET = (0.015386134, 0.0, 0.27770459)
XYB_SCALE = (22.995788804, 1.183000077, 1.502141333)
XYB_LO, XYB_HI = -0.5, 1.5  # the range of the CLUT's outputs, the cube roots minus cbrt(bias)


def xyb_encode(linear_rgb: np.ndarray) -> np.ndarray:
    """linear sRGB [..., 3] float64 -> the scaled XYB samples in [0, 1]"""
    mixed = np.einsum("rc,...c->...r", np.array(OPSIN), np.asarray(linear_rgb, np.float64)) + OPSIN_BIAS
    g = np.cbrt(mixed) - np.cbrt(OPSIN_BIAS)
    x, y, b = (g[..., 0] - g[..., 1]) / 2.0, (g[..., 0] + g[..., 1]) / 2.0, g[..., 2]
    return np.stack([(x + XYB_OFFSET[0]) * XYB_SCALE[0], (y + XYB_OFFSET[1]) * XYB_SCALE[1], (b - y + XYB_OFFSET[2]) * XYB_SCALE[2]], axis=-1)


def xyb_profile() -> bytes:
    """The jpegli XYB profile's shape: identity A, a 2 x 2 x 2 CLUT that undoes the scaling and the X / Y / B mixing, type-2
    para M curves that cube, a 3 x 4 matrix (the inverse opsin matrix, then sRGB's colorants), identity B, PCS XYZ"""
    corners = np.empty((2, 2, 2, 3))
    for idx in np.ndindex(2, 2, 2):
        x, y, bmy = (idx[k] / XYB_SCALE[k] - XYB_OFFSET[k] for k in range(3))
        corners[idx] = [(v - XYB_LO) / (XYB_HI - XYB_LO) for v in (y + x, y - x, bmy + y)]
    cube = R.para_tag(2, (3.0, XYB_HI - XYB_LO, XYB_LO + OPSIN_BIAS ** (1.0 / 3.0), -OPSIN_BIAS))
    to_xyz = np.array(SRGB_A) @ np.linalg.inv(np.array(OPSIN))
    return lut_profile(mab_tag(R.curv_tag(), a=R.curv_tag(), clut=((2, 2, 2), corners, 2), m=cube, matrix=_mat_to_pcs(to_xyz.tolist())), name="XYB")


def _identity_clut(grid):
    return _grid_rgb(grid)


@functools.lru_cache(maxsize=None)
def fixtures() -> dict:
    """name -> profile bytes"""
    g5 = _grid_rgb((5, 5, 5))
    mild = g5 + 0.04 * np.sin(math.pi * g5) * np.roll(g5, 1, axis=-1)  # a mild non-linearity, the corners fixed
    gamma11 = R.para_tag(0, (1.1,))
    mab_xyz = mab_tag(R.curv_tag(), a=R.SRGB_PARA, clut=((5, 5, 5), mild, 2), m=gamma11, matrix=_mat_to_pcs(P3_A))
    gamma22_256 = [[int(round(65535.0 * (i / 255.0) ** 2.2)) for i in range(256)]] * 3
    soft_out = [[0, 16384, 32768, 49151, 65535]] * 3
    mft2_lab = mft_tag(True, gamma22_256, 9, _lab_clut((9, 9, 9), True), soft_out)
    gamma22_u8 = [[int(round(255.0 * (i / 255.0) ** 2.2)) for i in range(256)]] * 3
    ident_u8 = [list(range(256))] * 3
    breaking = R.para_tag(4, (2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.45, 0.02, 0.01))  # its breakpoint inside what the CLUT gives
    return {
        "mab_xyz": lut_profile(mab_xyz, name="mAB XYZ"),
        "mab_xyz_v2": lut_profile(mab_xyz, version=2, name="mAB XYZ v2"),
        "mab_lab": lut_profile(mab_tag(R.curv_tag(), a=R.curv_tag(gamma_u8f8=0x0233), clut=((9, 9, 9), _lab_clut((9, 9, 9), False), 2)), b"Lab ", name="mAB Lab"),
        "mft2_lab": lut_profile(mft2_lab, b"Lab ", 2, "mft2 Lab"),
        "mft2_lab_v4": lut_profile(mft2_lab, b"Lab ", 4, "mft2 Lab v4"),
        "mft2_xyz": lut_profile(mft_tag(True, gamma22_256, 6, _xyz_clut((6, 6, 6)), [[0, 65535]] * 3), b"XYZ ", 2, "mft2 XYZ"),
        "mft1_lab": lut_profile(mft_tag(False, gamma22_u8, 9, _lab_clut((9, 9, 9), False), ident_u8), b"Lab ", 2, "mft1 Lab"),
        "p3_lut": lut_profile(mab_tag(R.curv_tag(), a=R.SRGB_PARA, clut=((2, 2, 2), _identity_clut((2, 2, 2)), 2), m=R.curv_tag(), matrix=_mat_to_pcs(P3_A)),
                              name="P3 as a LUT"),
        "xyb": xyb_profile(),
        "b_only": lut_profile(mab_tag(R.SRGB_PARA), name="B only", profile_class=b"spac"),
        "m_matrix_b": lut_profile(mab_tag((R.curv_tag(samples=(0, 30000, 65535)), R.curv_tag(), R.curv_tag(gamma_u8f8=0x0180)),
                                          m=(breaking, R.para_tag(1, (2.0, 1.2, -0.1)), R.para_tag(2, (1.8, 0.9, 0.05, 0.03))),
                                          matrix=[0.7 / XYZ_SCALE, 0.2 / XYZ_SCALE, 0.05 / XYZ_SCALE, 0.3 / XYZ_SCALE, 0.6 / XYZ_SCALE, 0.1 / XYZ_SCALE, 0.0, 0.1 / XYZ_SCALE,
                                                  0.7 / XYZ_SCALE, 0.01, -0.02, 0.005]), name="M matrix B", profile_class=b"scnr"),
        "grid235": lut_profile(mab_tag(R.curv_tag(gamma_u8f8=0x0120), a=(R.curv_tag(), R.para_tag(0, (1.8,)), R.curv_tag(samples=(0, 20000, 65535))),
                                       clut=((2, 3, 5), _xyz_clut((2, 3, 5)) * 0.9 + 0.02, 1)), name="grid 2 3 5"),
        "all_stages": lut_profile(mab_tag(R.curv_tag(samples=(0, 40000, 65535)), a=R.curv_tag(gamma_u8f8=0x0200), clut=((4, 3, 3), _grid_rgb((4, 3, 3)) ** 1.2, 2),
                                          m=(breaking, breaking, R.para_tag(3, (2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.04045))),
                                          matrix=_mat_to_pcs(SRGB_A)), name="all stages"),
    }


# ---- the reader (valid profiles only) -----------------------------------------------------------------------------------------------

def _read_curve(t: bytes, at: int):
    """-> (curve, bytes used before padding)"""
    if t[at:at + 4] == b"curv":
        n = struct.unpack_from(">I", t, at + 8)[0]
        return ("curv", struct.unpack_from(f">{n}H", t, at + 12), 65535.0), 12 + 2 * n
    assert t[at:at + 4] == b"para"
    ftype = struct.unpack_from(">H", t, at + 8)[0]
    k = (1, 3, 4, 5, 7)[ftype]
    return ("para", ftype, struct.unpack_from(f">{k}i", t, at + 12)), 12 + 4 * k


def _read_curves(t: bytes, at: int):
    out = []
    for _ in range(3):
        c, used = _read_curve(t, at)
        out.append(c)
        at += (used + 3) & ~3
    return out


@functools.lru_cache(maxsize=None)
def read_profile(profile: bytes, intent: int = 0) -> dict:
    """-> {pcs, type, a, clut (grid, [nodes, 3] integer samples, divisor) or None, m, matrix (12 ints) or None, b}; a curve is
    ("curv", samples, divisor) or ("para", ftype, ints); absent curve stages are None"""
    n = struct.unpack_from(">I", profile, 128)[0]
    tags = {}
    for i in range(n):
        sig, off, size = struct.unpack_from(">4sII", profile, 132 + 12 * i)
        tags.setdefault(sig, profile[off:off + size])
    used = b"A2B%d" % intent if b"A2B%d" % intent in tags else b"A2B0"
    t = tags[used]
    out = {"pcs": profile[20:24], "type": t[:4], "tag": used, "a": None, "clut": None, "m": None, "matrix": None, "b": None}
    assert t[8] == 3 and t[9] == 3
    if t[:4] == b"mAB ":
        ob, omat, om, oc, oa = struct.unpack_from(">5I", t, 12)
        out["b"] = _read_curves(t, ob)
        if om:
            out["m"], out["matrix"] = _read_curves(t, om), struct.unpack_from(">12i", t, omat)
        if oa:
            out["a"] = _read_curves(t, oa)
            grid, prec = tuple(t[oc:oc + 3]), t[oc + 16]
            nodes = grid[0] * grid[1] * grid[2]
            out["clut"] = (grid, np.array(struct.unpack_from(f">{3 * nodes}{'H' if prec == 2 else 'B'}", t, oc + 20)).reshape(nodes, 3), 65535.0 if prec == 2 else 255.0)
        return out
    wide = t[:4] == b"mft2"
    assert wide or t[:4] == b"mft1"
    g = t[10]
    n_in, n_out = struct.unpack_from(">HH", t, 48) if wide else (256, 256)
    code, div, at = ("H", 65535.0, 52) if wide else ("B", 255.0, 48)
    size = 2 if wide else 1
    take = lambda cnt, pos: struct.unpack_from(f">{cnt}{code}", t, pos)
    out["a"] = [("curv", take(n_in, at + c * n_in * size), div) for c in range(3)]
    at += 3 * n_in * size
    out["clut"] = ((g, g, g), np.array(take(3 * g ** 3, at)).reshape(g ** 3, 3), div)
    at += 3 * g ** 3 * size
    out["b"] = [("curv", take(n_out, at + c * n_out * size), div) for c in range(3)]
    return out


# ---- what the host builds ---------------------------------------------------------------------------------------------------------

def _input_curve_at(curve, e: float) -> float:
    if curve[0] == "curv" and len(curve[1]) >= 2:
        s, div = curve[1], curve[2]
        p = e * float(len(s) - 1)
        i = min(int(p), len(s) - 2)
        s0, s1 = s[i] / div, s[i + 1] / div
        return s0 + (s1 - s0) * (p - float(i))
    return R.curve_at(curve[:2] if curve[0] == "curv" else curve, e)


@functools.lru_cache(maxsize=None)
def input_tables(profile: bytes, depth: int, intent: int = 0) -> np.ndarray:
    """[3, 2^depth] float32"""
    maxv = (1 << depth) - 1
    a = read_profile(profile, intent)["a"]
    rows = [[R._clip01(v / maxv if a is None else _input_curve_at(a[c], v / maxv)) for v in range(maxv + 1)] for c in range(3)]
    out = np.array(rows, np.float64).astype(F32)
    out.setflags(write=False)
    return out


def clut_nodes(profile: bytes, intent: int = 0):
    """(grid, [nodes, 4] float32 with the fourth 0) or None"""
    c = read_profile(profile, intent)["clut"]
    if c is None:
        return None
    grid, samples, div = c
    out = np.zeros((samples.shape[0], 4), F32)
    out[:, :3] = (samples.astype(np.float64) / div).astype(F32)
    return grid, out


def matrix12(profile: bytes, intent: int = 0) -> np.ndarray:
    m = read_profile(profile, intent)["matrix"]
    if m is None:
        return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F32)
    return (np.array(m, np.float64) / 65536.0).astype(F32)


def curves(profile: bytes, intent: int = 0):
    """the six post-CLUT curves, M then B: ("identity",) | ("sampled", float32 samples) | ("power", ftype, [7 floats])"""
    p = read_profile(profile, intent)
    out = []
    for stage in (p["m"], p["b"]):
        for c in (stage or [("curv", (), 65535.0)] * 3):
            if c[0] == "para":
                out.append(("power", c[1], [v / 65536.0 for v in c[2]] + [0.0] * (7 - len(c[2]))))
            elif len(c[1]) == 0:
                out.append(("identity",))
            elif len(c[1]) == 1:
                out.append(("power", 0, [c[1][0] / 256.0] + [0.0] * 6))
            else:
                out.append(("sampled", (np.array(c[1], np.float64) / c[2]).astype(F32)))
    return out


def pcs_matrix() -> np.ndarray:
    a = [v for row in SRGB_A for v in row]
    return np.array(R._inv3(a), np.float64).astype(F32).reshape(3, 3)


# ---- the definition, per pixel ------------------------------------------------------------------------------------------------------

def icc_pow(base: np.ndarray, g: float) -> np.ndarray:
    """the header's B^g: 0 for B <= 0 or subnormal (0^g by its rule), the range rule on the exponent, else hlg_pow"""
    base = np.ascontiguousarray(base, np.float64)
    zero = ~(base >= 2.2250738585072014e-308)
    safe = np.where(zero, 1.0, base)
    e = ((safe.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    out_of_range = abs(g) * (np.abs(e).astype(np.float64) + 1.0) > 1000.0
    far = np.where(g * (e.astype(np.float64) + 0.5) > 0.0, np.inf, 0.0)
    with np.errstate(all="ignore"):
        p = H.hlg_pow(np.where(out_of_range, 1.0, safe), g)
    at_zero = np.inf if g < 0.0 else (1.0 if g == 0.0 else 0.0)
    return np.where(zero, at_zero, np.where(out_of_range, far, p))


def _clip01(x):
    return np.where(x > 0, np.where(x > 1, x.dtype.type(1), x), x.dtype.type(0))


def power_curve(ftype: int, q, xf: np.ndarray) -> np.ndarray:
    x = xf.astype(np.float64)
    g, a, b, c, d, e, f = (np.float64(v) for v in q)
    if ftype == 0:
        y = icc_pow(x, g)
    else:
        p = icc_pow(a * x + b, g)
        with np.errstate(all="ignore"):
            if ftype == 1:
                y = np.where(x >= -b / a, p, 0.0)
            elif ftype == 2:
                y = np.where(x >= -b / a, p + c, c)
            elif ftype == 3:
                y = np.where(x >= d, p, c * x)
            else:
                y = np.where(x >= d, p + e, c * x + f)
    return _clip01(y).astype(F32)


def curve_on(curve, x: np.ndarray) -> np.ndarray:
    if curve[0] == "identity":
        return x
    xc = _clip01(x)
    if curve[0] == "power":
        return power_curve(curve[1], curve[2], xc)
    s = curve[1]
    n = len(s)
    p = xc * F32(n - 1)
    i = np.minimum(p.astype(np.int64), n - 2)
    s0, s1 = s[i], s[i + 1]
    return s0 + (s1 - s0) * (p - i.astype(F32))


def _axis(a, g):
    p = a * F32(g - 1)
    i = np.minimum(p.astype(np.int64), g - 2)
    return i, p - i.astype(F32)


def _lerp(c0, c1, f):
    return c0 + (c1 - c0) * f


def clut_interpolate(grid, nodes, a: np.ndarray, interpolation: int) -> np.ndarray:
    """a [..., 3] float32 in [0, 1] -> [..., 3] float32"""
    (ix, fx), (iy, fy), (iz, fz) = (_axis(a[..., k], grid[k]) for k in range(3))
    s0, s1 = grid[1] * grid[2], grid[2]
    base = ix * s0 + iy * s1 + iz
    at = lambda off: nodes[base + off][..., :3]
    ex = lambda f: f[..., None]
    if interpolation == TRILINEAR:
        c00, c01 = _lerp(at(0), at(1), ex(fz)), _lerp(at(s1), at(s1 + 1), ex(fz))
        c10, c11 = _lerp(at(s0), at(s0 + 1), ex(fz)), _lerp(at(s0 + s1), at(s0 + s1 + 1), ex(fz))
        return _lerp(_lerp(c00, c01, ex(fy)), _lerp(c10, c11, ex(fy)), ex(fx))
    xy, yz, xz = fx >= fy, fy >= fz, fx >= fz
    # (stride of hi, stride of mid, hi, mid, lo) per case, in the header's order
    cases = [(xy & yz, s0, s1, fx, fy, fz), (xy & ~yz & xz, s0, 1, fx, fz, fy), (xy & ~yz & ~xz, 1, s0, fz, fx, fy),
             (~xy & xz, s1, s0, fy, fx, fz), (~xy & ~xz & yz, s1, 1, fy, fz, fx), (~xy & ~xz & ~yz, 1, s1, fz, fy, fx)]
    sh = np.select([c[0] for c in cases], [c[1] for c in cases])
    sm = np.select([c[0] for c in cases], [c[2] for c in cases])
    hi, mid, lo = (np.select([c[0] for c in cases], [c[k] for c in cases]).astype(F32) for k in (3, 4, 5))
    assert np.all(sum(c[0].astype(int) for c in cases) == 1)
    c000, ca, cb, c111 = at(0), at(sh), at(sh + sm), at(s0 + s1 + 1)
    return ((c000 + (ca - c000) * ex(hi)) + (cb - ca) * ex(mid)) + (c111 - cb) * ex(lo)


def _lab_t(f):
    return np.where(f > F32(6.0 / 29.0), (f * f) * f, (f - F32(4.0 / 29.0)) * F32(108.0 / 841.0))


def to_linear(pixels: np.ndarray, profile: bytes, depth: int, interpolation: int = TRILINEAR, intent: int = 0) -> np.ndarray:
    """[..., 3 or 4] uint8 / uint16 code values -> [..., 3] float32 (alpha dropped): what a linear batch stores"""
    p = read_profile(profile, intent)
    v = np.minimum(np.asarray(pixels)[..., :3].astype(np.int64), (1 << depth) - 1)
    tb = input_tables(profile, depth, intent)
    x = np.stack([tb[c][v[..., c]] for c in range(3)], axis=-1)
    cl = clut_nodes(profile, intent)
    if cl is not None:
        x = clut_interpolate(cl[0], cl[1], x, interpolation)
    cs = curves(profile, intent)
    x = np.stack([curve_on(cs[k], x[..., k]) for k in range(3)], axis=-1)
    if p["matrix"] is not None:
        m = matrix12(profile, intent)
        x = np.stack([((m[3 * i] * x[..., 0] + m[3 * i + 1] * x[..., 1]) + m[3 * i + 2] * x[..., 2]) + m[9 + i] for i in range(3)], axis=-1)
    x = np.stack([curve_on(cs[3 + k], x[..., k]) for k in range(3)], axis=-1)
    assert x.dtype == F32
    if p["pcs"] == b"XYZ ":
        xyz = x * F32(XYZ_SCALE)
    else:
        legacy = p["type"] == b"mft2"
        kl, kab = (F32(65535.0 / 652.8), F32(65535.0 / 256.0)) if legacy else (F32(100.0), F32(255.0))
        L, la, lb = x[..., 0] * kl, x[..., 1] * kab - F32(128.0), x[..., 2] * kab - F32(128.0)
        fy = (L + F32(16.0)) / F32(116.0)
        fx, fz = fy + la / F32(500.0), fy - lb / F32(200.0)
        xyz = np.stack([F32(D50[0]) * _lab_t(fx), _lab_t(fy), F32(D50[2]) * _lab_t(fz)], axis=-1)
    m = pcs_matrix()
    out = np.stack([(m[i, 0] * xyz[..., 0] + m[i, 1] * xyz[..., 1]) + m[i, 2] * xyz[..., 2] for i in range(3)], axis=-1)
    assert out.dtype == F32
    return R.sanitise(out)


def to_srgb(pixels: np.ndarray, profile: bytes, depth: int, depth_out: int = 8, out16=None, interpolation: int = TRILINEAR, intent: int = 0) -> np.ndarray:
    """what an RGB8 batch (depth_out 8, uint8) or a deep side of depth_out bits (uint16) stores"""
    code = R.encode(to_linear(pixels, profile, depth, interpolation, intent), depth_out)
    return code.astype(np.uint16) if (out16 if out16 is not None else depth_out != 8) else code.astype(np.uint8)


# ---- the pixels the tests feed ----------------------------------------------------------------------------------------------------

def edge_pixels(profile: bytes, depth: int, channels: int, dtype, n_px: int, seed: int) -> np.ndarray:
    """[n_px, channels] code values built to hit where the pixel can go wrong, then seeded random ones: maxv on each axis alone
    and together (the last cell with f = 1) and, for 16-bit samples below depth 16, codes above maxv; a grey ramp (every tie of
    the tetrahedral cases); the codes nearest the CLUT's node positions, axis by axis and all together; the six orderings of
    three distinct codes (one pixel inside each tetrahedron) and their two-equal ties.  The list starts `seed` entries in, so
    small images of different seeds see different parts of it."""
    rng = np.random.default_rng(seed)
    maxv = (1 << depth) - 1
    grid = (read_profile(profile)["clut"] or ((4, 4, 4),))[0]
    special = [(maxv, 0, 0), (0, maxv, 0), (0, 0, maxv), (maxv, maxv, maxv), (0, 0, 0), (maxv, maxv, 0)]
    if np.dtype(dtype).itemsize == 2 and depth < 16:
        special += [(maxv + 1, 3, maxv + 7), (65535, 65535, 65535), (5, 65535, maxv)]
    special += [(v, v, v) for v in np.linspace(0, maxv, 17).astype(int)]
    nodes = [[int(round(k * maxv / (g - 1))) for k in range(g)] for g in grid]
    special += [(nodes[0][i % grid[0]], nodes[1][i % grid[1]], nodes[2][i % grid[2]]) for i in range(max(grid))]
    special += [(nodes[0][1], nodes[1][0], nodes[2][grid[2] - 1]), (nodes[0][0], nodes[1][grid[1] - 1], nodes[2][1])]
    lo, mid, hi = maxv // 9 + 1, maxv // 3 + 2, maxv // 2 + 3
    special += [(lo, mid, hi), (lo, hi, mid), (mid, lo, hi), (mid, hi, lo), (hi, lo, mid), (hi, mid, lo)]
    special += [(lo, lo, hi), (hi, lo, lo), (lo, hi, lo), (hi, hi, lo), (lo, hi, hi), (hi, lo, hi)]
    special = np.roll(np.array(special, np.int64), -(seed % len(special)), axis=0)[:n_px]
    out = rng.integers(0, maxv + 1, (n_px, channels))
    out[:len(special), :3] = special
    return np.minimum(out, np.iinfo(dtype).max).astype(dtype)
