"""Matrix/TRC ICC profiles applied without a CMS (include/ce_metrics.h: ce_icc_*, ce_batch_set_*_icc, ce_srgb_encode_thresholds)
restated in numpy / Python floats, with a test-only writer of such profiles.

The tone tables, the matrix and the thresholds are built per entry in Python floats (IEEE f64, the host libm's pow - the
function the library's host code calls) in the order the header states and rounded once to float32; the per-pixel part is
numpy float32, whose products and sums are each rounded separately, as the device's are.  The reader below is written against
the ICC.1 layout on its own (struct.unpack of valid profiles only), not against the library's parser."""
import functools
import math
import struct

import numpy as np

LINEAR_MAX = np.float32(1024.0)
DEPTHS = (8, 10, 12, 16)
# the canonical sRGB profile's colorants as s15Fixed16: rXYZ, gXYZ, bXYZ
SRGB_COLORANTS = ((0x6FA2, 0x38F5, 0x0390), (0x6299, 0xB785, 0x18DA), (0x24A0, 0x0F84, 0xB6CF))


# ---- the writer ------------------------------------------------------------------------------------------------------------------

def _s15(x: float) -> int:
    return int(round(x * 65536.0))


def _colorants(r, g, b):
    return tuple(tuple(_s15(v) for v in c) for c in (r, g, b))


P3_COLORANTS = _colorants((0.51512, 0.24120, -0.00105), (0.29198, 0.69225, 0.04189), (0.15710, 0.06657, 0.78407))
ADOBE_COLORANTS = _colorants((0.60974, 0.31111, 0.01947), (0.20528, 0.62567, 0.06087), (0.14919, 0.06322, 0.74457))
PROPHOTO_COLORANTS = _colorants((0.79767, 0.28804, 0.0), (0.13519, 0.71188, 0.0), (0.03134, 0.00009, 0.82491))


def xyz_tag(ints) -> bytes:
    return b"XYZ \0\0\0\0" + struct.pack(">3i", *ints)


def curv_tag(samples=(), gamma_u8f8=None) -> bytes:
    """`curv`: no samples = the identity, gamma_u8f8 = one u8Fixed8 number, else u16 samples."""
    vals = [gamma_u8f8] if gamma_u8f8 is not None else list(samples)
    return b"curv\0\0\0\0" + struct.pack(">I", len(vals)) + struct.pack(f">{len(vals)}H", *vals)


def para_tag(ftype: int, params) -> bytes:
    assert len(params) == (1, 3, 4, 5, 7)[ftype]
    return b"para\0\0\0\0" + struct.pack(">HH", ftype, 0) + struct.pack(f">{len(params)}i", *(_s15(p) for p in params))


def _text_tag(version: int, text: str) -> bytes:
    if version >= 4:
        u = text.encode("utf-16-be")
        return b"mluc\0\0\0\0" + struct.pack(">II", 1, 12) + b"enUS" + struct.pack(">II", len(u), 28) + u
    return b"text\0\0\0\0" + text.encode("ascii") + b"\0"


def _desc_tag(version: int, text: str) -> bytes:
    if version >= 4:
        return _text_tag(version, text)
    a = text.encode("ascii") + b"\0"
    return b"desc\0\0\0\0" + struct.pack(">I", len(a)) + a + b"\0" * (4 + 4 + 2 + 1 + 67)


def write_profile(tags, version: int = 4, colour_space: bytes = b"RGB ", pcs: bytes = b"XYZ ", profile_class: bytes = b"mntr") -> bytes:
    """An ICC profile of `tags` = [(signature, data bytes)], identical data stored once, every element 4-byte aligned."""
    n = len(tags)
    pos = 128 + 4 + 12 * n
    blobs, table, seen = [], [], {}
    for sig, data in tags:
        if data not in seen:
            pad = (-len(data)) % 4
            seen[data] = (pos, len(data))
            blobs.append(data + b"\0" * pad)
            pos += len(data) + pad
        table.append(struct.pack(">4sII", sig, *seen[data]))
    header = struct.pack(">I4sI4s4s4s", pos, b"\0\0\0\0", 0x04300000 if version >= 4 else 0x02400000, profile_class, colour_space, pcs)
    header += struct.pack(">6H", 2024, 1, 1, 0, 0, 0) + b"acsp" + b"\0" * 4 + struct.pack(">I", 0) + b"\0" * 8 + b"\0" * 8
    header += struct.pack(">I", 0) + struct.pack(">3i", 0xF6D6, 0x10000, 0xD32D) + b"\0" * 4 + b"\0" * 16 + b"\0" * 28
    assert len(header) == 128
    return header + struct.pack(">I", n) + b"".join(table) + b"".join(blobs)


def matrix_trc_profile(colorants, curves, version: int = 4, name: str = "test") -> bytes:
    """colorants: three (X, Y, Z) s15Fixed16 triples; curves: one tag's bytes for all channels or three of them."""
    if isinstance(curves, bytes):
        curves = (curves,) * 3
    tags = [(b"desc", _desc_tag(version, name)), (b"cprt", _text_tag(version, "no copyright")), (b"wtpt", xyz_tag((0xF6D6, 0x10000, 0xD32D)))]
    tags += [(s, xyz_tag(c)) for s, c in zip((b"rXYZ", b"gXYZ", b"bXYZ"), colorants)]
    tags += [(s, c) for s, c in zip((b"rTRC", b"gTRC", b"bTRC"), curves)]
    return write_profile(tags, version)


def _srgb_eotf(e: float) -> float:
    return e / 12.92 if e <= 0.04045 else math.pow((e + 0.055) / 1.055, 2.4)


SRGB_PARA = para_tag(3, (2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.04045))


@functools.lru_cache(maxsize=None)
def fixtures() -> dict:
    """name -> profile bytes"""
    srgb_curv = curv_tag(samples=[int(round(65535.0 * _srgb_eotf(i / 1023.0))) for i in range(1024)])
    return {
        "srgb_para": matrix_trc_profile(SRGB_COLORANTS, SRGB_PARA, 4, "sRGB para"),
        "srgb_para_v2": matrix_trc_profile(SRGB_COLORANTS, SRGB_PARA, 2, "sRGB para v2"),
        "srgb_curv1024": matrix_trc_profile(SRGB_COLORANTS, srgb_curv, 2, "sRGB curv"),
        "p3": matrix_trc_profile(P3_COLORANTS, SRGB_PARA, 4, "Display P3"),
        "p3_gamma22": matrix_trc_profile(P3_COLORANTS, curv_tag(gamma_u8f8=0x0233), 2, "P3 gamma 2.2"),
        "adobe": matrix_trc_profile(ADOBE_COLORANTS, curv_tag(gamma_u8f8=563), 2, "Adobe RGB"),
        "prophoto": matrix_trc_profile(PROPHOTO_COLORANTS, curv_tag(gamma_u8f8=461), 4, "ProPhoto"),
        "mixed_para": matrix_trc_profile(P3_COLORANTS, (para_tag(0, (2.2,)), para_tag(1, (2.4, 1.1, -0.05)), para_tag(2, (1.9, 0.9, 0.02, 0.05))), 4, "mixed para"),
        "mixed_curv": matrix_trc_profile(ADOBE_COLORANTS, (para_tag(4, (2.4, 1.0 / 1.055, 0.055 / 1.055, 1.0 / 12.92, 0.04045, 0.001, 0.0005)),
                                                           curv_tag(), curv_tag(samples=(3000, 61000))), 2, "mixed curv"),
    }


# ---- the reader (valid profiles only) -----------------------------------------------------------------------------------------------

def read_profile(profile: bytes) -> dict:
    n = struct.unpack_from(">I", profile, 128)[0]
    tags = {}
    for i in range(n):
        sig, off, size = struct.unpack_from(">4sII", profile, 132 + 12 * i)
        tags.setdefault(sig, profile[off:off + size])
    out = {"colorants": [], "curves": []}
    for s in (b"rXYZ", b"gXYZ", b"bXYZ"):
        assert tags[s][:4] == b"XYZ "
        out["colorants"].append(struct.unpack_from(">3i", tags[s], 8))
    for s in (b"rTRC", b"gTRC", b"bTRC"):
        t = tags[s]
        if t[:4] == b"curv":
            cnt = struct.unpack_from(">I", t, 8)[0]
            out["curves"].append(("curv", struct.unpack_from(f">{cnt}H", t, 12)))
        else:
            assert t[:4] == b"para"
            ftype = struct.unpack_from(">H", t, 8)[0]
            out["curves"].append(("para", ftype, struct.unpack_from(f">{(1, 3, 4, 5, 7)[ftype]}i", t, 12)))
    return out


# ---- the definition -------------------------------------------------------------------------------------------------------------------

def _pow(base: float, g: float) -> float:
    """C's pow on a base taken as 0 when negative: where Python raises - 0 to a negative power, a result past the doubles -
    C returns +inf, which the clip turns into 1"""
    base = base if base > 0.0 else 0.0
    if base == 0.0 and g < 0.0:
        return math.inf
    try:
        return math.pow(base, g)
    except OverflowError:
        return math.inf


def curve_at(curve, e: float) -> float:
    if curve[0] == "curv":
        s = curve[1]
        if len(s) == 0:
            return e
        if len(s) == 1:
            return _pow(e, s[0] / 256.0)
        p = e * float(len(s) - 1)
        i = min(int(p), len(s) - 2)
        s0, s1 = s[i] / 65535.0, s[i + 1] / 65535.0
        return s0 + (s1 - s0) * (p - float(i))
    ftype, q = curve[1], [v / 65536.0 for v in curve[2]] + [0.0] * 7
    g, a, b, c, d, ee, f = q[:7]
    if ftype == 0:
        return _pow(e, g)
    if ftype == 1:
        return _pow(a * e + b, g) if e >= -b / a else 0.0
    if ftype == 2:
        return _pow(a * e + b, g) + c if e >= -b / a else c
    if ftype == 3:
        return _pow(a * e + b, g) if e >= d else c * e
    return _pow(a * e + b, g) + ee if e >= d else c * e + f


def _clip01(y: float) -> float:
    return 0.0 if not y > 0.0 else (1.0 if y > 1.0 else y)


@functools.lru_cache(maxsize=None)
def tables(profile: bytes, depth: int) -> np.ndarray:
    """[3, 2^depth] float32"""
    maxv = (1 << depth) - 1
    curves = read_profile(profile)["curves"]
    out = np.array([[_clip01(curve_at(c, v / maxv)) for v in range(maxv + 1)] for c in curves], np.float64).astype(np.float32)
    out.setflags(write=False)
    return out


def _inv3(a):
    c00 = a[4] * a[8] - a[5] * a[7]
    c01 = a[5] * a[6] - a[3] * a[8]
    c02 = a[3] * a[7] - a[4] * a[6]
    det = (a[0] * c00 + a[1] * c01) + a[2] * c02
    return [c00 / det, (a[2] * a[7] - a[1] * a[8]) / det, (a[1] * a[5] - a[2] * a[4]) / det,
            c01 / det, (a[0] * a[8] - a[2] * a[6]) / det, (a[2] * a[3] - a[0] * a[5]) / det,
            c02 / det, (a[1] * a[6] - a[0] * a[7]) / det, (a[0] * a[4] - a[1] * a[3]) / det]


def matrix(profile: bytes) -> np.ndarray:
    cols = read_profile(profile)["colorants"]
    if tuple(tuple(c) for c in cols) == SRGB_COLORANTS:
        return np.eye(3, dtype=np.float32)
    a = [SRGB_COLORANTS[c][r] / 65536.0 for r in range(3) for c in range(3)]
    p = [cols[c][r] / 65536.0 for r in range(3) for c in range(3)]
    ai = _inv3(a)
    return np.array([[(ai[3 * r] * p[c] + ai[3 * r + 1] * p[3 + c]) + ai[3 * r + 2] * p[6 + c] for c in range(3)] for r in range(3)],
                    np.float64).astype(np.float32)


def has_matrix(profile: bytes) -> bool:
    return not np.array_equal(matrix(profile), np.eye(3, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def thresholds(depth: int) -> np.ndarray:
    """T[1 .. 2^depth - 1] at [0 .. 2^depth - 2], float32"""
    maxv = (1 << depth) - 1
    out = np.array([_srgb_eotf((k - 0.5) / maxv) for k in range(1, maxv + 1)], np.float64).astype(np.float32)
    out.setflags(write=False)
    return out


def sanitise(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a, np.float32)
    return np.where(np.isnan(a), np.float32(0.0), np.clip(a, -LINEAR_MAX, LINEAR_MAX)).astype(np.float32)


def to_linear(pixels: np.ndarray, profile: bytes, depth: int, tone_tables=None) -> np.ndarray:
    """[..., 3 or 4] uint8 / uint16 code values -> [..., 3] float32 (alpha dropped): what a linear batch stores"""
    v = np.minimum(np.asarray(pixels)[..., :3].astype(np.int64), (1 << depth) - 1)
    tb = tables(profile, depth) if tone_tables is None else tone_tables
    t = np.stack([tb[c][v[..., c]] for c in range(3)], axis=-1)
    if not has_matrix(profile):
        return sanitise(t)
    m = matrix(profile)
    r, g, b = t[..., 0], t[..., 1], t[..., 2]
    out = np.stack([(m[i, 0] * r + m[i, 1] * g) + m[i, 2] * b for i in range(3)], axis=-1)
    assert out.dtype == np.float32
    return sanitise(out)


def encode(x: np.ndarray, depth_out: int) -> np.ndarray:
    """#{k : x >= T[k]}, NaN -> 0; uint8 at depth 8, else uint16"""
    x = np.asarray(x, np.float32)
    code = np.searchsorted(thresholds(depth_out), x, side="right")
    code = np.where(np.isnan(x), 0, code)
    return code.astype(np.uint8 if depth_out == 8 else np.uint16)


def to_srgb(pixels: np.ndarray, profile: bytes, depth: int, depth_out: int = 8, out16=None, tone_tables=None) -> np.ndarray:
    """what an RGB8 batch (depth_out 8, uint8) or a deep side of depth_out bits (uint16) stores"""
    code = encode(to_linear(pixels, profile, depth, tone_tables), depth_out)
    return code.astype(np.uint16) if (out16 if out16 is not None else depth_out != 8) else code.astype(np.uint8)
