"""The device code of the HLG ingest (codec-eval_amd/csrc/cicp_kernel.h and yuv_cicp_kernel.h, with the hlg_pixel.h they run)
compiled for the host with -ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/hlg_kernel_host.cpp, a
stand-alone program): the same text the GPU runs, every thread of every block in turn, on sources, planes, tables and slabs
allocated at exactly their size, the image written into slot 0, 1 or 2 of the slab.  Its output must equal the numpy
restatement (tests/hlg_restatement.py) bit for bit - hlg_pow's f64 sequence included - the other slots must stay untouched,
and the sanitizers must see no access outside the buffers and no misaligned wide access."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import hlg_restatement as H  # noqa: E402
import yuv_linear_cases as L  # noqa: E402
import yuv_restatement as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (3, 5), (7, 2), (16, 1), (17, 9), (100, 76))
FORMATS = {0: (np.uint8, 3), 1: (np.uint8, 4), 4: (np.uint16, 3), 5: (np.uint16, 4)}  # CE_PIXEL_*: sample type, channels


def rgb_cases():
    out, n = [], 0
    for fmt in FORMATS:
        for depth in ((8,) if fmt < 2 else H.DEPTHS):
            for prim in H.PRIMARIES:
                for w, h in SHAPES:
                    out.append(dict(fmt=fmt, depth=depth, prim=prim, n_px=w * h, slot=n % 3, off=(0, 4, 8, 16)[n % 4], seed=100 + n,
                                    zeros=int(n % 5 != 0), display=H.DISPLAYS[(n // 3) % len(H.DISPLAYS)]))
                    n += 1
    return out


def yuv_cases():
    """tests/yuv_linear_cases.py's shapes and option pairs; its transfer option is not read, the display walks H.DISPLAYS"""
    return [dict(c, display=H.DISPLAYS[n % len(H.DISPLAYS)]) for n, c in enumerate(L.cases())]


def pixel_args(prim, display):
    m = R.colour_matrix(prim).reshape(-1).view(np.uint32).tolist()
    p = np.array(H.hlg_params(prim, *display), np.float64).view(np.uint64).tolist()
    return [int(prim != 1), *m, *p]


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hlghost") / "hlg_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "hlg_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernels_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    rgb, yuv = rgb_cases(), yuv_cases()
    offsets, pos = {}, 0
    for depth in H.DEPTHS:
        offsets[depth] = pos
        pos += 1 << depth
    np.concatenate([H.hlg_table(d) for d in H.DEPTHS]).tofile(tmp_path / "tables.bin")
    with open(tmp_path / "cases.txt", "w") as f:
        for c in rgb:
            f.write(" ".join(str(v) for v in ("rgb", c["fmt"], c["n_px"], c["slot"], c["off"], c["seed"], c["zeros"], (1 << c["depth"]) - 1,
                                              offsets[c["depth"]], *pixel_args(c["prim"], c["display"]))) + "\n")
        for n, c in enumerate(yuv):
            (w, h), (d, msb), D = c["shape"], c["sample"], L.c_depth(c)
            k = Y.coefficients(c["matrix"], c["range"], d, D)
            f.write(" ".join(str(v) for v in ("yuv", w, h, c["sub"], c["layout"], c["mode"], d, int(msb), c["pad"] * (1 if d == 8 else 2), c["slot"],
                                              (0, 4, 8, 12)[n % 4], c["seed"], *k, (1 << D) - 1, offsets[D], *pixel_args(c["prim"], c["display"]))) + "\n")
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "tables.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout) == len(rgb) + len(yuv)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos = 0

    def take(nbytes):
        nonlocal pos
        a = raw[pos:pos + nbytes]
        pos += nbytes
        return a

    def check_slab(c, n_px, want):
        slot, n = c["slot"], n_px * 12
        slab = take((slot + 2) * n)
        assert np.array_equal(slab[slot * n:(slot + 1) * n], want.reshape(-1).view(np.uint8)), c
        assert np.all(slab[:slot * n] == 0xEE) and np.all(slab[(slot + 1) * n:] == 0xEE), c

    above = black = 0
    for c in rgb:
        dt, nc = FORMATS[c["fmt"]]
        src = take(c["n_px"] * nc * np.dtype(dt).itemsize).view(dt).reshape(c["n_px"], nc)
        above += int((src[:, :3].astype(np.int64) > (1 << c["depth"]) - 1).sum())
        black += int((src[:, :3] == 0).all(axis=1).sum())
        check_slab(c, c["n_px"], H.to_linear(src, c["prim"], c["depth"], *c["display"]))
    assert above > 1000 and black > 1000  # samples above maxv were met (and clamped), and pixels whose luminance is 0
    above = 0
    for c in yuv:
        (w, h), (d, msb), sub = c["shape"], c["sample"], c["sub"]
        dt = np.uint8 if d == 8 else np.uint16
        bps = np.dtype(dt).itemsize
        cw, ch = Y.chroma_size(w, h, sub)
        y = take(h * w * bps).view(dt).reshape(h, w)
        cb = cr = None
        if sub != Y.SUB_400:
            if c["layout"] == Y.SEMIPLANAR:
                cbcr = take(ch * 2 * cw * bps).view(dt).reshape(ch, 2 * cw)
                cb, cr = cbcr[:, 0::2], cbcr[:, 1::2]
            else:
                cb = take(ch * cw * bps).view(dt).reshape(ch, cw)
                cr = take(ch * cw * bps).view(dt).reshape(ch, cw)
        if not msb:
            above += int((y.astype(np.int64) > (1 << d) - 1).sum())
        want = H.yuv_to_linear(y, cb, cr, w, h, sub, c["matrix"], c["range"], c["mode"], d, msb, c["prim"], L.c_depth(c), *c["display"])
        check_slab(c, w * h, want)
    assert pos == raw.size
    assert above > 1000  # samples above 2^d - 1 were met (and clamped)
