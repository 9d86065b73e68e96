"""The device code of the Y'CbCr ingest (codec-eval_amd/csrc/yuv_kernel.h) compiled for the host and run under
AddressSanitizer and UBSan (tests/cpp/yuv_kernel_host.cpp): the same text the GPU runs, every thread of every block in
turn, on planes allocated at exactly the size their rows need and a slot of exactly its size.  Its output must equal the
numpy restatement bit for bit, and the sanitizers must see no access outside a plane or the slot.  Covers what a device
run cannot show: an out-of-bounds load that happens to land in mapped memory."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv_restatement as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the GPU test's shapes but the large one, and those under 8 pixels wide or 2 tall (the per-sample luma route, one row)
SHAPES = [(8, 8), (9, 9), (10, 8), (17, 9), (301, 9), (9, 301), (100, 76), (1, 1), (3, 5), (7, 2), (16, 1)]


def cases():
    out, n = [], 0
    for w, h in SHAPES:
        for sub in range(4):
            for semi in (0, 1):
                for tri in (0, 1):  # 8 bits into u8: odd pitches and odd slot offsets
                    out.append(dict(w=w, h=h, sub=sub, semi=semi, tri=tri, d=8, msb=0, D=8, out16=0, pad=(0, 1, 7, 64)[n % 4],
                                    off=(0, 1, 4, 8, 3)[n % 5], matrix=n % 3, range_=(n // 3) % 2))
                    n += 1
            for d in (10, 12):
                for msb in (0, 1):
                    for D, out16 in ((8, 0), (d, 1), (16, 1)):
                        out.append(dict(w=w, h=h, sub=sub, semi=n % 2, tri=(n // 2) % 2, d=d, msb=msb, D=D, out16=out16,
                                        pad=(0, 2, 64)[n % 3], off=(0, 2, 4, 16, 6)[n % 5] if out16 else (0, 1, 4, 8, 3)[n % 5],
                                        matrix=n % 3, range_=(n // 3) % 2))
                        n += 1
            out.append(dict(w=w, h=h, sub=sub, semi=n % 2, tri=1, d=8, msb=0, D=10, out16=1, pad=0, off=(0, 2, 4, 16)[n % 4],
                            matrix=0, range_=0))  # 8-bit planes into a deep slot
            n += 1
    return out


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("yuvhost") / "yuv_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "yuv_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    with open(tmp_path / "cases.txt", "w") as f:
        for i, c in enumerate(cs):
            k = Y.coefficients(c["matrix"], c["range_"], c["d"], c["D"])
            f.write(" ".join(str(v) for v in (c["w"], c["h"], c["sub"], c["semi"], c["tri"], c["d"], c["msb"], c["D"], c["out16"], c["pad"],
                                              c["off"], 1000 + i, *k)) + "\n")
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout) == len(cs)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos = 0

    def take(rows, cols, dt):
        nonlocal pos
        n = rows * cols * np.dtype(dt).itemsize
        a = raw[pos:pos + n].view(dt).reshape(rows, cols)
        pos += n
        return a

    for c in cs:
        w, h, sub = c["w"], c["h"], c["sub"]
        dt = np.uint8 if c["d"] == 8 else np.uint16
        cw, ch = Y.chroma_size(w, h, sub)
        y, cb, cr = take(h, w, dt), None, None
        if sub != Y.SUB_400:
            if c["semi"]:
                uv = take(ch, 2 * cw, dt)
                cb, cr = uv[:, 0::2], uv[:, 1::2]
            else:
                cb, cr = take(ch, cw, dt), take(ch, cw, dt)
        got = take(h, w * 3, np.uint16 if c["out16"] else np.uint8).reshape(h, w, 3)
        want = Y.yuv_to_rgb(y, cb, cr, w, h, sub, c["matrix"], c["range_"], c["tri"], c["d"], c["D"], bool(c["msb"]))
        assert np.array_equal(got, want), c
    assert pos == raw.size
