"""The device code of the ICC ingest (codec-eval_amd/csrc/icc_kernel.h and cicp_kernel.h around icc_pixel.h's pixel) compiled
for the host with -ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/icc_kernel_host.cpp): the same text
the GPU runs, every thread of every block in turn, on a source, three tone tables, thresholds and a slab allocated at exactly
their size, the image written into slot 0, 1 or 2 of the slab at an offset that changes the store width.  Its output must
equal the numpy restatement bit for bit, the other slots must stay untouched, and the sanitizers must see no access outside
the buffers - the thresholds' entry 0 included - and no misaligned wide access."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (3, 5), (7, 2), (16, 1), (17, 9), (100, 76))
FORMATS = {0: (np.uint8, 3), 1: (np.uint8, 4), 4: (np.uint16, 3), 5: (np.uint16, 4)}  # CE_PIXEL_*: sample type, channels
PROFILES = ("p3", "srgb_curv1024", "mixed_curv", "adobe", "mixed_para", "srgb_para")
# out_kind (0 f32, 1 u8, 2 u16), the slot's depth, the offsets a slab starts at behind a 16-byte boundary
OUTPUTS = ((0, 0, (0, 4, 8, 16)), (1, 8, (0, 1, 2, 4)), (2, 8, (0, 2, 4, 8)), (2, 10, (0, 2, 4, 8)), (2, 12, (0, 2, 4, 8)), (2, 16, (0, 2, 4, 8)))


def cases():
    out, n = [], 0
    for fmt in FORMATS:
        for depth in ((8,) if fmt < 2 else R.DEPTHS):
            for kind, depth_out, offs in OUTPUTS:
                for w, h in SHAPES:
                    out.append(dict(fmt=fmt, depth=depth, n_px=w * h, slot=n % 3, off=offs[(n // 3) % 4], seed=500 + n, kind=kind, depth_out=depth_out,
                                    profile=PROFILES[n % len(PROFILES)]))
                    n += 1
    return out


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("icchost") / "icc_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-fno-strict-aliasing",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "icc_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernels_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    F = R.fixtures()
    blocks, offsets, pos = [], {}, 0

    def put(key, arr):
        nonlocal pos
        if key not in offsets:
            offsets[key] = pos
            blocks.append(np.ascontiguousarray(arr, np.float32).reshape(-1))
            pos += arr.size
        return offsets[key]

    with open(tmp_path / "cases.txt", "w") as f:
        for c in cs:
            p = F[c["profile"]]
            t_at = put((c["profile"], c["depth"]), R.tables(p, c["depth"]))
            thr_at = put(("thr", c["depth_out"]), R.thresholds(c["depth_out"])) if c["kind"] else 0
            m = R.matrix(p).reshape(-1).view(np.uint32)
            f.write(" ".join(str(v) for v in (c["fmt"], c["n_px"], c["slot"], c["off"], c["seed"], (1 << c["depth"]) - 1, t_at, int(R.has_matrix(p)),
                                              c["kind"], c["depth_out"], thr_at, *m.tolist())) + "\n")
    np.concatenate(blocks).tofile(tmp_path / "tables.bin")
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "tables.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout) == len(cs)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos = 0

    def take(nbytes):
        nonlocal pos
        a = raw[pos:pos + nbytes]
        pos += nbytes
        return a

    above = 0
    for c in cs:
        n_px, slot, p = c["n_px"], c["slot"], F[c["profile"]]
        dt, nc = FORMATS[c["fmt"]]
        src = take(n_px * nc * np.dtype(dt).itemsize).view(dt).reshape(n_px, nc)
        above += int((src[:, :3].astype(np.int64) > (1 << c["depth"]) - 1).sum())
        if c["kind"] == 0:
            want = R.to_linear(src, p, c["depth"])
        else:
            want = R.to_srgb(src, p, c["depth"], c["depth_out"], out16=c["kind"] == 2)
        slot_bytes = n_px * 3 * want.dtype.itemsize
        assert want.dtype == (np.float32, np.uint8, np.uint16)[c["kind"]]
        slab = take((slot + 2) * slot_bytes)
        got = slab[slot * slot_bytes:(slot + 1) * slot_bytes]
        assert np.array_equal(got, want.reshape(-1).view(np.uint8)), c
        assert np.all(slab[:slot * slot_bytes] == 0xEE) and np.all(slab[(slot + 1) * slot_bytes:] == 0xEE), c
    assert pos == raw.size
    assert above > 1000  # samples above maxv were met (and clamped)
