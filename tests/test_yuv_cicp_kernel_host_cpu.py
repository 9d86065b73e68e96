"""The device code of the fused Y'CbCr + CICP ingest (codec-eval_amd/csrc/yuv_cicp_kernel.h and the yuv_kernel.h /
cicp_kernel.h it calls) compiled for the host with -ffp-contract=off and run under AddressSanitizer and UBSan
(tests/cpp/yuv_cicp_kernel_host.cpp): the same text the GPU runs, every thread of every block in turn, on planes, a table
and a slab allocated at exactly their size, the image written into slot 0, 1 or 2 of the slab (slot k starts
k * w * h * 12 bytes in and a row y * w * 12 further, so the width of a row's stores changes with both).  Its output must
equal the composed numpy restatement bit for bit, the other slots must stay untouched, and the sanitizers must see no
access outside the buffers and no misaligned wide access.  Covers what a device run cannot show: an out-of-bounds access
that happens to land in mapped memory."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import yuv_linear_cases as L  # noqa: E402
import yuv_restatement as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("yuvcicphost") / "yuv_cicp_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "yuv_cicp_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = L.cases()
    tables, offsets, pos = [], {}, 0
    for tr in R.TRANSFERS:
        for depth in R.DEPTHS:
            t = R.transfer_table(tr, depth, L.WHITE)
            offsets[(tr, depth)] = pos
            tables.append(t)
            pos += t.size
    np.concatenate(tables).tofile(tmp_path / "tables.bin")
    with open(tmp_path / "cases.txt", "w") as f:
        for n, c in enumerate(cs):
            (w, h), (d, msb), D = c["shape"], c["sample"], L.c_depth(c)
            m = R.colour_matrix(c["prim"]).reshape(-1).view(np.uint32)
            k = Y.coefficients(c["matrix"], c["range"], d, D)
            f.write(" ".join(str(v) for v in (w, h, c["sub"], c["layout"], c["mode"], d, int(msb), c["pad"] * (1 if d == 8 else 2), c["slot"],
                                              (0, 4, 8, 12)[n % 4], c["seed"], *k, (1 << D) - 1, offsets[(c["tr"], D)], int(c["prim"] != 1),
                                              *m.tolist())) + "\n")
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
        (w, h), (d, msb), sub, slot = c["shape"], c["sample"], c["sub"], c["slot"]
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
        want = L.want_of(c, (y, cb, cr))
        n = w * h * 12
        slab = take((slot + 2) * n)
        assert np.array_equal(slab[slot * n:(slot + 1) * n], want.reshape(-1).view(np.uint8)), c
        assert np.all(slab[:slot * n] == 0xEE) and np.all(slab[(slot + 1) * n:] == 0xEE), c
    assert pos == raw.size
    assert above > 1000  # samples above 2^d - 1 were met (and clamped)
