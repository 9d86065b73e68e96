"""The device code of the CICP ingest and of the linear-f32 upload (codec-eval_amd/csrc/cicp_kernel.h) compiled for the
host with -ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/cicp_kernel_host.cpp): the same text the
GPU runs, every thread of every block in turn, on a source, a table and a slab allocated at exactly their size, the image
written into slot 0, 1 or 2 of the slab (slot k starts k * w * h * 12 bytes in, so the store width changes with it).  Its
output must equal the numpy restatement bit for bit, the other slots must stay untouched, and the sanitizers must see no
access outside the buffers and no misaligned wide access.  Covers what a device run cannot show: an out-of-bounds access
that happens to land in mapped memory."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (3, 5), (7, 2), (16, 1), (17, 9), (100, 76))
FORMATS = {0: (np.uint8, 3), 1: (np.uint8, 4), 4: (np.uint16, 3), 5: (np.uint16, 4)}  # CE_PIXEL_*: sample type, channels
WHITE = 203.0


def cases():
    out, n = [], 0
    for fmt in FORMATS:
        for depth in ((8,) if fmt < 2 else R.DEPTHS):
            for prim in R.PRIMARIES:
                for tr in R.TRANSFERS:
                    for w, h in SHAPES:
                        out.append(dict(fmt=fmt, depth=depth, prim=prim, tr=tr, n_px=w * h, slot=n % 3, off=(0, 4, 8, 16)[n % 4], seed=100 + n))
                        n += 1
    for w, h in SHAPES:  # the f32 upload
        for slot in (0, 1, 2):
            out.append(dict(fmt=7, depth=0, prim=1, tr=8, n_px=w * h, slot=slot, off=(0, 4)[slot % 2], seed=9000 + n))
            n += 1
    return out


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cicphost") / "cicp_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "cicp_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    tables, offsets, pos = [], {}, 0
    for tr in R.TRANSFERS:
        for depth in R.DEPTHS:
            t = R.transfer_table(tr, depth, WHITE)
            offsets[(tr, depth)] = pos
            tables.append(t)
            pos += t.size
    np.concatenate(tables).tofile(tmp_path / "tables.bin")
    with open(tmp_path / "cases.txt", "w") as f:
        for c in cs:
            m = R.colour_matrix(c["prim"]).reshape(-1).view(np.uint32)
            maxv = (1 << c["depth"]) - 1 if c["depth"] else 0
            f.write(" ".join(str(v) for v in (c["fmt"], c["n_px"], c["slot"], c["off"], c["seed"], maxv, offsets.get((c["tr"], c["depth"]), 0),
                                              int(c["prim"] != 1), *m.tolist())) + "\n")
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
        n_px, slot = c["n_px"], c["slot"]
        if c["fmt"] == 7:
            src = take(n_px * 12).view(np.float32)
            want = R.sanitise(src)
        else:
            dt, nc = FORMATS[c["fmt"]]
            src = take(n_px * nc * np.dtype(dt).itemsize).view(dt).reshape(n_px, nc)
            above += int((src[:, :3].astype(np.int64) > (1 << c["depth"]) - 1).sum())
            want = R.to_linear(src, c["prim"], c["tr"], c["depth"], WHITE)
        slab = take((slot + 2) * n_px * 12)
        got = slab[slot * n_px * 12:(slot + 1) * n_px * 12]
        assert np.array_equal(got, want.reshape(-1).view(np.uint8)), c
        assert np.all(slab[:slot * n_px * 12] == 0xEE) and np.all(slab[(slot + 1) * n_px * 12:] == 0xEE), c
    assert pos == raw.size
    assert above > 1000  # samples above maxv were met (and clamped)
