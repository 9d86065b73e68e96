"""The device code of linear-light compositing (codec-eval_amd/csrc/over_linear_kernel.h: both frames) compiled for the host
with -ffp-contract=off as a stand-alone program and run under AddressSanitizer and UBSan
(tests/cpp/over_linear_kernel_host.cpp): the same text the GPU runs, every thread of every block in turn, on a source, two
tables and a slab allocated at exactly their size, the image written over n_bg backgrounds into slots first .. first + n_bg - 1
(slot k starts k * w * h * 12 bytes in, so the store width changes from slot to slot where w * h is odd).  Every output must
equal the numpy restatement bit for bit, the slots in front must stay untouched, and the sanitizers must see no access outside
the buffers and no misaligned wide access.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alpha_linear_restatement as A  # noqa: E402
import cicp_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGBA8, RGBA16, RGBA_F32 = 1, 5, 8
WHITE = 203.0


def cases():
    out, n = [], 0
    for fmt in (RGBA8, RGBA16):
        for depth in ((8,) if fmt == RGBA8 else A.DEPTHS):
            for prim, tr in A.CICP_PIXELS:
                for w, h in A.SHAPES:
                    out.append(dict(fmt=fmt, depth=depth, prim=prim, tr=tr, n_px=w * h, first=A.FIRST_SLOTS[n % 2], off=(0, 4, 8, 16)[n % 4],
                                    n_bg=A.N_BGS[n % 3], premul=0, seed=500 + n))
                    n += 1
    for premul in (0, 1):
        for w, h in A.SHAPES:
            for n_bg in A.N_BGS:
                out.append(dict(fmt=RGBA_F32, depth=0, prim=1, tr=8, n_px=w * h, first=A.FIRST_SLOTS[n % 2], off=(0, 4)[n % 2], n_bg=n_bg,
                                premul=premul, seed=9000 + n))
                n += 1
    return out


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("overhost") / "over_linear_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-fno-strict-aliasing",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "over_linear_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_both_frames_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    tables, offsets, pos = [], {}, 0
    for tr in R.TRANSFERS:
        for depth in R.DEPTHS:
            t = R.transfer_table(tr, depth, WHITE)
            offsets[(tr, depth)] = pos
            tables.append(t)
            pos += t.size
    for depth in A.DEPTHS:
        t = A.alpha_table(depth)
        offsets[("alpha", depth)] = pos
        tables.append(t)
        pos += t.size
    np.concatenate(tables).tofile(tmp_path / "tables.bin")
    with open(tmp_path / "cases.txt", "w") as f:
        for c in cs:
            m = R.colour_matrix(c["prim"]).reshape(-1).view(np.uint32)
            bg = A.BACKGROUNDS[:c["n_bg"]].reshape(-1).view(np.uint32)
            maxv = (1 << c["depth"]) - 1 if c["depth"] else 0
            f.write(" ".join(str(v) for v in (c["fmt"], c["n_px"], c["first"], c["off"], c["seed"], maxv, offsets.get((c["tr"], c["depth"]), 0),
                                              offsets.get(("alpha", c["depth"]), 0), int(c["prim"] != 1), c["premul"], c["n_bg"],
                                              *m.tolist(), *bg.tolist())) + "\n")
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

    met = dict(zero=0, full=0, above=0, nan=0)
    for c in cs:
        n_px, first, n_bg = c["n_px"], c["first"], c["n_bg"]
        bgs = A.BACKGROUNDS[:n_bg]
        if c["fmt"] == RGBA_F32:
            src = take(n_px * 16).view(np.float32).reshape(n_px, 4)
            met["nan"] += int(np.isnan(src[:, 3]).sum())
            want = A.over_f32(src, bool(c["premul"]), bgs)
        else:
            dt = np.uint8 if c["fmt"] == RGBA8 else np.uint16
            src = take(n_px * 4 * np.dtype(dt).itemsize).view(dt).reshape(n_px, 4)
            m = (1 << c["depth"]) - 1
            met["zero"] += int((src[:, 3] == 0).sum())
            met["full"] += int((src[:, 3] == m).sum())
            met["above"] += int((src[:, 3].astype(np.int64) > m).sum())
            want = A.over_int(R.to_linear(src, c["prim"], c["tr"], c["depth"], WHITE), src[:, 3], c["depth"], bgs)
        slab = take((first + n_bg) * n_px * 12)
        got = slab[first * n_px * 12:]
        assert np.array_equal(got, want.reshape(-1).view(np.uint8)), c
        assert np.all(slab[:first * n_px * 12] == 0xEE), c
    assert pos == raw.size
    assert min(met.values()) > 100, met  # hidden, opaque and above-range alphas and NaN coverage were all met
