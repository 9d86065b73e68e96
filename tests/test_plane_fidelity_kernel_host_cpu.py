"""The device code of the plane-domain scores (codec-eval_amd/csrc/plane_fidelity_kernel.h) compiled for the host with
-ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/plane_fidelity_kernel_host.cpp, a stand-alone program
with its own main; nothing of it is loaded into Python): the same text the GPU runs, every thread of every block of the
launcher's own grids in turn, on planes allocated at exactly their size - pitch padding between rows only, none after the last
row - and tables, pyramid levels and LDS stand-ins sized the same way.  Every integer of every pair must equal the numpy
restatement (tests/plane_fidelity_restatement.py), and the sanitizers must see no access outside the buffers and no misaligned
16-byte load."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_fidelity_restatement as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("planehost") / "plane_fidelity_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "plane_fidelity_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def one(w, h, sub, depth, levels, layouts=(K.PLANAR, K.PLANAR), msb=(False, False), pads=(0, 0)):
    """one pair -> (header fields, [(layout, msb, planes)] references then tests, pair table, wants)"""
    ref, test = K.planes(w, h, sub, depth)
    imgs = [(layouts[k], msb[k], K.host_planes(s, sub, depth, layouts[k], msb[k], pads[k], seed=k)) for k, s in enumerate((ref, test))]
    return (depth, w, h, sub, levels), imgs[:1], imgs[1:], [0], [K.expected(w, h, sub, depth, levels)]


def cases():
    out = []
    for (w, h, sub, layout, depth, msb) in K.FIVE_LEVELS + K.TILE_EDGES:
        out.append(one(w, h, sub, depth, 5, (K.PLANAR, layout), (False, msb), (0, 2 if depth > 8 else 1)))
    for w, h, sub in K.ONE_LEVEL:
        out.append(one(w, h, sub, 8, 1, (K.SEMIPLANAR, K.PLANAR), pads=(3, 0)))
    # the SSE kernel's paths: one sample, a row of one wide piece and a tail, both sample sizes, both layouts, odd pitches
    for w, h in [(1, 1), (17, 9), (33, 31), (100, 76)]:
        for sub in (P.SUB_420, P.SUB_444):
            out.append(one(w, h, sub, 8, 0, (K.PLANAR, K.SEMIPLANAR), pads=(0, 0)))
            out.append(one(w, h, sub, 8, 0, (K.SEMIPLANAR, K.SEMIPLANAR), pads=(1, 15)))
            out.append(one(w, h, sub, 10, 0, (K.SEMIPLANAR, K.PLANAR), (True, False), (2, 0)))
            out.append(one(w, h, sub, 12, 0, (K.SEMIPLANAR, K.SEMIPLANAR), pads=(0, 16)))
    # two references, three pairs, a pair table that is no identity, mixed layouts
    w, h, sub = 176, 163, P.SUB_420
    refs = [(K.PLANAR, False, K.host_planes(K.planes(w, h, sub, 8, s)[0], sub, 8)) for s in (0, 1)]
    tests = [(K.SEMIPLANAR, False, K.host_planes(K.planes(w, h, sub, 8, s)[1], sub, 8, K.SEMIPLANAR, pad=5)) for s in (1, 0, 2)]
    wants = [K.expected(w, h, sub, 8, 5, 1), K.expected(w, h, sub, 8, 5, 0), K.expected(w, h, sub, 8, 5, 2, 1)]
    out.append(((8, w, h, sub, 5), refs, tests, [1, 0, 1], wants))
    return out


def test_host_build_of_the_kernels_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for (depth, w, h, sub, levels), refs, tests, pair_ref, _ in cs:
            words = [depth, w, h, sub, len(refs), len(tests), levels] + pair_ref
            for layout, msb, planes in refs + tests:
                words += [layout, int(msb)] + [K.pitch_of(p) for p in planes]
                for p in planes:  # exactly the plane: the last row ends with its last sample
                    pitch, (rows, row) = K.pitch_of(p), p.shape
                    full = np.lib.stride_tricks.as_strided(p, (rows, pitch), (pitch, 1))[:rows - 1].tobytes() if rows > 1 else b""
                    data.write(full + p[rows - 1].tobytes())
            cfg.write(" ".join(map(str, words)) + "\n")
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(cs)] == f"done {len(cs)}"
    got = np.fromfile(tmp_path / "out.bin", np.int64)
    pos, wide, scalar, tiles = 0, 0, 0, []
    for n, ((depth, w, h, sub, levels), refs, tests, pair_ref, wants) in enumerate(cs):
        f = lines[n].split()
        wide, scalar = wide + int(f[2]), scalar + int(f[3])
        tiles.append(int(f[4]))
        for p, want in enumerate(wants):
            q = got[pos:pos + 33]
            where = (depth, w, h, sub, levels, p)
            assert q[:3].tolist() == want["sse"], (where, "sse", q[:3].tolist(), want["sse"])
            lv = q[3:].reshape(3, 5, 2)
            assert lv[:, :, 0].tolist() == want["ssim_q"], (where, "ssim_q")
            assert lv[:, :, 1].tolist() == want["cs_q"], (where, "cs_q")
            pos += 33
    assert pos == got.size
    assert wide > 500 and scalar > 500, (wide, scalar)  # rows of the calls by the load path they took: both ran
    tiles = [t for t in tiles if t]  # the cases with levels
    assert min(tiles) == 1 and max(tiles) >= 60  # one block, and grids of several rows and columns of tiles
