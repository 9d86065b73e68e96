"""The device code of VIFp (codec-eval_amd/csrc/plane_vif_kernel.h) compiled for the host with -ffp-contract=off and run under
AddressSanitizer and UBSan (tests/cpp/plane_vif_kernel_host.cpp, a stand-alone program with its own main; nothing of it is
loaded into Python): the same text the GPU runs, every thread of every block of the launcher's own grids in turn and phase by
phase, on planes and a pyramid allocated at exactly their size - pitch padding between rows only, none after the last row -
with LDS stand-ins sized the same way.  Every sum of every pair must equal the numpy restatement
(tests/plane_vif_restatement.py), and the sanitizers must see no access outside the buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_vif_cases as VK  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("vifhost") / "plane_vif_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "plane_vif_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def cases():
    """-> [((depth, w, h, sub), references, tests, pair table, wants)], an image as (layout, msb, planes)"""
    out = []
    for n, (w, h, sub, depth, layout, msb) in enumerate(VK.SHAPES):
        ref, test = VK.planes(w, h, sub, depth)
        pad = (1, 3)[n % 2] * (1 if depth == 8 else 2)  # odd pitches where the samples are bytes
        refs = [(K.PLANAR, False, K.host_planes(ref, sub, depth, K.PLANAR, False, 0))]
        tests = [(layout, msb, K.host_planes(test, sub, depth, layout, msb, pad, seed=n))]
        out.append(((depth, w, h, sub), refs, tests, [0], [VK.expected(w, h, sub, depth)]))
    # three references of which one is not named, three pairs, a pair table that is no identity, mixed layouts
    w, h, sub = 82, 82, VK.V.SUB_420
    refs = [(K.SEMIPLANAR, False, K.host_planes(VK.planes(w, h, sub, 8, s)[0], sub, 8, K.SEMIPLANAR, pad=5)) for s in (0, 3, 1)]
    tests = [(K.PLANAR, False, K.host_planes(VK.planes(w, h, sub, 8, s)[1], sub, 8, pad=1)) for s in (1, 0, 2)]
    wants = [VK.expected(w, h, sub, 8, 1), VK.expected(w, h, sub, 8, 0), VK.expected(w, h, sub, 8, 2, 1)]
    out.append(((8, w, h, sub), refs, tests, [2, 0, 2], wants))
    return out


def test_host_build_of_the_kernels_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for (depth, w, h, sub), refs, tests, pair_ref, _ in cs:
            words = [depth, w, h, sub, len(refs), len(tests)] + pair_ref
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
    got = np.fromfile(tmp_path / "out.bin", np.uint64)
    pos, scale1_blocks, dead, idle = 0, [], 0, 0
    for n, ((depth, w, h, sub), refs, tests, pair_ref, wants) in enumerate(cs):
        f = lines[n].split()
        scale1_blocks.append(int(f[2]))
        dead, idle = dead + int(f[3]), idle + int(f[4])
        for i, want in enumerate(wants):
            q = got[pos:pos + 24].reshape(3, 4, 2)
            for p in range(3):
                assert [int(v) for v in q[p, :, 0]] == want["num_q"][p], ((depth, w, h, sub, i), "num_q", p, q[p, :, 0], want["num_q"][p])
                assert [int(v) for v in q[p, :, 1]] == want["den_q"][p], ((depth, w, h, sub, i), "den_q", p, q[p, :, 1], want["den_q"][p])
            assert min(want["den_q"][0]) > 0 and sum(want["num_q"][0]) > 0
            pos += 24
    assert pos == got.size
    # one thread block at scale 1, several, blocks of a chroma plane that found no tile, and partly empty blocks
    assert min(scale1_blocks) == 1 and max(scale1_blocks) >= 12 and dead > 0 and idle > 0, (scale1_blocks, dead, idle)
