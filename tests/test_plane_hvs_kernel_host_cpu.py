"""The device code of PSNR-HVS / PSNR-HVS-M (codec-eval_amd/csrc/plane_hvs_kernel.h) compiled for the host with
-ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/plane_hvs_kernel_host.cpp, a stand-alone program with
its own main; nothing of it is loaded into Python): the same text the GPU runs, every thread of every block of the launcher's
own grid in turn and phase by phase, on planes allocated at exactly their size - pitch padding between rows only, none after
the last row - with tables and an LDS stand-in sized the same way.  Every sum of every pair must equal the numpy restatement
(tests/plane_hvs_restatement.py), and the sanitizers must see no access outside the buffers."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_hvs_cases as HK  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hvshost") / "plane_hvs_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "plane_hvs_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def cases():
    """-> [((depth, w, h, sub, step), references, tests, pair table, wants)], an image as (layout, msb, planes)"""
    out = []
    for n, (w, h, sub, depth, step, layout, msb) in enumerate(HK.SHAPES):
        ref, test = HK.planes(w, h, sub, depth)
        pad = (1, 3)[n % 2] * (1 if depth == 8 else 2)  # odd pitches where the samples are bytes
        refs = [(K.PLANAR, False, K.host_planes(ref, sub, depth, K.PLANAR, False, 0))]
        tests = [(layout, msb, K.host_planes(test, sub, depth, layout, msb, pad, seed=n))]
        out.append(((depth, w, h, sub, step), refs, tests, [0], [HK.expected(w, h, sub, depth, step)]))
    # two references, three pairs, a pair table that is no identity, mixed layouts
    w, h, sub, step = 93, 67, HK.H.SUB_420, 7
    refs = [(K.SEMIPLANAR, False, K.host_planes(HK.planes(w, h, sub, 8, s)[0], sub, 8, K.SEMIPLANAR, pad=5)) for s in (0, 1)]
    tests = [(K.PLANAR, False, K.host_planes(HK.planes(w, h, sub, 8, s)[1], sub, 8, pad=1)) for s in (1, 0, 2)]
    wants = [HK.expected(w, h, sub, 8, step, 1), HK.expected(w, h, sub, 8, step, 0), HK.expected(w, h, sub, 8, step, 2, 1)]
    out.append(((8, w, h, sub, step), refs, tests, [1, 0, 1], wants))
    return out


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for (depth, w, h, sub, step), refs, tests, pair_ref, _ in cs:
            words = [depth, w, h, sub, len(refs), len(tests), step] + pair_ref
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
    pos, thread_blocks, dead = 0, [], 0
    for n, ((depth, w, h, sub, step), refs, tests, pair_ref, wants) in enumerate(cs):
        f = lines[n].split()
        thread_blocks.append(int(f[2]))
        dead += int(f[3])
        for i, want in enumerate(wants):
            q = got[pos:pos + 12].reshape(3, 2, 2)
            for p in range(3):
                for m, name in enumerate(("hvs_q", "hvsm_q")):
                    total = int(q[p][m][0]) + (int(q[p][m][1]) << 32)
                    assert total == want[name][p][0] + (want[name][p][1] << 32), ((depth, w, h, sub, step, i), name, p)
            assert want["hvs_q"][0] != [0, 0]
            pos += 12
    assert pos == got.size
    assert min(thread_blocks) == 1 and max(thread_blocks) >= 9 and dead > 0  # one thread block, several, and some partly empty
