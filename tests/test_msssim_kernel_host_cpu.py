"""The device code of SSIM / MS-SSIM (codec-eval_amd/csrc/msssim_kernel.h) compiled for the host with -ffp-contract=off and run
under AddressSanitizer and UBSan (tests/cpp/msssim_kernel_host.cpp, a stand-alone program with its own main; nothing of it is
loaded into Python): the same text the GPU runs, every thread of every block of the launcher's own grids in turn, on slabs,
pair tables, pyramid levels and LDS stand-ins allocated at exactly their size.  The integers of every pair must equal the numpy
restatement (tests/msssim_restatement.py) exactly - the f64 filters, quotients and rint included - and the sanitizers must see
no access outside the buffers and no misaligned 16-byte load."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mssimhost") / "msssim_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "msssim_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def cases():
    """-> [(w, h, depth, levels, refs, tests, pair_ref, wants)]: one pair a shape, and on 176 x 163 three pairs of two
    references with a pair table that is no identity"""
    out = []
    for (w, h, depth, levels) in ([(w, h, 8, 5) for w, h in K.SHAPES_8 + K.TILE_EDGES] + [(w, h, d, 5) for w, h, d in K.DEEP] +
                                  [(w, h, 8, 1) for w, h in K.ONE_LEVEL] + [(12, 11, 16, 1)]):
        ref, test = K.pair(w, h, depth)
        out.append((w, h, depth, levels, [ref], [test], [0], [K.expected(w, h, depth, levels)]))
    w, h = 176, 163
    refs = [K.pair(w, h, 8, 0)[0], K.pair(w, h, 8, 1)[0]]
    tests = [K.pair(w, h, 8, 1)[1], K.pair(w, h, 8, 0)[1], K.pair(w, h, 8, 2)[1]]
    wants = [K.expected(w, h, 8, 5, 1), K.expected(w, h, 8, 5, 0), K.expected(w, h, 8, 5, 2, 1)]
    out.append((w, h, 8, 5, refs, tests, [1, 0, 1], wants))
    return out


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for w, h, depth, levels, refs, tests, pair_ref, _ in cs:
            cfg.write(f"{refs[0].itemsize} {depth} {w} {h} {len(refs)} {len(tests)} {levels} {' '.join(map(str, pair_ref))}\n")
            for img in refs + tests:
                assert img.shape == (h, w, 3)
                np.ascontiguousarray(img).tofile(data)
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(cs)] == f"done {len(cs)}"
    got = np.fromfile(tmp_path / "out.bin", np.int64)
    pos, tiles = 0, []
    for n, (w, h, depth, levels, refs, tests, pair_ref, wants) in enumerate(cs):
        tiles.append(int(lines[n].split()[2]))
        for p, want in enumerate(wants):
            q = got[pos:pos + 30].reshape(5, 3, 2)
            assert q[:, :, 0].tolist() == want["ssim_q"], (w, h, depth, levels, p, "ssim_q")
            assert q[:, :, 1].tolist() == want["cs_q"], (w, h, depth, levels, p, "cs_q")
            pos += 30
    assert pos == got.size
    assert min(tiles) == 1 and max(tiles) >= 60  # one block, and grids of several rows and columns of tiles
