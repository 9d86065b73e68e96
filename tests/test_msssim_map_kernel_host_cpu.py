"""The device code of the SSIM / MS-SSIM maps (codec-eval_amd/csrc/msssim_map_kernel.h) compiled for the host with
-ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/msssim_map_kernel_host.cpp, a stand-alone program with its
own main; nothing of it is loaded into Python): the same text the GPU runs, every thread of every block of the launcher's own
grids in turn, on slabs, pair tables, pyramid levels, LDS stand-ins, maps and cell arrays allocated at exactly their size.
Every element of the map and of the cells of every block, and every count, must equal the numpy restatement
(tests/msssim_map_restatement.py), and the sanitizers must see no access outside the buffers and no misaligned 8-byte store -
the rows of a map of odd width are not 8-byte aligned."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as K  # noqa: E402
import msssim_map_cases as MK  # noqa: E402
import msssim_map_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mssmaphost") / "msssim_map_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "msssim_map_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def cases():
    """-> [(w, h, depth, levels, level, what, refs, tests, pair_ref, want_maps)]: want_maps[p] the block-1 map of pair p.  One
    pair a shape and level; both values of `what` on 176 x 163; three pairs of two references with a pair table that is no
    identity; the checkerboard, which saturates."""
    out = []
    for w, h, depth, levels, lvls in MK.SHAPES:
        for level in lvls:
            for what in (("ssim", "cs") if (w, h) == (176, 163) else ("ssim",)):
                ref, test = K.pair(w, h, depth)
                out.append((w, h, depth, levels, level, what, [ref], [test], [0], [MK.expected(w, h, depth, levels, level, what)]))
    w, h = 176, 163
    refs = [K.pair(w, h, 8, 0)[0], K.pair(w, h, 8, 1)[0]]
    tests = [K.pair(w, h, 8, 1)[1], K.pair(w, h, 8, 0)[1], K.pair(w, h, 8, 2)[1]]
    wants = [MK.expected(w, h, 8, 5, 1, "cs", 1, 1), MK.expected(w, h, 8, 5, 1, "cs", 1, 0), MK.expected(w, h, 8, 5, 1, "cs", 1, 2, 1)]
    out.append((w, h, 8, 5, 1, "cs", refs, tests, [1, 0, 1], wants))
    a, b = K.checkerboard(43, 27)
    out.append((43, 27, 8, 1, 0, "ssim", [a], [b], [0], [R.full_map(a, b, 8, 1, 0)]))
    return out


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for w, h, depth, levels, level, what, refs, tests, pair_ref, _ in cs:
            cfg.write(f"{refs[0].itemsize} {depth} {w} {h} {len(refs)} {len(tests)} {levels} {level} {R.WHAT[what]} "
                      f"{' '.join(map(str, MK.THR8))} {' '.join(map(str, pair_ref))}\n")
            for img in refs + tests:
                assert img.shape == (h, w, 3)
                np.ascontiguousarray(img).tofile(data)
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(cs)] == f"done {len(cs)}"
    got = np.fromfile(tmp_path / "out.bin", np.uint32)
    pos, tiles, rows = 0, [], set()
    for n, (w, h, depth, levels, level, what, refs, tests, pair_ref, wants) in enumerate(cs):
        tiles.append(int(lines[n].split()[2]))
        rows.add(lines[n].split()[3])
        full = np.stack(wants)  # [pairs, 3, vh, vw]
        for block in MK.BLOCKS:
            want = R.cells(full, block)
            assert np.array_equal(got[pos:pos + want.size].reshape(want.shape), want), (w, h, depth, level, what, block)
            pos += want.size
        n_counts = len(tests) * 3 * 8
        counts = got[pos:pos + 4 * n_counts].view(np.uint64).reshape(2, len(tests), 3, 8)
        pos += 4 * n_counts
        want = np.stack([R.over(m, MK.THR8) for m in wants])
        assert np.array_equal(counts[0], want) and np.array_equal(counts[1], want), (w, h, depth, level, what)
        assert not want[:, :, 7].any() and (want[:, :, 0] > 0).all()
    assert pos == got.size
    assert min(tiles) == 1 and max(tiles) >= 60 and rows == {"odd_rows", "aligned_rows"}
