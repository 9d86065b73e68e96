"""The device code of GMSD (codec-eval_amd/csrc/plane_gmsd_kernel.h) compiled for the host with -ffp-contract=off and run under
AddressSanitizer and UBSan (tests/cpp/plane_gmsd_kernel_host.cpp, a stand-alone program with its own main; nothing of it is
loaded into Python): the same text the GPU runs, every thread of every block of the launcher's own grid in turn and phase by
phase, on planes allocated at exactly their size - pitch padding between rows only, none after the last row - at an aligned
base with rows 16 bytes apart, where every row takes the wide path, and one sample off it with an odd pitch, where none
does.  Every integer of every pair must equal the numpy restatement (tests/plane_gmsd_restatement.py), the doubles the
header's finishing forms from them too, and the sanitizers must see no access outside the buffers."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_fidelity_cases as K  # noqa: E402
import plane_gmsd_cases as GK  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gmsdhost") / "plane_gmsd_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "plane_gmsd_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


stored_planes = GK.stored_planes


def to_16(row):
    return -row % 16


def cases():
    """-> [((depth, w, h, sub), references, tests, pair table, wants)], an image as (layout, msb, offset, planes)"""
    out = []
    for n, (w, h, sub, depth, layout, msb) in enumerate(GK.SHAPES):
        bps = 1 if depth == 8 else 2
        kinds = (GK.NOISY, GK.FLAT_TEST) if (w, h) == (93, 67) else (GK.NOISY,)
        ref = GK.planes(w, h, sub, depth)[0]
        refs = [(K.PLANAR, False, 0, stored_planes(ref, sub, depth, K.PLANAR, False, to_16))]
        tests, wants = [], []
        for kind in kinds:
            test = GK.planes(w, h, sub, depth, 0, kind)[1]
            # rows 16 bytes apart from an aligned base: the wide path; an odd pitch one sample off it: sample by sample
            tests.append((layout, msb, 0, stored_planes(test, sub, depth, layout, msb, to_16, seed=n)))
            tests.append((layout, msb, bps, stored_planes(test, sub, depth, layout, msb, lambda row: (1, 3)[n % 2] * bps, seed=n)))
            wants += [GK.expected(w, h, sub, depth, 0, None, kind)] * 2
        out.append(((depth, w, h, sub), refs, tests, [0] * len(tests), wants))
    # two references, three pairs, a pair table that is no identity, mixed layouts; the references one sample off alignment
    w, h, sub = 93, 67, GK.G.SUB_420
    refs = [(K.SEMIPLANAR, False, 1, stored_planes(GK.planes(w, h, sub, 8, s)[0], sub, 8, K.SEMIPLANAR, False, to_16)) for s in (0, 1)]
    tests = [(K.PLANAR, False, 0, stored_planes(GK.planes(w, h, sub, 8, s)[1], sub, 8, K.PLANAR, False, to_16)) for s in (1, 0, 2)]
    wants = [GK.expected(w, h, sub, 8, 1), GK.expected(w, h, sub, 8, 0), GK.expected(w, h, sub, 8, 2, 1)]
    out.append(((8, w, h, sub), refs, tests, [1, 0, 1], wants))
    return out


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for (depth, w, h, sub), refs, tests, pair_ref, _ in cs:
            words = [depth, w, h, sub, len(refs), len(tests)] + pair_ref
            for layout, msb, offset, planes in refs + tests:
                words += [layout, int(msb), offset] + [K.pitch_of(p) for p in planes]
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
    got = open(tmp_path / "out.bin", "rb").read()
    pos, thread_blocks, dead, wide = 0, [], 0, 0
    for n, ((depth, w, h, sub), refs, tests, pair_ref, wants) in enumerate(cs):
        f = lines[n].split()
        thread_blocks.append(int(f[2]) // (len(tests) * wants[0]["n_planes"]))
        dead += int(f[3])
        wide += int(f[4])
        for i, want in enumerate(wants):
            for p in range(want["n_planes"]):
                sum_q, lo, hi, n_pos, max_dis, gmsd, gmsm = struct.unpack_from("<5Q2d", got, pos)
                pos += 56
                where = ((depth, w, h, sub), i, p)
                assert (sum_q, [lo, hi], n_pos, max_dis) == (want["sum_q"][p], want["sum_q2"][p], want["n_pos"][p], want["max_dis"][p]), where
                assert gmsd == want["gmsd"][p] and gmsm == want["gmsm"][p], (where, gmsd, want["gmsd"][p])
    assert pos == len(got)
    # one thread block a plane, several (93 x 67 luma: 47 x 34 positions, 3 tiles), chroma planes with fewer tiles than the grid,
    # and rows that admit the wide path
    assert min(thread_blocks) == 1 and max(thread_blocks) >= 3 and dead > 0 and wide > 0
