"""The device code of the CIEDE2000 scores (codec-eval_amd/csrc/ciede2000_kernel.h with the ciede2000_pixel.h it runs) compiled
for the host with -ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/ciede2000_kernel_host.cpp, a stand-alone
program with its own main; nothing of it is loaded into Python): the same text the GPU runs, every thread of every block of the
launcher's own grid in turn, on slabs, pair tables, sRGB tables and an LDS stand-in allocated at exactly their size.  The ten
integers of every pair must equal the numpy restatement (tests/ciede2000_restatement.py) exactly, and the sanitizers must see no
access outside the buffers and no misaligned 16-byte load."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_cases as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a deep image of 512 x 264 pixels with 16 pairs: 64 blocks a pair whose lanes hold 131072 pixels, eight each
HOST_BIG, HOST_BIG_KIND = (512, 264), (12, 16)


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ciehost") / "ciede2000_kernel_host"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ciede2000_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def layouts():
    """-> [(w, h, kind, n_pairs, thresholds)]: every shape at every kind with five pairs, with the thresholds, once with none and twice
    with two tables of unequal depth in LDS, and the large deep shape with sixteen."""
    out = [(w, h, kind, 5, K.THRESHOLDS) for w, h in K.SHAPES for kind in K.KINDS]
    out += [(16, 8, (0, 0), 5, []), (16, 8, (10, 12), 5, K.THRESHOLDS), (5, 3, (12, 10), 5, K.THRESHOLDS)]  # two tables in LDS
    out.append(HOST_BIG + (HOST_BIG_KIND, K.BIG_PAIRS, K.THRESHOLDS))
    return out


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(ce, host_kernel, tmp_path):
    K.use(ce)
    cases = layouts()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for w, h, kind, n_pairs, thresholds in cases:
            dr, dt = (8, 8) if kind == (0, 0) else kind
            refs, tests = K.images(w, h, kind)
            thr = list(thresholds) + [(1 << 32) - 1] * (8 - len(thresholds))
            binding = [K.BINDING[p % 5] for p in range(n_pairs)]
            cfg.write(f"{int(kind != (0, 0))} {dr} {dt} {w * h} 2 {n_pairs} {' '.join(map(str, thr))} {' '.join(map(str, binding))}\n")
            K.TABLES[dr].astype(np.float32).tofile(data)
            K.TABLES[dt].astype(np.float32).tofile(data)
            for img in refs + [tests[p % 5] for p in range(n_pairs)]:
                assert img.dtype == (np.uint8 if kind == (0, 0) else np.uint16) and img.size == w * h * 3
                img.tofile(data)
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == f"done {len(cases)}"
    got = np.fromfile(tmp_path / "out.bin", np.uint64)
    pos, seen = 0, set()
    for n, (w, h, kind, n_pairs, thresholds) in enumerate(cases):
        _, _, nblocks, path, lds = lines[n].split()
        deep = kind != (0, 0)
        assert int(nblocks) == K.blocks(w * h, n_pairs, deep) and (path == "wide") == K.wide(w * h, deep), (w, h, kind)
        seen.add((deep, path, K.goes_round(w * h, n_pairs, deep), int(lds)))
        want = K.expected(w, h, kind, bool(thresholds))
        for p in range(n_pairs):
            ten = [int(v) for v in got[pos:pos + 10]]
            e = want[p % 5]
            assert ten == [e["sum_q20"], e["max_q20"]] + e["n_above"] + [0] * (8 - len(e["n_above"])), (w, h, kind, p)
            pos += 10
    assert pos == got.size
    # both load paths of both kernels; LDS for one table, for two, for one beside a gathered one and for none
    assert {(d, p) for d, p, _, _ in seen} == {(False, "wide"), (False, "scalar"), (True, "wide"), (True, "scalar")}
    assert {l for _, _, _, l in seen} == {256, 1024, 4096, 0, 1024 + 4096}
    # the grid-stride loop went round on the scalar path (333 x 251 with five pairs) and on the wide one (the large shape)
    assert (False, "scalar", True, 256) in seen and (True, "wide", True, 4096) in seen
    assert K.goes_round(333 * 251, 5, False) and K.goes_round(HOST_BIG[0] * HOST_BIG[1], K.BIG_PAIRS, True)
