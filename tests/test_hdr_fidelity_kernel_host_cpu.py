"""The device code of the HDR fidelity scores (codec-eval_amd/csrc/hdr_fidelity_kernel.h) compiled for the host with
-ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/hdr_fidelity_kernel_host.cpp, a stand-alone program with
its own main; nothing of it is loaded into Python): the same text the GPU runs, every thread of every block of the launcher's
own grid in turn, on slabs, pair tables, thresholds and an LDS stand-in allocated at exactly their size.  The three integers of
every pair must equal the numpy restatement (tests/hdr_fidelity_restatement.py) exactly - the f64 square root, quotient and
rint included - and the sanitizers must see no access outside the buffers and no misaligned 16-byte load."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_fidelity_cases as K  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hdrfhost") / "hdr_fidelity_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "hdr_fidelity_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def layouts():
    """-> [(shape index, depth, white, refs, tests, pair_ref)]: every shape's pairs at each of its parameters, as one batch with
    a reference slot per distinct reference (pairs that share a reference array share its slot, so pair_ref is no identity);
    the largest shape once, at depth 16 (two four-pixel groups a lane)."""
    out = []
    for si, (w, h, params, pairs) in enumerate(K.shape_cases()):
        refs, tests, pair_ref = [], [], []
        for _, ref, test in pairs:
            slot = next((i for i, r in enumerate(refs) if r is ref), None)
            if slot is None:
                slot = len(refs)
                refs.append(ref)
            tests.append(test)
            pair_ref.append(slot)
        for depth, white in (params if w * h < 100000 else [p for p in params if p[0] == 16]):
            out.append((si, depth, white, refs, tests, pair_ref))
    return out


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    a, b = F.matrices()
    mats = " ".join(str(v) for v in np.concatenate([a.reshape(-1), b.reshape(-1)]).view(np.uint32).tolist())
    cases = layouts()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for si, depth, white, refs, tests, pair_ref in cases:
            n_px = refs[0].shape[0] * refs[0].shape[1]
            cfg.write(f"{depth} {n_px} {len(refs)} {len(tests)} {mats} {' '.join(map(str, pair_ref))}\n")
            F.thresholds(depth, white).tofile(data)
            for img in refs + tests:
                assert img.dtype == np.float32 and img.size == n_px * 3
                np.ascontiguousarray(img).tofile(data)
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == f"done {len(cases)}"
    got = np.fromfile(tmp_path / "out.bin", np.uint64)
    pos, paths, blocks = 0, set(), []
    for n, (si, depth, white, refs, tests, pair_ref) in enumerate(cases):
        _, _, nblocks, path = lines[n].split()
        paths.add(path)
        blocks.append(int(nblocks))
        want = K.expected(si, depth, white)
        for p in range(len(tests)):
            triple = tuple(int(v) for v in got[pos:pos + 3])
            assert triple == (want[p]["pq_sse"], want[p]["itp_sum_q20"], want[p]["itp_max_q20"]), (si, depth, white, p)
            pos += 3
    assert pos == got.size
    assert paths == {"wide", "scalar"} and min(blocks) == 1 and max(blocks) >= 64
    # the largest shape ran with fewer lanes than four-pixel groups: the grid-stride loop went round
    w, h, _, pairs = K.shape_cases()[-1]
    assert blocks[-1] * 256 * 4 < w * h
