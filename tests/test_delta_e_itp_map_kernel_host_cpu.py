"""The device code of the Delta E ITP maps (codec-eval_amd/csrc/hdr_fidelity_map_kernel.h) compiled for the host with
-ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/delta_e_itp_map_kernel_host.cpp, a stand-alone program
with its own main; nothing of it is loaded into Python): the same text the GPU runs, every thread of every block of the
launcher's own grid in turn, on slabs, pair tables, thresholds, an LDS stand-in, maps and cell arrays allocated at exactly their
size.  The full map, the cell maxima at B = 8 and the counts at four thresholds - with the map, with the cells and alone - must
equal the numpy restatement (tests/delta_e_itp_map_restatement.py) exactly, and the sanitizers must see no access outside the
buffers and no misaligned 16-byte load or store."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import delta_e_itp_map_restatement as M  # noqa: E402
import hdr_fidelity_cases as K  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("itpmaphost") / "delta_e_itp_map_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "delta_e_itp_map_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def layouts():
    """-> [(shape index, depth, white, refs, tests, pair_ref)]: every shape's pairs at each of its parameters, as one batch with
    a reference slot per distinct reference (pairs that share a reference array share its slot, so pair_ref is no identity) -
    the layout tests/test_hdr_fidelity_kernel_host_cpu.py builds; the largest shape once, at depth 16."""
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


def test_host_build_of_the_map_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    a, b = F.matrices()
    mats = " ".join(str(v) for v in np.concatenate([a.reshape(-1), b.reshape(-1)]).view(np.uint32).tolist())
    cases = layouts()
    assert any(pair_ref != list(range(len(pair_ref))) for *_, pair_ref in cases)
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for si, depth, white, refs, tests, pair_ref in cases:
            h, w = refs[0].shape[:2]
            cfg.write(f"{depth} {w} {h} {len(refs)} {len(tests)} {mats} {' '.join(map(str, pair_ref))} {' '.join(map(str, M.THRESHOLDS))}\n")
            F.thresholds(depth, white).tofile(data)
            for img in refs + tests:
                assert img.dtype == np.float32 and img.shape == (h, w, 3)
                np.ascontiguousarray(img).tofile(data)
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(cases)] == f"done {len(cases)}"
    got = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos, paths, blocks = 0, set(), []

    def take(dtype, n):
        nonlocal pos
        out = got[pos:pos + n * np.dtype(dtype).itemsize].view(dtype)
        pos += out.nbytes
        return out

    for n, (si, depth, white, refs, tests, pair_ref) in enumerate(cases):
        _, _, nblocks, path = lines[n].split()
        paths.add(path)
        blocks.append(int(nblocks))
        h, w = refs[0].shape[:2]
        ch, cw, n_pairs = -(-h // 8), -(-w // 8), len(tests)
        maps = take(np.uint32, n_pairs * h * w).reshape(n_pairs, h, w)
        cells = take(np.uint32, n_pairs * ch * cw).reshape(n_pairs, ch, cw)
        counts = take(np.uint64, 3 * n_pairs * 4).reshape(3, n_pairs, 4)
        want = M.expected_maps(si, depth, white)
        for p in range(n_pairs):
            what = (si, depth, white, p)
            assert np.array_equal(maps[p], want[p]), what
            assert np.array_equal(cells[p], M.block_max(want[p], 8)), what
            for run in range(3):
                assert np.array_equal(counts[run, p], M.over(want[p], M.THRESHOLDS)), (what, run)
    assert pos == got.size
    assert paths == {"wide", "scalar"} and min(blocks) == 1 and max(blocks) >= 64
    # the largest shape ran with fewer lanes than four-pixel groups: the grid-stride loop went round
    w, h, _, pairs = K.shape_cases()[-1]
    assert (w, h) == (512, 256) and blocks[-1] * 256 * 4 < w * h
