"""The device code of the CIEDE2000 maps (codec-eval_amd/csrc/ciede2000_map_kernel.h, on top of ciede2000_kernel.h and the
ciede2000_pixel.h they run) compiled for the host with -ffp-contract=off and run under AddressSanitizer and UBSan
(tests/cpp/ciede2000_map_kernel_host.cpp, a stand-alone program with its own main; nothing of it is loaded into Python): the same
text the GPU runs, every thread of every block of the launcher's own grid in turn, on slabs, pair tables, sRGB tables, an LDS
stand-in, maps and cell arrays allocated at exactly their size.  Every map element, every cell and every count must equal the
numpy restatement (tests/ciede2000_map_restatement.py) exactly, for every `what`, on both load paths and both slab types, and the
sanitizers must see no access outside the buffers and no misaligned 16-byte load or store."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ciede2000_cases as K  # noqa: E402
import ciede2000_map_restatement as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(1, 1), (3, 1), (4, 1), (5, 3), (16, 8), (5, 16)]
CLIPPED = [(72, 34), (70, 37)]  # 2448 = 16 * 153 pixels on the wide path, 2590 on the scalar one: clipped cells on both edges at every B
# a deep image of 512 x 264 pixels with 16 pairs: 64 blocks a pair whose lanes hold 131072 pixels, eight each
HOST_BIG, HOST_BIG_KIND = (512, 264), (12, 16)


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ciemaphost") / "ciede2000_map_kernel_host"
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ciede2000_map_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def layouts():
    """-> [(w, h, kind, n_pairs, what, blocks)]: the small and the clipped shapes at every kind and every `what`, the clipped ones
    at every B; 333 x 251 (several blocks a pair, ragged) and the large shapes with one `what` each, in turn."""
    out = [(w, h, kind, 5, what, (2, 4, 64)) for w, h in SMALL for kind in K.KINDS for what in M.WHATS]
    out += [(w, h, kind, 5, what, M.BLOCKS) for w, h in CLIPPED for kind in K.KINDS for what in M.WHATS]
    out += [(333, 251, kind, 5, what, (8,)) for kind, what in (((0, 0), M.DH), ((16, 16), M.DC), ((8, 16), M.DL))]
    out.append(HOST_BIG + (HOST_BIG_KIND, K.BIG_PAIRS, M.DE, (32,)))
    out.append(K.BIG + ((0, 0), K.BIG_PAIRS, M.DH, ()))
    return out


def test_host_build_of_the_map_kernel_equals_the_restatement_with_no_stray_access(ce, host_kernel, tmp_path):
    K.use(ce)
    cases = layouts()
    with open(tmp_path / "cases.txt", "w") as cfg, open(tmp_path / "in.bin", "wb") as data:
        for w, h, kind, n_pairs, what, blocks in cases:
            dr, dt = (8, 8) if kind == (0, 0) else kind
            refs, tests = K.images(w, h, kind)
            binding = [K.BINDING[p % 5] for p in range(n_pairs)]
            cfg.write(f"{int(kind != (0, 0))} {dr} {dt} {w} {h} 2 {n_pairs} {what} {' '.join(map(str, K.THRESHOLDS))} "
                      f"{' '.join(map(str, binding))} {len(blocks)} {' '.join(map(str, blocks))}\n")
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
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos, seen = 0, set()

    def take(dtype, count):
        nonlocal pos
        out = raw[pos:pos + count * np.dtype(dtype).itemsize].view(dtype)
        pos += out.nbytes
        assert out.size == count
        return out

    for n, (w, h, kind, n_pairs, what, blocks) in enumerate(cases):
        _, _, nblocks, path, lds = lines[n].split()
        deep = kind != (0, 0)
        assert int(nblocks) == K.blocks(w * h, n_pairs, deep) and (path == "wide") == K.wide(w * h, deep), (w, h, kind)
        seen.add((deep, path, K.goes_round(w * h, n_pairs, deep), what))
        want = M.expected(w, h, kind)[..., what]  # [5, h, w]
        full = take(np.uint32, n_pairs * w * h).reshape(n_pairs, h, w)
        for p in range(n_pairs):
            assert np.array_equal(full[p], want[p % 5]), (w, h, kind, what, p)
        for block in blocks:
            ch, cw = -(-h // block), -(-w // block)
            cells = take(np.uint32, n_pairs * ch * cw).reshape(n_pairs, ch, cw)
            for p in range(n_pairs):
                assert np.array_equal(cells[p], M.block_max(want[p % 5], block)), (w, h, kind, what, block, p)
        counts = take(np.uint64, (2 + len(blocks)) * n_pairs * 8).reshape(2 + len(blocks), n_pairs, 8)
        for p in range(n_pairs):
            over = M.over(want[p % 5], K.THRESHOLDS)
            for run in range(2 + len(blocks)):
                assert np.array_equal(counts[run, p], over), (w, h, kind, what, run, p)
    assert pos == raw.size
    # every `what` on both load paths of both slab types
    assert {(d, p, wh) for d, p, _, wh in seen} == {(d, p, wh) for d in (False, True) for p in ("wide", "scalar") for wh in M.WHATS}
    # the grid-stride loop went round on the scalar path (333 x 251 with five pairs) and on the wide one of both slab types
    assert {(d, p) for d, p, r, _ in seen if r} == {(False, "scalar"), (True, "scalar"), (False, "wide"), (True, "wide")}
    # 5 x 16: the wide path with w below the unit; 72 x 34: units that straddle row ends
    assert K.wide(5 * 16, False) and K.wide(5 * 16, True) and K.wide(72 * 34, False) and 72 % 16 and not K.wide(70 * 37, True)
