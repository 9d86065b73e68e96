"""The device code of the gain-map ingest (codec-eval_amd/csrc/gainmap_kernel.h with the gainmap_pixel.h it runs) compiled
for the host with -ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/gainmap_kernel_host.cpp, a stand-alone
program): the same text the GPU runs, every thread of every block in turn, on a base, a map, tables and a slab allocated at
exactly their size, the image written into slot 0, 1 or 2 of the slab.  Its output must equal the numpy restatement
(tests/gainmap_restatement.py) bit for bit - gm_exp2's f64 sequence included - the other slots must stay untouched, and the
sanitizers must see no access outside the buffers and no misaligned wide access."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import gainmap_restatement as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (base w, h), (map gw, gh): one pixel; a map of one sample, of the base's size and between; rows shorter than a group, so
# that a group spans several; a one-row image; an odd shape with a tail; more than one block, with a map a quarter of the
# base's size each way and one that is full height only
SHAPES = (((1, 1), (1, 1)), ((3, 5), (1, 1)), ((3, 5), (2, 2)), ((3, 5), (3, 5)), ((7, 2), (2, 1)), ((16, 1), (4, 1)), ((17, 9), (5, 3)),
          ((100, 76), (25, 19)), ((100, 76), (33, 76)))
FORMATS = {0: (np.uint8, 3), 1: (np.uint8, 4), 4: (np.uint16, 3), 5: (np.uint16, 4)}  # CE_PIXEL_*: sample type, channels
CHANNELS = (1, 3)


def cases():
    """every format x primaries x map channels x shape; the metadata (gamma 1 and 2.2, W in {0, 0.37, 1}, zero and non-zero
    offsets), the transfer and the depth of the u16 formats walk through their lists"""
    out, n = [], 0
    for fmt in FORMATS:
        for prim in R.PRIMARIES:
            for channels in CHANNELS:
                for base, gmap in SHAPES:
                    out.append(dict(fmt=fmt, prim=prim, channels=channels, base=base, map=gmap, slot=n % 3, off=(0, 4, 8, 16)[n % 4], seed=300 + n,
                                    depth=8 if fmt < 2 else R.DEPTHS[n % 4], transfer=R.TRANSFERS[(n // 2) % 3], meta=G.METAS[(n // 3) % len(G.METAS)]))
                    n += 1
    return out


def coverage(c, src):
    """what the cases together must have met, counted for one case: pixels whose
    sample position was clamped at the map's left, right, top and bottom edge; pixels with a zero and with a non-zero
    fraction; groups of four that straddle a row end; samples above maxv"""
    (w, h), (gw, gh) = c["base"], c["map"]
    x, y = np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64)
    nx, ny = (2 * x + 1) * gw - w, (2 * y + 1) * gh - h
    _, _, fx = G.axis(w, gw)
    _, _, fy = G.axis(h, gh)
    frac = (fx[None, :] != 0) | (fy[:, None] != 0)
    first = np.arange(w * h // 4, dtype=np.int64) * 4
    return np.array([(nx < 0).sum() * h, (nx > (gw - 1) * 2 * w).sum() * h, (ny < 0).sum() * w, (ny > (gh - 1) * 2 * h).sum() * w,
                     (~frac).sum(), frac.sum(), (first % w + 3 >= w).sum(), (src[:, :3].astype(np.int64) > (1 << c["depth"]) - 1).sum()])


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("gainmaphost") / "gainmap_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "gainmap_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    todo = cases()
    tables, offsets, pos = [], {}, 0
    for c in todo:
        key = (c["transfer"], c["depth"])
        if key not in offsets:
            offsets[key] = pos
            tables.append(R.transfer_table(*key))
            pos += 1 << c["depth"]
    np.concatenate(tables).tofile(tmp_path / "tables.bin")
    ytabs = [G.tables(c["meta"], c["channels"]) for c in todo]
    np.concatenate([t.reshape(-1) for t in ytabs]).tofile(tmp_path / "ytables.bin")
    ypos = np.concatenate([[0], np.cumsum([t.size for t in ytabs])])
    with open(tmp_path / "cases.txt", "w") as f:
        for n, c in enumerate(todo):
            pick = (0, 1, 2) if c["channels"] == 3 else (0, 0, 0)
            kb = np.array([c["meta"].f32("base_offset")[k] for k in pick], np.float64).view(np.uint64).tolist()
            ka = np.array([c["meta"].f32("alternate_offset")[k] for k in pick], np.float64).view(np.uint64).tolist()
            m = R.colour_matrix(c["prim"]).reshape(-1).view(np.uint32).tolist()
            f.write(" ".join(str(v) for v in (c["fmt"], *c["base"], *c["map"], c["channels"], c["slot"], c["off"], c["seed"], (1 << c["depth"]) - 1,
                                              offsets[(c["transfer"], c["depth"])], ypos[n], int(c["prim"] != 1), *m, *kb, *ka)) + "\n")
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "tables.bin"), str(tmp_path / "ytables.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout) == len(todo)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos = 0

    def take(nbytes):
        nonlocal pos
        a = raw[pos:pos + nbytes]
        pos += nbytes
        return a

    met = np.zeros(8, np.int64)
    for c in todo:
        (w, h), (gw, gh) = c["base"], c["map"]
        dt, nc = FORMATS[c["fmt"]]
        src = take(w * h * nc * np.dtype(dt).itemsize).view(dt).reshape(h, w, nc)
        gmap = take(gw * gh * c["channels"]).reshape(gh, gw, c["channels"])
        met += coverage(c, src.reshape(-1, nc))
        want = G.to_linear(src, c["prim"], c["transfer"], c["depth"], gmap, c["meta"])
        slot, n = c["slot"], w * h * 12
        slab = take((slot + 2) * n)
        assert np.array_equal(slab[slot * n:(slot + 1) * n], want.reshape(-1).view(np.uint8)), c
        assert np.all(slab[:slot * n] == 0xEE) and np.all(slab[(slot + 1) * n:] == 0xEE), c
    assert pos == raw.size
    # clamped at the left, right, top and bottom edge of the map; zero and non-zero fractions; groups straddling a row end;
    # samples above maxv (clamped)
    assert np.all(met >= 100), met
