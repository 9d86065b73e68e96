"""The device code of the LUT-based ICC ingest (codec-eval_amd/csrc/icc_kernel.h and cicp_kernel.h around icc_lut_pixel.h's
pixel) compiled for the host with -ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/icc_lut_kernel_host.cpp):
the same text the GPU runs, every thread of every block in turn, on a source, three input tables, a CLUT, sampled curves,
thresholds and a slab allocated at exactly their size, the image written into slot 0, 1 or 2 of the slab at an offset that
changes the store width.  The cases are the GPU test's: every fixture, both interpolations, every format and source depth, the
six shapes, the pixels of icc_lut_restatement.edge_pixels.  The output must equal the numpy restatement bit for bit, the other
slots must stay untouched, and the sanitizers must see no access outside the buffers and no misaligned wide access."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_lut_restatement as L  # noqa: E402
import icc_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (3, 5), (7, 2), (16, 1), (17, 9), (100, 76))
FORMATS = {0: (np.uint8, 3), 1: (np.uint8, 4), 4: (np.uint16, 3), 5: (np.uint16, 4)}  # CE_PIXEL_*: sample type, channels
# out_kind (0 f32, 1 u8, 2 u16), the slot's depth, the offsets a slab starts at behind a 16-byte boundary
OUTPUTS = ((0, 0, (0, 4, 8, 16)), (1, 8, (0, 1, 2, 4)), (2, 8, (0, 2, 4, 8)), (2, 10, (0, 2, 4, 8)), (2, 12, (0, 2, 4, 8)), (2, 16, (0, 2, 4, 8)))
KINDS = {"identity": 0, "sampled": 1, "power": 2}


def cases():
    """every format x source depth x output x shape, the fixture and the interpolation walking"""
    names = sorted(L.fixtures())
    out, n = [], 0
    for fmt in FORMATS:
        for depth in ((8,) if fmt < 2 else R.DEPTHS):
            for kind, depth_out, offs in OUTPUTS:
                for w, h in SHAPES:
                    out.append(dict(fmt=fmt, depth=depth, n_px=w * h, slot=n % 3, off=offs[(n // 3) % 4], seed=900 + n, kind=kind, depth_out=depth_out,
                                    profile=names[n % len(names)], tetra=(n // len(names)) % 2))
                    n += 1
    return out


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("icclut") / "icc_lut_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function", "-fno-strict-aliasing",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "icc_lut_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernels_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    F = L.fixtures()
    assert {c["profile"] for c in cs} == set(F) and {(c["profile"], c["tetra"]) for c in cs} >= {(n, t) for n in F for t in (0, 1)}
    blocks, offsets, pos = [], {}, 0

    def put(key, arr):
        nonlocal pos
        if key not in offsets:
            offsets[key] = pos
            blocks.append(np.ascontiguousarray(arr, np.float32).reshape(-1))
            pos += blocks[-1].size
        return offsets[key]

    sources, src_pos = [], 0
    with open(tmp_path / "cases.txt", "w") as f:
        for c in cs:
            p = F[c["profile"]]
            dt, nc = FORMATS[c["fmt"]]
            c["src"] = L.edge_pixels(p, c["depth"], nc, dt, c["n_px"], c["seed"])
            src_at, src_pos = src_pos, src_pos + c["src"].nbytes
            sources.append(c["src"].reshape(-1).view(np.uint8))
            t_at = put((c["profile"], c["depth"]), L.input_tables(p, c["depth"]))
            thr_at = put(("thr", c["depth_out"]), R.thresholds(c["depth_out"])) if c["kind"] else 0
            cl = L.clut_nodes(p)
            grid, cl_at = (cl[0], put((c["profile"], "clut"), cl[1])) if cl else ((0, 0, 0), 0)
            parsed = L.read_profile(p)
            pcs = 0 if parsed["pcs"] == b"XYZ " else 2 if parsed["type"] == b"mft2" else 1
            fields = [c["fmt"], c["n_px"], c["slot"], c["off"], src_at, (1 << c["depth"]) - 1, t_at, c["kind"], c["depth_out"], thr_at, c["tetra"], cl_at, *grid, pcs,
                      int(parsed["matrix"] is not None), put((c["profile"], "mat"), L.matrix12(p)), put("pcsm", L.pcs_matrix())]
            for k, cv in enumerate(L.curves(p)):
                q = np.array(cv[2] if cv[0] == "power" else [0.0] * 7, np.float64).view(np.uint64).tolist()
                n = len(cv[1]) if cv[0] == "sampled" else cv[1] if cv[0] == "power" else 0
                fields += [KINDS[cv[0]], n, put((c["profile"], "curve", k), cv[1]) if cv[0] == "sampled" else 0, *q]
            f.write(" ".join(str(int(v)) for v in fields) + "\n")
    np.concatenate(blocks).tofile(tmp_path / "tables.bin")
    np.concatenate(sources).tofile(tmp_path / "sources.bin")
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "tables.bin"), str(tmp_path / "sources.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout) == len(cs)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos = 0
    for c in cs:
        n_px, slot, p = c["n_px"], c["slot"], F[c["profile"]]
        if c["kind"] == 0:
            want = L.to_linear(c["src"], p, c["depth"], c["tetra"])
        else:
            want = L.to_srgb(c["src"], p, c["depth"], c["depth_out"], out16=c["kind"] == 2, interpolation=c["tetra"])
        slot_bytes = n_px * 3 * want.dtype.itemsize
        assert want.dtype == (np.float32, np.uint8, np.uint16)[c["kind"]]
        slab = raw[pos:pos + (slot + 2) * slot_bytes]
        pos += (slot + 2) * slot_bytes
        got = slab[slot * slot_bytes:(slot + 1) * slot_bytes]
        assert np.array_equal(got, want.reshape(-1).view(np.uint8)), {k: v for k, v in c.items() if k != "src"}
        assert np.all(slab[:slot * slot_bytes] == 0xEE) and np.all(slab[(slot + 1) * slot_bytes:] == 0xEE), c["profile"]
    assert pos == raw.size
