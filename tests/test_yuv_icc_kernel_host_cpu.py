"""The device code of the fused Y'CbCr + ICC ingest (codec-eval_amd/csrc/yuv_icc_kernel.h's k_yuv_icc_encode and
yuv_cicp_kernel.h's k_yuv_tagged around icc_pixel.h's and icc_lut_pixel.h's pixels) compiled for the host with
-ffp-contract=off and run under AddressSanitizer and UBSan (tests/cpp/yuv_icc_kernel_host.cpp): the same text the GPU runs,
every thread of every block in turn, over the case list of tests/yuv_icc_cases.py, on planes, tables, a CLUT, sampled curves,
thresholds and a slab allocated at exactly their size, the image written into slot 0, 1 or 2 of the slab at an offset that
changes the store width, the thresholds' entry 0 poisoned.  Its output must equal the composed numpy restatement bit for
bit, the other slots must stay untouched, and the sanitizers must see no access outside the buffers and no misaligned wide
access.  Covers what a device run cannot show: an out-of-bounds access that happens to land in mapped memory."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icc_lut_restatement as LR  # noqa: E402
import icc_restatement as R  # noqa: E402
import yuv_icc_cases as K  # noqa: E402
import yuv_restatement as Y  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"identity": 0, "sampled": 1, "power": 2}
OUT_KIND = {"lin": 0, "u8": 1, "u16": 2}
# the offsets a slab starts at behind a 16-byte boundary, per slot kind: every residue a store width is picked from
OFFS = {"lin": (0, 4, 8, 12), "u8": (0, 1, 2, 4), "u16": (0, 2, 4, 8)}


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("yuvicchost") / "yuv_icc_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-fno-strict-aliasing", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "yuv_icc_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernels_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = K.cases()
    blocks, offsets, pos = [], {}, 0

    def put(key, arr):
        nonlocal pos
        if key not in offsets:
            offsets[key] = pos
            blocks.append(np.ascontiguousarray(arr, np.float32).reshape(-1))
            pos += blocks[-1].size
        return offsets[key]

    with open(tmp_path / "cases.txt", "w") as f:
        for n, c in enumerate(cs):
            (w, h), (d, msb), D, (kind, depth_out) = c["shape"], c["sample"], K.rgb_depth(c), c["dest"]
            flavour, _, interpolation = K.PROFILES[c["profile"]]
            p = K.profile_bytes(c["profile"])
            k = Y.coefficients(c["matrix"], c["range"], d, D)
            fields = [w, h, c["sub"], c["layout"], c["mode"], d, int(msb), c["pad"] * (1 if d == 8 else 2), c["slot"], OFFS[kind][n % 4], c["seed"], *k,
                      (1 << D) - 1]
            thr_at = put(("thr", depth_out), R.thresholds(depth_out)) if depth_out else 0
            if flavour == "matrix":
                fields += [put((c["profile"], D), R.tables(p, D)), OUT_KIND[kind], depth_out, thr_at, 0, int(R.has_matrix(p)), 0, 0, 0, 0, 0, 0, 0,
                           put((c["profile"], "m"), R.matrix(p))]
                fields += [0] * 60
            else:
                cl = LR.clut_nodes(p)
                grid, cl_at = (cl[0], put((c["profile"], "clut"), cl[1])) if cl else ((0, 0, 0), 0)
                parsed = LR.read_profile(p)
                pcs = 0 if parsed["pcs"] == b"XYZ " else 2 if parsed["type"] == b"mft2" else 1
                fields += [put((c["profile"], D), LR.input_tables(p, D)), OUT_KIND[kind], depth_out, thr_at, 1, interpolation, cl_at, *grid, pcs,
                           int(parsed["matrix"] is not None), put((c["profile"], "mat"), LR.matrix12(p)), put("pcsm", LR.pcs_matrix())]
                for i, cv in enumerate(LR.curves(p)):
                    q = np.array(cv[2] if cv[0] == "power" else [0.0] * 7, np.float64).view(np.uint64).tolist()
                    cnt = len(cv[1]) if cv[0] == "sampled" else cv[1] if cv[0] == "power" else 0
                    fields += [KINDS[cv[0]], cnt, put((c["profile"], "curve", i), cv[1]) if cv[0] == "sampled" else 0, *q]
            f.write(" ".join(str(int(v)) for v in fields) + "\n")
    np.concatenate(blocks).tofile(tmp_path / "tables.bin")
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "tables.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout) == len(cs)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos = 0

    def take(nbytes):
        nonlocal pos
        a = raw[pos:pos + nbytes]
        pos += nbytes
        return a

    above = 0
    for c in cs:
        (w, h), (d, msb), sub, slot = c["shape"], c["sample"], c["sub"], c["slot"]
        dt = np.uint8 if d == 8 else np.uint16
        bps = np.dtype(dt).itemsize
        cw, ch = Y.chroma_size(w, h, sub)
        y = take(h * w * bps).view(dt).reshape(h, w)
        cb = cr = None
        if sub != Y.SUB_400:
            if c["layout"] == Y.SEMIPLANAR:
                cbcr = take(ch * 2 * cw * bps).view(dt).reshape(ch, 2 * cw)
                cb, cr = cbcr[:, 0::2], cbcr[:, 1::2]
            else:
                cb = take(ch * cw * bps).view(dt).reshape(ch, cw)
                cr = take(ch * cw * bps).view(dt).reshape(ch, cw)
        if not msb:
            above += int((y.astype(np.int64) > (1 << d) - 1).sum())
        want = K.want_of(c, (y, cb, cr))
        assert want.dtype == {"lin": np.float32, "u8": np.uint8, "u16": np.uint16}[c["dest"][0]]
        n = w * h * 3 * want.dtype.itemsize
        slab = take((slot + 2) * n)
        assert np.array_equal(slab[slot * n:(slot + 1) * n], want.reshape(-1).view(np.uint8)), c
        assert np.all(slab[:slot * n] == 0xEE) and np.all(slab[(slot + 1) * n:] == 0xEE), c
    assert pos == raw.size
    assert above > 1000  # samples above 2^d - 1 were met (and clamped)
