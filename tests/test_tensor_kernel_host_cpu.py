"""The device code of the tensor ingest (codec-eval_amd/csrc/tensor_kernel.h) compiled for the host and run under
AddressSanitizer and UBSan (tests/cpp/tensor_kernel_host.cpp): the same text the GPU runs, every thread of every block in
turn, with the arguments ce_launch_tensor makes, on sources allocated at exactly their extent and slots of exactly theirs,
placed at every offset from a 16-byte boundary at which the kernel chooses another load path or store width.  Its output must
equal the numpy restatement bit for bit, and the sanitizers must see no access outside the buffers and no misaligned wide
access.  Covers what a device run cannot show: an out-of-bounds access that happens to land in mapped memory."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tensor_restatement as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 259)  # around the group (4, 8 or 16 pixels) and a block's 64 threads
OFFSETS_U8 = (0, 1, 2, 3, 4, 8, 16)
OFFSETS_WIDE = (0, 2, 4, 6, 16)  # u16 slots; f32 slots take the multiples of 4
SLOTS = {"u8": 0, "u16": 1, "lin": 2}
PAIRS = [(T.U8, "u8"), (T.U8, "u16"), (T.U16, "u16")] + [(dt, s) for dt in (T.F16, T.BF16, T.F32) for s in ("u8", "u16", "lin")]
LAYOUTS = ("planar", "hwc", "rgba", "gray", "padded")
H = 3


def strides(layout, w, count):
    """(sn, sc, sy, sx) in elements"""
    if layout == "planar":
        return 3 * H * w, H * w, w, 1
    if layout == "hwc":
        return H * w * 3, 1, w * 3, 3
    if layout == "rgba":
        return H * w * 4, 1, w * 4, 4
    if layout == "gray":
        return H * w, 0, w, 1
    return 3 * H * (w + 5) + 7, H * (w + 5), w + 5, 1  # a cropped view: rows and images further apart than their pixels


def cases():
    out, n = [], 0
    for dtype, slot in PAIRS:
        es = T.ELEM_BYTES[dtype]
        dst_offs = OFFSETS_U8 if slot == "u8" else OFFSETS_WIDE if slot == "u16" else (0, 4, 8, 16)
        src_offs = range(16 // es)
        for layout in LAYOUTS:
            for w in WIDTHS:
                # every source offset with the slot offsets in turn, then every slot offset over an aligned source
                for so, do in [(so, dst_offs[(n + so) % len(dst_offs)]) for so in src_offs] + [(0, do) for do in dst_offs]:
                    count = 3 if n % 2 else 1
                    depth = 8 if slot == "u8" or dtype == T.U8 else (8, 10, 12, 16)[n % 4]
                    quant = (n // 2) % 2 if dtype >= T.F16 and slot != "lin" else 0
                    sn, sc, sy, sx = strides(layout, w, count)
                    extent = (count - 1) * sn + 2 * sc + (H - 1) * sy + (w - 1) * sx + 1
                    out.append(dict(dtype=dtype, slot=slot, depth=depth, quant=quant, st=(sn, sc, sy, sx), w=w, count=count, dst_off=do,
                                    src_off=so, extent=extent, layout=layout))
                    n += 1
    return out


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tensorhost") / "tensor_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "tensor_kernel_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_host_build_of_the_kernel_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    rng = np.random.default_rng(11)
    with open(tmp_path / "cases.txt", "w") as f, open(tmp_path / "src.bin", "wb") as g:
        for c in cs:
            c["src"] = T.sample_elements(rng, c["dtype"], c["extent"], c["slot"] == "lin")
            g.write(c["src"].tobytes())
            f.write(" ".join(str(v) for v in (c["dtype"], SLOTS[c["slot"]], c["depth"], c["quant"], *c["st"], c["w"], H, c["count"], c["dst_off"],
                                              c["src_off"], c["extent"])) + "\n")
    r = subprocess.run([host_kernel, str(tmp_path / "cases.txt"), str(tmp_path / "src.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert int(r.stdout) == len(cs)
    raw = np.fromfile(tmp_path / "out.bin", np.uint8)
    pos = 0
    seen = set()
    for c in cs:
        dst_dt = {"u8": np.uint8, "u16": np.uint16, "lin": np.uint32}[c["slot"]]
        n = c["count"] * H * c["w"] * 3
        got = raw[pos:pos + n * np.dtype(dst_dt).itemsize].view(dst_dt).reshape(c["count"], H, c["w"], 3)
        pos += n * np.dtype(dst_dt).itemsize
        want = T.to_slot(T.gather(c["src"], 0, c["st"], c["count"], H, c["w"]), c["dtype"], c["slot"], c["depth"], c["quant"])
        if c["slot"] == "lin":
            want = want.view(np.uint32)
        assert np.array_equal(got, want), {k: v for k, v in c.items() if k != "src"}
        seen.add((c["dtype"], c["slot"], c["layout"], c["quant"], c["count"]))
    assert pos == raw.size
    for dtype, slot in PAIRS:
        for layout in LAYOUTS:
            for count in (1, 3):
                quants = (0, 1) if dtype >= T.F16 and slot != "lin" else (0,)
                assert all((dtype, slot, layout, q, count) in seen for q in quants)
