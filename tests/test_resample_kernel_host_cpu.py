"""The device code of the resampler (codec-eval_amd/csrc/resample_kernel.h) compiled for the host and run under
AddressSanitizer and UBSan (tests/cpp/resample_kernel_host.cpp): the same text the GPU runs, every thread of every block of
the grid the launcher's own geometry function returns, on tables, sources, an image between the passes, an LDS stand-in and
destinations allocated at exactly their size.  The tap tables are the product's (ce_build_resample_table, ce_tables.cpp
linked into the harness).  Output bytes must equal the numpy restatement (tests/resample_restatement.py, pinned to Pillow in
test_viewing_cpu.py), every table must equal the restatement's taps, and the sanitizers must see no access outside a buffer:
what a device run cannot show, where a byte past a row end lands in mapped memory.

The shapes sit where the index arithmetic changes: row lengths within a dword of 0, 1024 and 2048 bytes (the tile is 1024
row bytes, shifted by the row's address modulo 4) at all four destination phases, the last tap count that is staged in LDS
and the first that is not, the vertical pass's word loads at the end of an exactly sized source."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")  # ce_tables.cpp includes ce_internal.h, which includes the HIP runtime's header

TILE_BYTES, TILE_PIXELS, LDS_BYTES = 1024, 1024 // 3 + 2, 48 * 1024
EDGE_WIDTHS = (1, 2, 3, 4, 5, 340, 341, 342, 343, 682, 683, 684)  # row bytes within a dword of 0, 1024 and 2048
OFFSETS = (0, 1, 2, 3)

# The axis pairs of the table comparison besides those of the cases below.  DESIGN.md section 12 once cited 19 pairs x 4
# filters without naming them and they could not be recovered; these 19 are the axes of the shapes test_gpu_viewing.py
# sends to the device (down and up, integer and fractional scales, the global-table route, a one-sample axis).
TABLE_AXES = ((768, 384), (768, 256), (768, 1024), (768, 2304), (512, 171), (512, 683), (512, 1536), (3840, 1920), (2160, 1080),
              (2000, 150), (257, 193), (129, 97), (100, 300), (76, 228), (9, 5), (301, 151), (8, 3), (8, 24), (9, 1))


def cases():
    """(w, h, out_w, out_h, n, off, filter) of every kernel run."""
    out = []
    # tile edges: each width by 1:2 and 2:1 horizontal resampling, at every offset; three images, so the image stride and the
    # row stride each shift the phase (at 341 x 1 an image is 1023 bytes: images 0, 1, 2 at `off` 0 have phases 0, 3, 2)
    for ow in EDGE_WIDTHS:
        for w in (2 * ow, (ow + 1) // 2 if ow > 1 else 3):  # one pixel has no half: from three instead
            for h in (1, 2, 5):
                for off in OFFSETS:
                    out.append((w, h, ow, h, 3, off, R.LANCZOS3))
    # every filter at the first width past a tile and the one before it
    for filt in (R.BOX, R.BILINEAR, R.BICUBIC):
        for ow in (341, 342):
            for w in (2 * ow, (ow + 1) // 2):
                for off in OFFSETS:
                    out.append((w, 2, ow, 2, 3, off, filt))
    # the route boundary: 1840 -> 345 is ksize 33, the last that is staged; 1841 -> 345 is ksize 35, the first that is not;
    # both two tiles wide (1035 row bytes).  The other filters stage at both.
    for filt in R.FILTERS:
        for w in (1840, 1841):
            for off in OFFSETS:
                out.append((w, 2, 345, 2, 2, off, filt))
    out.append((3700, 2, 684, 2, 2, 3, R.LANCZOS3))  # global route, ksize 35, three tiles
    # the vertical pass alone: word loads up to the last byte of an exactly sized source
    for ow in EDGE_WIDTHS:
        for i, (h, oh) in enumerate(((1, 3), (7, 2), (301, 5), (5, 301))):
            for off in (OFFSETS if h < 301 and oh < 301 else ((ow + i) % 4,)):
                out.append((ow, h, ow, oh, 2, off, R.LANCZOS3))
    for filt in (R.BOX, R.BILINEAR, R.BICUBIC):
        for ow in (341, 342):
            out.append((ow, 7, ow, 2, 2, filt, filt))
            out.append((ow, 5, ow, 12, 2, 3 - filt, filt))
    # both passes, through the image between them
    for w, h, ow, oh in ((257, 129, 193, 97), (100, 7, 300, 21)):
        for off in OFFSETS:
            out.append((w, h, ow, oh, 3, off, R.LANCZOS3))
    for filt in (R.BOX, R.BILINEAR, R.BICUBIC):
        out.append((100, 7, 300, 21, 3, filt, filt))
    return out


def table_jobs(cs):
    axes = set()
    for w, h, ow, oh, _, _, filt in cs:
        axes.update({(w, ow, filt)} if ow != w else set())
        axes.update({(h, oh, filt)} if oh != h else set())
    axes.update((a, b, f) for a, b in TABLE_AXES for f in R.FILTERS)
    return sorted(axes)


_images, _expected = {}, {}


def source(w, h, n):
    if (w, h, n) not in _images:
        _images[w, h, n] = np.stack([R.content(w, h, "noise", seed=i) for i in range(n)])
    return _images[w, h, n]


def expected(w, h, ow, oh, n, filt):
    """The n restated outputs, computed once per shape: a pass treats the lines across it alike, so the images of a
    one-pass case go through the restatement side by side."""
    key = (w, h, ow, oh, n, filt)
    if key not in _expected:
        src = source(w, h, n)
        if oh == h:
            e = R.resample(src.reshape(n * h, w, 3), ow, n * h, filt).reshape(n, oh, ow, 3)
        elif ow == w:
            e = R.resample(np.concatenate(list(src), axis=1), n * w, oh, filt).reshape(oh, n, ow, 3).transpose(1, 0, 2, 3)
        else:
            e = np.stack([R.resample(s, ow, oh, filt) for s in src])
        _expected[key] = np.ascontiguousarray(e)
    return _expected[key]


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    exe = tmp_path_factory.mktemp("resamplehost") / "resample_kernel_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           "-isystem", os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "tests", "cpp", "resample_kernel_host.cpp"),
                           os.path.join(ROOT, "codec-eval_amd", "csrc", "ce_tables.cpp"), "-o", str(exe)])
    return str(exe)


class Reader:
    def __init__(self, path):
        self.raw, self.pos = np.fromfile(path, np.uint8), 0

    def take(self, count, dt):
        n = count * np.dtype(dt).itemsize
        assert self.pos + n <= self.raw.size, "the harness wrote less than its jobs need"
        a = self.raw[self.pos:self.pos + n].view(dt)
        self.pos += n
        return a


def check_table(rd, n_in, n_out, filt):
    """One dumped table against the restatement's taps; returns ksize."""
    ksize = int(rd.take(1, np.uint32)[0])
    tab = rd.take(n_out * (2 + ksize), np.int32)
    where = (n_in, n_out, filt)
    assert ksize == 2 * math.ceil(R.SUPPORT[filt] * max(n_in / n_out, 1.0)) + 1, where
    first, count, k = tab[:n_out], tab[n_out:2 * n_out], tab[2 * n_out:].reshape(n_out, ksize)
    assert (first >= 0).all() and (count <= ksize).all() and (first + count <= n_in).all(), where
    want = R.taps(n_in, n_out, filt)
    assert first.tolist() == [xmin for xmin, _ in want], where
    assert count.tolist() == [len(ks) for _, ks in want], where
    want_k = np.zeros((n_out, ksize), np.int64)  # zeros in the unused tail
    for xx, (_, ks) in enumerate(want):
        want_k[xx, :len(ks)] = ks
    assert np.array_equal(k, want_k), where
    return ksize


def run(host_kernel, tmp_path, lines, blob):
    (tmp_path / "jobs.txt").write_text("".join(line + "\n" for line in lines))
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([host_kernel, str(tmp_path / "jobs.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    out = r.stdout.split("\n")
    assert out[-2] == f"done {len(lines)}" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    passes = {}
    for line in out[:-2]:
        tag, job, axis, tiles, grid, lds_bytes, lds, empty = line.split()
        assert tag == "pass"
        passes[int(job), axis] = dict(tiles=int(tiles), grid=int(grid), lds_bytes=int(lds_bytes), lds=bool(int(lds)), empty=int(empty))
    return Reader(tmp_path / "out.bin"), passes


def test_host_tables_equal_the_restatement(host_kernel, tmp_path):
    jobs = table_jobs(cases())
    assert {(a, b) for a, b, _ in jobs} >= set(TABLE_AXES) and len(TABLE_AXES) == 19
    rd, _ = run(host_kernel, tmp_path, [f"table {a} {b} {f}" for a, b, f in jobs], b"")
    rows = 0
    for n_in, n_out, filt in jobs:
        check_table(rd, n_in, n_out, filt)
        rows += n_out
    assert rd.pos == rd.raw.size and rows > 40000


def test_host_build_of_the_kernels_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    lines = [f"case {w} {h} {ow} {oh} {n} {off} {filt}" for w, h, ow, oh, n, off, filt in cs]
    blob = b"".join(source(w, h, n).tobytes() for w, h, _, _, n, _, _ in cs)
    rd, passes = run(host_kernel, tmp_path, lines, blob)
    for job, (w, h, ow, oh, n, off, filt) in enumerate(cs):
        c = dict(job=job, w=w, h=h, out_w=ow, out_h=oh, n=n, off=off, filter=filt)
        assert ((job, "h") in passes) == (ow != w) and ((job, "v") in passes) == (oh != h), c
        if ow != w:
            ksize = check_table(rd, w, ow, filt)
            p = passes[job, "h"]
            # the launcher's geometry, stated once more from the header's constants
            fits = (2 + ksize) * TILE_PIXELS * 4 <= LDS_BYTES
            assert p["lds"] == fits and p["lds_bytes"] == ((2 + ksize) * TILE_PIXELS * 4 if fits else 0), c
            assert p["tiles"] == (3 * ow + 3 + TILE_BYTES - 1) // TILE_BYTES and p["grid"] == p["tiles"] * h * n, c
        if oh != h:
            check_table(rd, h, oh, filt)
            p = passes[job, "v"]
            assert not p["lds"] and p["lds_bytes"] == 0 and p["grid"] == p["tiles"] * oh * n, c
        got = rd.take(n * oh * ow * 3, np.uint8).reshape(n, oh, ow, 3)
        want = expected(w, h, ow, oh, n, filt)
        for i in range(n):
            assert np.array_equal(got[i], want[i]), {**c, "image": i}
    assert rd.pos == rd.raw.size

    # what the list is for, read from what the harness printed
    job_of = {c: j for j, c in enumerate(cs)}
    # an empty trailing tile: 341 pixels are 1023 row bytes, two tiles by the count's + 3, and at phase 0 the second holds none
    p = passes[job_of[(682, 1, 341, 1, 3, 0, R.LANCZOS3)], "h"]
    assert p["tiles"] == 2 and p["empty"] >= 1
    assert any(p["empty"] for (j, axis), p in passes.items() if axis == "v")
    # both tap routes, the boundary between them exactly where the launcher puts it
    for off in OFFSETS:
        staged = passes[job_of[(1840, 2, 345, 2, 2, off, R.LANCZOS3)], "h"]
        wide = passes[job_of[(1841, 2, 345, 2, 2, off, R.LANCZOS3)], "h"]
        assert staged["lds"] and staged["lds_bytes"] == 48020 and staged["tiles"] == 2
        assert not wide["lds"] and wide["lds_bytes"] == 0 and wide["tiles"] == 2
    assert (2 + 35) * TILE_PIXELS * 4 == 50764 > LDS_BYTES
    far = passes[job_of[(3700, 2, 684, 2, 2, 3, R.LANCZOS3)], "h"]
    assert not far["lds"] and far["tiles"] == 3
