"""The device code of the float resampler (codec-eval_amd/csrc/resample_f32_kernel.h) compiled for the host and run under
AddressSanitizer and UBSan (tests/cpp/resample_f32_kernel_host.cpp): the same text the GPU runs, every thread of every block
of the grids the launcher's own geometry function returns, on tables, sources, an image between the passes, an LDS stand-in
(refilled with a sentinel per block) and destinations allocated at exactly their size.  The tap tables are the product's
(ce_build_resample_table_f64, ce_tables.cpp linked into the harness).  Output floats must equal the numpy restatement
(tests/resample_linear_restatement.py, pinned to Pillow in test_resample_linear_cpu.py) bit for bit, and the sanitizers must
see no access outside a buffer.  Nothing is loaded into Python under a sanitizer: the program has its own main.

The shapes sit where the index arithmetic changes: output rows of 3 * out_w floats next to 0, 1 and 2 tiles of 256 floats,
the last tap count that is staged in LDS (69) and the first that is not (71), each pass alone and both through the image
between them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_f32_host as H  # noqa: E402
import resample_linear_restatement as RL  # noqa: E402

TILE_FLOATS, TILE_PIXELS, LDS_BYTES = 256, 256 // 3 + 2, 48 * 1024
EDGE_WIDTHS = (1, 2, 85, 86, 170, 171, 172)  # 3, 6 | 255, 258 | 510, 513, 516 floats a row: the nearest rows on both sides of 1 and 2 tiles


def lds_bytes(ksize):
    return TILE_PIXELS * (8 * ksize + 8)


def cases():
    """(w, h, out_w, out_h, n, filter) of every kernel run."""
    out = []
    # tile edges, horizontal only: each width from twice and from (about) half as many pixels
    for ow in EDGE_WIDTHS:
        for w in (2 * ow, (ow + 1) // 2 if ow > 1 else 3):
            out.append((w, 3, ow, 3, 2, RL.LANCZOS3))
    for filt in (RL.BOX, RL.BILINEAR, RL.BICUBIC):
        for ow in (85, 86):
            out.append((2 * ow, 2, ow, 2, 2, filt))
            out.append((57, 2, ow, 2, 2, filt))
    # the route boundary: 336 -> 30 is ksize 69, the last that is staged; 345 -> 30 is ksize 71, the first that is not.  The
    # other filters stage at both.
    for filt in RL.FILTERS:
        for w in (336, 345):
            out.append((w, 2, 30, 2, 2, filt))
    out.append((2100, 1, 172, 1, 2, RL.LANCZOS3))  # global route, ksize 75, three tiles
    # the vertical pass alone
    for ow in EDGE_WIDTHS:
        for h, oh in ((1, 3), (7, 2), (5, 12)):
            out.append((ow, h, ow, oh, 2, RL.LANCZOS3))
    for filt in (RL.BOX, RL.BILINEAR, RL.BICUBIC):
        out.append((86, 7, 86, 2, 2, filt))
        out.append((85, 5, 85, 12, 2, filt))
    out.append((3, 301, 3, 5, 2, RL.LANCZOS3))  # ksize 363 down a column
    # both passes, through the image between them
    for filt in RL.FILTERS:
        out.append((100, 7, 300, 21, 3, filt))
        out.append((257, 129, 86, 43, 2, filt))
    out.append((1, 1, 5, 3, 1, RL.LANCZOS3))
    return out


_images, _expected = {}, {}


def source(w, h, n):
    if (w, h, n) not in _images:
        src = np.stack([RL.content(w, h, seed=i, negatives=True) for i in range(n)])
        src[0].reshape(-1)[::7] = np.float32(1023.0)  # next to the clamp: a negative lobe on one side overshoots it
        _images[w, h, n] = src
    return _images[w, h, n]


def expected(w, h, ow, oh, n, filt):
    key = (w, h, ow, oh, n, filt)
    if key not in _expected:
        src = source(w, h, n)
        if oh == h:  # a pass treats the lines across it alike: the images side by side
            e = RL.resample(src.reshape(n * h, w, 3), ow, n * h, filt).reshape(n, oh, ow, 3)
        elif ow == w:
            e = RL.resample(np.concatenate(list(src), axis=1), n * w, oh, filt).reshape(oh, n, ow, 3).transpose(1, 0, 2, 3)
        else:
            e = np.stack([RL.resample(s, ow, oh, filt) for s in src])
        _expected[key] = np.ascontiguousarray(e)
    return _expected[key]


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    return H.build(tmp_path_factory.mktemp("resamplef32host"))


def test_host_build_of_the_kernels_equals_the_restatement_with_no_stray_access(host_kernel, tmp_path):
    cs = cases()
    lines = [f"case {w} {h} {ow} {oh} {n} {filt}" for w, h, ow, oh, n, filt in cs]
    blob = b"".join(source(w, h, n).tobytes() for w, h, _, _, n, _ in cs)
    rd, passes = H.run(host_kernel, tmp_path, lines, blob)
    clamped = 0
    for job, (w, h, ow, oh, n, filt) in enumerate(cs):
        c = dict(job=job, w=w, h=h, out_w=ow, out_h=oh, n=n, filter=filt)
        assert ((job, "h") in passes) == (ow != w) and ((job, "v") in passes) == (oh != h), c
        if ow != w:
            ksize = H.check_table(rd, w, ow, filt)
            p = passes[job, "h"]
            fits = lds_bytes(ksize) <= LDS_BYTES  # the launcher's geometry, stated once more from the header's constants
            assert p["lds"] == fits and p["lds_bytes"] == (lds_bytes(ksize) if fits else 0), c
            assert p["tiles"] == (3 * ow + TILE_FLOATS - 1) // TILE_FLOATS and p["grid"] == p["tiles"] * h * n, c
            assert p["clamp"] == (oh == h), c
        if oh != h:
            H.check_table(rd, h, oh, filt)
            p = passes[job, "v"]
            assert not p["lds"] and p["lds_bytes"] == 0 and p["grid"] == p["tiles"] * oh * n and p["clamp"], c
        got = rd.take(n * oh * ow * 3, np.float32).reshape(n, oh, ow, 3)
        want = expected(w, h, ow, oh, n, filt)
        clamped += int((np.abs(want) == RL.LINEAR_MAX).sum())
        for i in range(n):
            assert np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32)), {**c, "image": i}
    assert rd.pos == rd.raw.size
    assert clamped > 0  # the clamp was reached, and matched

    # what the list is for, read from what the harness printed
    job_of = {c: j for j, c in enumerate(cs)}
    assert passes[job_of[(170, 3, 85, 3, 2, RL.LANCZOS3)], "h"]["tiles"] == 1  # 255 floats
    assert passes[job_of[(172, 3, 86, 3, 2, RL.LANCZOS3)], "h"]["tiles"] == 2  # 258
    assert passes[job_of[(340, 3, 170, 3, 2, RL.LANCZOS3)], "h"]["tiles"] == 2  # 510
    assert passes[job_of[(342, 3, 171, 3, 2, RL.LANCZOS3)], "h"]["tiles"] == 3  # 513
    staged = passes[job_of[(336, 2, 30, 2, 2, RL.LANCZOS3)], "h"]
    wide = passes[job_of[(345, 2, 30, 2, 2, RL.LANCZOS3)], "h"]
    assert staged["lds"] and staged["lds_bytes"] == lds_bytes(69) == 48720
    assert not wide["lds"] and wide["lds_bytes"] == 0 and lds_bytes(71) == 50112 > LDS_BYTES
    far = passes[job_of[(2100, 1, 172, 1, 2, RL.LANCZOS3)], "h"]
    assert not far["lds"] and far["tiles"] == 3
