"""The deep content of tests/deep_content.py, the parts that need no GPU: the composed reference of
tests/test_gpu_deep_content.py (tests/deep_input_shim.py's tables, then tests/linear_input_shim.py) is the deep shim itself
with ==, every class is what it claims to be, the reference is finite on all of it, and - on the reference's own maps - each
mistake the content is aimed at moves something that the GPU test compares bit for bit."""
import math

import numpy as np
import pytest

import deep_content as DC
import deep_input_shim as D
import linear_input_shim as LS


@pytest.fixture(scope="module")
def shims(tmp_path_factory, oracle):
    return D.Shim(tmp_path_factory.mktemp("deep_content_deep_shim")), LS.Shim(tmp_path_factory.mktemp("deep_content_linear_shim"))


@pytest.fixture(scope="module")
def content():
    return {b: DC.cases(*b) for b in DC.BATCHES}


def batch_id(b):
    return "%dx%d-%d/%d" % b


def test_the_plan_is_the_stated_one():
    assert [w * h * 6 % 16 for w, h in DC.EDGE_SHAPES] == [2, 12, 4]  # slots 1 and up are not 16-byte aligned
    assert all(w * h * 6 % 16 == 0 for w, h in DC.ALIGNED_SHAPES)
    assert {(w, h) for w, h, _, _ in DC.BATCHES} == set(DC.SHAPES)
    for pairing in DC.PAIRINGS:  # every pairing at an unaligned edge shape; the equal depths and 8 / 10 at all of them
        at = {(w, h) for w, h, rd, td in DC.BATCHES if (rd, td) == pairing} & set(DC.EDGE_SHAPES)
        assert at == set(DC.EDGE_SHAPES) if pairing in DC.EQUAL + [(8, 10)] else len(at) >= 1, pairing
    assert {(w, h) for w, h, _, _ in DC.BRIGHT} == set(DC.SHAPES) and set(DC.BRIGHT) <= set(DC.BATCHES)  # 250 nits: one pairing per shape
    assert (200, 136, 16, 16) in DC.BATCHES and DC.can_cover(200, 136, 16) and not any(DC.can_cover(w, h, 16) for w, h in DC.SHAPES[:-1])


@pytest.mark.parametrize("b", DC.BATCHES, ids=batch_id)
def test_composed_reference_is_the_deep_shim(shims, content, b):
    """Table lookup, then the linear shim, equals the deep shim's three scores with ==; and no map holds a non-finite value."""
    w, h, rd, td = b
    deep, lin = shims
    cs = content[b]
    for intensity in (DC.INTENSITIES if b in DC.BRIGHT else DC.INTENSITIES[:1]):
        want = DC.expected(shims, cs, w, h, rd, td, intensity)
        for p, (name, ref, test) in enumerate(cs):
            where = (name, b, intensity)
            assert ref.dtype == test.dtype == np.uint16 and ref.shape == test.shape == (h, w, 3), where
            assert want.ssim2_default[p] == deep.ssimulacra2(ref, rd, test, td, w, h, 1), where
            assert want.dssim[p][0] == deep.dssim(ref, rd, test, td, w, h), where
            assert want.ba_default[p] == deep.butteraugli(ref, rd, test, td, w, h, intensity), where
            score, p3, dm = want.ba[p]
            assert math.isfinite(score) and math.isfinite(p3) and np.isfinite(dm).all(), where
            assert all(np.isfinite(m).all() and math.isfinite(s) for m, s in want.dssim[p][1]), where
            assert all(np.isfinite(d).all() and np.isfinite(e).all() and np.isfinite(f).all() for d, e, f in want.ssim2[p]), where
            if name == "identical":
                assert (want.dssim[p][0], want.ssim2_default[p], score) == (0.0, 100.0, 0.0), where
                assert rd != td or deep.sse(ref, test) == 0


@pytest.mark.parametrize("b", DC.BATCHES, ids=batch_id)
def test_every_class_is_what_it_claims(content, b):
    w, h, rd, td = b
    cs = {name: (ref, test) for name, ref, test in content[b]}
    n = 3 * w * h
    refs, tests, pair_ref = DC.grid(content[b])
    assert len(refs) >= 3 and len(tests) == len(content[b]) and all(p != r for p, r in enumerate(pair_ref))
    assert ("identical" in cs) == (rd == td or (rd, td) == (8, 16))
    if "identical" in cs:
        assert pair_ref[list(cs).index("identical")] == pair_ref[list(cs).index("lsb")]  # one reference, two distorted images
    for name, (ref, test) in cs.items():  # only extremes_over leaves the sides' ranges
        if name != "extremes_over":
            assert ref.max() <= DC.maxv(rd) and test.max() <= DC.maxv(td), name

    # every_entry: complete on every side with enough samples, there whenever one side has them, permuted
    assert ("every_entry" in cs) == (DC.can_cover(w, h, rd) or DC.can_cover(w, h, td))
    if "every_entry" in cs:
        for a, depth in zip(cs["every_entry"], (rd, td)):
            if DC.can_cover(w, h, depth):
                assert np.array_equal(np.unique(a), np.arange(1 << depth)), depth
        flat = cs["every_entry"][1].reshape(-1).astype(np.int64)
        assert np.mean(np.abs(np.diff(flat)) > DC.maxv(td) // 64) > 0.9  # not a ramp
        assert not np.array_equal(*cs["every_entry"])

    # bytes: no sample of the built side has two equal bytes, few of a requantised side; neighbours differ in both bytes
    for side, (a, depth) in enumerate(zip(cs["bytes"], (rd, td))):
        if depth == 8:
            continue
        hi, lo = a >> 8, a & 255
        built = depth == max(rd, td)
        assert np.mean(hi == lo) <= (DC.BYTES_EQUAL_SHARE_BUILT if built else DC.BYTES_EQUAL_SHARE_REQUANTISED), (side, float(np.mean(hi == lo)))
        if built:
            for part in (hi, lo):
                assert (part[:, 1:] != part[:, :-1]).all()  # horizontally adjacent samples of a channel
                assert (part[..., 0] != part[..., 1]).all() and (part[..., 1] != part[..., 2]).all() and (part[..., 0] != part[..., 2]).all()
            if depth < 16:
                assert np.mean(a >= 512) >= DC.BYTES_HIGH_BIT_SHARE
            assert not np.array_equal(a.byteswap(), a)

    # lsb: the stated share of samples, each by exactly one LSB of the test side
    ref, test = cs["lsb"]
    diff = test.astype(np.int64) - DC.requantise(ref, rd, td).astype(np.int64)
    assert set(np.unique(diff)) <= {-1, 0, 1} and abs(np.mean(diff != 0) - DC.LSB_SHARE) <= 1.0 / n

    # knee: both sides of the curve's boundary, and the first codes
    for a, depth in zip(cs["knee"], (rd, td)):
        k = DC.KNEE * DC.maxv(depth)
        assert (a < k).any() and (a > k).any() and a.min() == 0 and a.max() <= k + 9
        pool, drawn = set(DC.knee_pool(depth).tolist()), set(np.unique(a).tolist())
        assert drawn == pool if n >= 360 else drawn <= pool and len(drawn) >= 12

    # extremes: the four codes; the uploaded copy leaves the range on every side under 16 bits, the clamped one is `extremes`
    for a, depth in zip(cs["extremes"], (rd, td)):
        m = DC.maxv(depth)
        assert set(np.unique(a)) == {0, 1, m - 1, m}
    assert ("extremes_over" in cs) == (rd < 16 or td < 16)
    if "extremes_over" in cs:
        for a, c, depth in zip(cs["extremes_over"], cs["extremes"], (rd, td)):
            m = DC.maxv(depth)
            if depth < 16:
                assert (a == m + 1).any() and (a == 65535).any() and not (a == m).any()
            assert DC.clamp(a, depth).max() == m and np.array_equal(DC.clamp(a, depth), c)


# ---- the mistakes, applied to the composed reference -------------------------------------------------------------------
def everything(shims, r0, t0, r1, t1, w, h):
    """Every map that tests/test_gpu_deep_content.py compares bit for bit, from planes: one flat float32 array."""
    _, lin = shims
    lin.set_device_switches(True)
    try:
        dm = lin.butteraugli_map(r0, t0, w, h, 80.0)[2]
    finally:
        lin.set_device_switches(False)
    parts = [dm.reshape(-1)] + [m.reshape(-1) for m, _ in lin.dssim_maps(r1, t1, w, h)[1]] + [d.reshape(-1) for d, _, _ in lin.ssim2_maps(r0, t0, w, h)]
    return np.concatenate(parts)


def moved(shims, b, name, mistake, content):
    """Whether the reference's maps change, per metric family, when the distorted side of `name` is read through `mistake`:
    (samples, depth, table) -> planes in place of table[min(v, maxv)]."""
    w, h, rd, td = b
    deep, _ = shims
    ref, test = next((r, t) for n, r, t in content[b] if n == name)
    right = everything(shims, DC.planes(deep, ref, rd, 0), DC.planes(deep, test, td, 0), DC.planes(deep, ref, rd, 1), DC.planes(deep, test, td, 1), w, h)
    wrong = everything(shims, DC.planes(deep, ref, rd, 0), mistake(test, 0), DC.planes(deep, ref, rd, 1), mistake(test, 1), w, h)
    return int(np.sum(right.view(np.uint32) != wrong.view(np.uint32)))


def test_a_byte_swap_moves_the_maps_and_is_invisible_to_the_anchor(shims, content):
    deep, _ = shims
    b = (33, 35, 16, 16)
    swap = lambda a, rule: DC.planes(deep, a.byteswap(), 16, rule)
    assert moved(shims, b, "bytes", swap, content) > 0 and moved(shims, b, "lsb", swap, content) > 0
    anchor = (np.arange(33 * 35 * 3, dtype=np.uint16).reshape(35, 33, 3) % 256) * 257
    assert np.array_equal(anchor.byteswap(), anchor)  # v8 * 257: what the suite held before this content
    b = (65, 34, 12, 12)  # a truncation to one byte
    assert moved(shims, b, "bytes", lambda a, rule: DC.planes(deep, a & 255, 12, rule), content) > 0


@pytest.mark.parametrize("b", [(33, 35, 10, 10), (65, 34, 12, 12), (200, 136, 16, 16)], ids=batch_id)
def test_a_one_entry_table_offset_moves_the_maps(shims, content, b):
    deep, _ = shims
    td = b[3]
    off = lambda a, rule: deep.table(td, rule)[np.minimum(DC.clamp(a, td).astype(np.int64) + 1, DC.maxv(td))]
    for name in ("every_entry", "lsb", "knee"):
        assert moved(shims, b, name, off, content) > 0, name
    # one entry alone: the samples that hold a single code, read one entry up
    _, ref, test = next(c for c in content[b] if c[0] == "every_entry")
    code = int(test[0, 0, 0])
    one = lambda a, rule: deep.table(td, rule)[np.where(a == code, min(code + 1, DC.maxv(td)), a)]
    assert (test == code).sum() >= 1 and moved(shims, b, "every_entry", one, content) > 0


@pytest.mark.parametrize("b", [(33, 35, 8, 10), (66, 35, 16, 10), (65, 34, 12, 16), (33, 35, 8, 16)], ids=batch_id)
def test_the_wrong_sides_maxv_or_table_moves_the_maps(shims, content, b):
    deep, _ = shims
    rd, td = b[2], b[3]
    wrong_table = lambda a, rule: deep.table(rd, rule)[np.minimum(a, DC.maxv(rd))]  # the reference's table and maxv for the distorted side
    wrong_maxv = lambda a, rule: deep.table(td, rule)[np.minimum(a, DC.maxv(rd))]  # the right table, clamped to the reference's maxv
    for name in ("bytes", "lsb", "extremes"):
        assert moved(shims, b, name, wrong_table, content) > 0, name
    if td > rd:
        assert moved(shims, b, "extremes", wrong_maxv, content) > 0
    else:  # a larger maxv clamps nothing that is in range: only over-range samples show it
        over = next(t for n, _, t in content[b] if n == "extremes_over")
        assert (np.minimum(over, DC.maxv(rd)) > DC.maxv(td)).any()


@pytest.mark.parametrize("b", DC.BATCHES, ids=batch_id)
def test_ingest_mistakes_change_the_bytes(content, b):
    """The slab comparison of the GPU test is on bytes, so a mistake shows wherever it changes them: a copy that is off by
    one sample, and a wrong dword among the six that four RGBA16 pixels are repacked into."""
    w, h, rd, td = b
    for name, ref, test in content[b]:
        for a, depth in ((ref, rd), (test, td)):
            flat = DC.clamp(a, depth).reshape(-1)
            assert np.mean(np.roll(flat, 1) != flat) > 0.4, name  # off by one sample
            if flat.size % 2 == 0 and name in ("bytes", "every_entry", "knee", "gradient_noise", "blocky"):
                d = flat.view(np.uint32)
                d = d[:d.size // 6 * 6].reshape(-1, 6)
                for i in range(5):  # dword i taken for dword i + 1
                    assert np.mean(d[:, i] != d[:, i + 1]) > 0.9, (name, i)
