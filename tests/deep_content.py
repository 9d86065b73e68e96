"""Deep content for deep batches: deterministic uint16 pairs, each side at its own depth, aimed at the
mistakes that the two anchors of tests/test_gpu_deep_input.py (depths 8 / 8, and a 16-bit image holding v8 * 257) cannot see.
Shared by tests/test_deep_content_cpu.py and tests/test_gpu_deep_content.py.

Every generator takes (w, h, rd, td, seed) and returns a list of (name, ref, test), uint16 [h, w, 3]: the arrays as they are
UPLOADED.  Only `extremes_over` holds samples above a side's maxv = 2^depth - 1; clamp() gives what the slab then holds.  The
reference of a deep batch is, by definition, the oracle's stages run on table(depth, rule)[min(v, maxv)]: expected() composes
tests/deep_input_shim.py's tables with tests/linear_input_shim.py, which returns every map from float planes.
"""
import collections

import numpy as np

import deep_input_shim as D

EDGE_SHAPES = [(33, 35), (65, 34), (66, 35)]  # last tiles of 1 and 2 columns, half-resolution levels 17, 33 and 33 wide; w * h * 6 mod 16 = 2, 12, 4
ALIGNED_SHAPES = [(12, 10), (200, 136)]  # under 16 x 16; multi-tile, the only shape with 65 536 samples and more
SHAPES = EDGE_SHAPES + [(12, 10), (8, 8), (200, 136)]
EQUAL = [(10, 10), (12, 12), (16, 16)]
PAIRINGS = EQUAL + [(8, 10), (8, 16), (16, 10), (12, 16)]
# (w, h, rd, td): the equal depths and 8 / 10 at every edge shape, every other pairing at one unaligned edge shape, two pairings at
# each of the other shapes
BATCHES = ([(w, h, rd, td) for w, h in EDGE_SHAPES for rd, td in EQUAL + [(8, 10)]]
           + [(33, 35, 8, 16), (66, 35, 16, 10), (65, 34, 12, 16)]
           + [(12, 10, 12, 12), (12, 10, 16, 10), (8, 8, 10, 10), (8, 8, 12, 16), (200, 136, 16, 16), (200, 136, 8, 16)])
BRIGHT = [(33, 35, 8, 10), (65, 34, 12, 12), (66, 35, 16, 16), (12, 10, 16, 10), (8, 8, 10, 10), (200, 136, 16, 16)]  # also at 250 nits
INTENSITIES = (80.0, 250.0)
RUNS = [(*b, 80.0) for b in BATCHES] + [(*b, 250.0) for b in BRIGHT]

# the conditions tests/test_deep_content_cpu.py holds the classes to
BYTES_EQUAL_SHARE_BUILT = 0.0  # `bytes`, the side the pattern is built on: samples whose high and low bytes are equal
BYTES_EQUAL_SHARE_REQUANTISED = 0.02  # ... and the coarser side of a mixed pair, requantised from it (depth above 8)
BYTES_HIGH_BIT_SHARE = 0.4  # `bytes` at 10 and 12 bits: samples with a bit above bit 8 set (codes >= 512)
LSB_SHARE = 0.25  # `lsb`: the share of samples moved by one LSB of the test side's depth
KNEE = 0.04045  # the sRGB curve's select boundary
Reference = collections.namedtuple("Reference", "ba ba_default dssim ssim2 ssim2_default")  # tests/test_gpu_wide_content.py: Reference


def maxv(depth):
    return (1 << depth) - 1


def clamp(a, depth):
    """What ingest leaves in the slab: samples above maxv become maxv."""
    return np.minimum(np.asarray(a, np.uint16), np.uint16(maxv(depth)))


def requantise(a, d_from, d_to):
    """round(v * maxv(d_to) / maxv(d_from)) in integers."""
    if d_from == d_to:
        return np.asarray(a, np.uint16).copy()
    m_from, m_to = maxv(d_from), maxv(d_to)
    return ((np.asarray(a, np.int64) * m_to * 2 + m_from) // (2 * m_from)).astype(np.uint16)


def _seed(w, h, rd, td, seed):
    return [seed, w, h, rd, td]


def _sides(fine, rd, td, coarse):
    """(ref, test) from the image built at the finer depth and its coarser counterpart; at equal depths the test is the built one."""
    return (coarse, fine) if td >= rd else (fine, coarse)


def can_cover(w, h, depth):
    return 3 * w * h >= (1 << depth)


def every_entry(w, h, rd, td, seed):
    """Every code 0 .. maxv of a side occurs at least once across the three channels, on every side with 3 w h >= 2^depth;
    permuted, not ramped.  Built on the finer side: its covering codes (all of them, or - with too few samples for that - the
    ones that requantise onto every code of the coarser side) plus random codes, shuffled.  The coarser side is that,
    requantised; at equal depths the reference is the test with bit 0 flipped on the covering samples (a bijection of the
    codes, one LSB of error) and +-(maxv / 128) of noise on the rest; at unequal depths the rest carries that noise too."""
    rng = np.random.default_rng(_seed(w, h, rd, td, seed))
    n = 3 * w * h
    df, dc = max(rd, td), min(rd, td)
    if can_cover(w, h, df):
        cover = np.arange(1 << df, dtype=np.int64)
    elif can_cover(w, h, dc):
        cover = requantise(np.arange(1 << dc), dc, df).astype(np.int64)
    else:
        return []
    rest = rng.integers(0, 1 << df, n - cover.size)
    order = rng.permutation(n)
    fine = np.concatenate([cover, rest])[order]
    amp = max(2, maxv(df) // 128)
    noisy = np.clip(fine + rng.integers(-amp, amp + 1, n), 0, maxv(df))
    covering = (np.arange(n) < cover.size)[order]
    if df == dc:
        coarse = np.where(covering, fine ^ 1, noisy)
    else:
        coarse = requantise(np.where(covering, fine, noisy), df, dc)
    shape = (h, w, 3)
    ref, test = _sides(fine.astype(np.uint16).reshape(shape), rd, td, coarse.astype(np.uint16).reshape(shape))
    return [("every_entry", ref, test)]


def bytes_pattern(w, h, depth, rng):
    """Codes whose high byte steps through its range from sample to sample and whose low byte runs against it (255 - the high
    byte, scaled, plus noise of +-3): R, G and B of a pixel and horizontally adjacent samples differ in both bytes, and no
    sample has two equal bytes.  At depth 8 there is one byte: it takes the low byte's place."""
    n = 3 * w * h
    i = np.arange(n, dtype=np.int64)
    high_codes = 1 << max(depth - 8, 0)
    step = {1: 0, 4: 1, 16: 5, 256: 37}[high_codes]
    hi = (i * step) % high_codes
    lo = 255 - hi * 255 // max(high_codes - 1, 1) if high_codes > 1 else (i * 37) % 256
    lo = np.clip(lo + rng.integers(-3, 4, n), 0, 255)
    lo = np.where((lo == hi) & (high_codes > 1), lo ^ 4, lo)
    return hi, lo


def bytes_(w, h, rd, td, seed):
    rng = np.random.default_rng(_seed(w, h, rd, td, seed))
    df, dc = max(rd, td), min(rd, td)
    hi, lo = bytes_pattern(w, h, df, rng)
    fine = (hi << 8) | lo
    lo2 = np.clip(lo + rng.integers(-2, 3, lo.size), 0, 255)  # the other side: noise in the low byte only
    lo2 = np.where((lo2 == hi) & (df > 8), lo2 ^ 4, lo2)
    other = (hi << 8) | lo2
    shape = (h, w, 3)
    coarse = other if df == dc else requantise(other, df, dc)
    ref, test = _sides(fine.astype(np.uint16).reshape(shape), rd, td, coarse.astype(np.uint16).reshape(shape))
    return [("bytes", ref, test)]


def ramp(w, h, depth):
    y, x = np.mgrid[0:h, 0:w]
    m = maxv(depth)
    return np.stack([(x * m) // max(w - 1, 1), (y * m) // max(h - 1, 1), ((x + y) * m) // max(w + h - 2, 1)], axis=-1).astype(np.uint16)


def lsb_test(ref, rd, td, rng):
    """ref at the test side's depth with exactly round(LSB_SHARE * samples) samples moved by one LSB of that depth."""
    base = requantise(ref, rd, td).astype(np.int64).reshape(-1)
    moved = rng.permutation(base.size)[:int(round(LSB_SHARE * base.size))]
    step = rng.choice([-1, 1], moved.size)
    step = np.where(base[moved] == 0, 1, np.where(base[moved] == maxv(td), -1, step))
    base[moved] += step
    return base.astype(np.uint16).reshape(ref.shape)


def lsb(w, h, rd, td, seed):
    """A smooth two-way ramp; the test moves LSB_SHARE of its samples by +-1 LSB of its own depth.  At equal depths, and at
    8 / 16, the ramp is also the reference of `identical` (the same array: one slot, two distorted images)."""
    rng = np.random.default_rng(_seed(w, h, rd, td, seed))
    ref = ramp(w, h, rd)
    out = [("lsb", ref, lsb_test(ref, rd, td, rng))]
    if rd == td:
        out.append(("identical", ref, ref.copy()))
    elif (rd, td) == (8, 16):
        out.append(("identical", ref, ref * np.uint16(257)))
    return out


def knee_pool(depth):
    k = int(round(KNEE * maxv(depth)))
    return np.concatenate([np.arange(max(k - 8, 0), k + 9), np.arange(0, 17)])  # 34 codes


def knee(w, h, rd, td, seed):
    """Codes within +-8 of 0.04045 * maxv - where the curve selects between its linear and its power segment - and 0 .. 16,
    as noise; the test draws the neighbouring entry of its own pool at a third of the samples."""
    rng = np.random.default_rng(_seed(w, h, rd, td, seed))
    pr, pt = knee_pool(rd), knee_pool(td)
    idx = rng.integers(0, pr.size, (h, w, 3))
    move = rng.integers(-1, 2, idx.shape)
    return [("knee", pr[idx].astype(np.uint16), pt[np.clip(idx + move, 0, pt.size - 1)].astype(np.uint16))]


def extremes(w, h, rd, td, seed):
    """0, 1, maxv - 1 and maxv: 4 x 4 blocks that rotate per channel in the upper half, one-pixel checkers of 0 / maxv and
    1 / maxv - 1 below; the test swaps 0 <-> 1 and maxv - 1 <-> maxv on a sparse lattice.  `extremes_over` is the same pair as
    uploaded with samples above maxv on every side under 16 bits: maxv + 1 and 65535 in place of maxv, alternately."""
    y, x = np.mgrid[0:h, 0:w]
    blocks = np.stack([(x // 4 + y // 4 + c) % 4 for c in range(3)], axis=-1)
    checker = np.where(x < w // 2, ((x + y) % 2) * 3, 1 + (x + y) % 2)[..., None].repeat(3, axis=-1)
    idx = np.where((y < h // 2)[..., None], blocks, checker)
    tidx = idx.copy()
    tidx[2::5, 3::7] ^= 1

    def values(i, depth):
        return np.array([0, 1, maxv(depth) - 1, maxv(depth)], np.uint16)[i]

    def over(a, depth):
        if depth == 16:
            return a
        top = a == maxv(depth)
        return np.where(top & ((x + y) % 2 == 0)[..., None], np.uint16(maxv(depth) + 1), np.where(top, np.uint16(65535), a)).astype(np.uint16)

    ref, test = values(idx, rd), values(tidx, td)
    out = [("extremes", ref, test)]
    if rd < 16 or td < 16:
        out.append(("extremes_over", over(ref, rd), over(test, td)))
    return out


def gradient_noise(w, h, rd, td, seed):
    return [("gradient_noise", *D.gradient_noise_pair(w, h, rd, td, seed))]


def blocky(w, h, rd, td, seed):
    return [("blocky", *D.blocky_pair(w, h, rd, td, seed))]


CLASSES = {"every_entry": every_entry, "bytes": bytes_, "lsb": lsb, "knee": knee, "extremes": extremes, "gradient_noise": gradient_noise,
           "blocky": blocky}
SEED = 20


def cases(w, h, rd, td):
    """Every class at one shape and pairing: the pairs of one deep batch."""
    return [case for gen in CLASSES.values() for case in gen(w, h, rd, td, SEED)]


def replacement(cs, w, h, rd, td):
    """(pair index, (name, ref, new test)): another distorted image for the `lsb` pair - the ramp moved at other samples - on
    the reference slot it keeps."""
    p = next(i for i, c in enumerate(cs) if c[0] == "lsb")
    ref = cs[p][1]
    return p, ("lsb_replaced", ref, lsb_test(ref, rd, td, np.random.default_rng(_seed(w, h, rd, td, SEED + 1))))


def grid(cs):
    """-> refs, tests, pair_ref: the cases as the pairs of one batch, pair p being case p.  Cases that share a reference array
    share a slot - at least three references per batch - and the slots are numbered from the last case back, rotated by the
    first amount at which no pair sits at its reference's index: the pairs are bound out of order."""
    distinct = []
    for _, ref, _ in cs:
        if not any(r is ref for r in distinct):
            distinct.append(ref)
    assert len(distinct) >= 3
    for k in range(2 * len(distinct)):  # ... or, where every such numbering has a fixed point, from the first case on
        order = distinct[::-1] if k < len(distinct) else distinct
        k %= len(distinct)
        refs = order[k:] + order[:k]
        pair_ref = [next(i for i, r in enumerate(refs) if r is ref) for _, ref, _ in cs]
        if all(p != r for p, r in enumerate(pair_ref)):
            return refs, [t for _, _, t in cs], pair_ref
    raise AssertionError("no rotation binds every pair off its own index")


def planes(deep_shim, a, depth, rule):
    """table(depth, rule)[min(v, maxv)]: float32 [h, w, 3]"""
    return deep_shim.table(depth, rule)[clamp(a, depth)]


def expected(shims, cs, w, h, rd, td, intensity, fixed=None):
    """What a deep batch of depths (rd, td) must return for `cs`: tests/test_gpu_wide_content.py's Reference, from the tables
    (rule 0 for SSIMULACRA2 and Butteraugli, rule 1 for DSSIM) and the linear shim - Butteraugli's map with the oracle's two
    device switches on, the default scores with them off.  `fixed`: the (dssim, ssim2, ssim2_default) part of an earlier call
    for the same cases, which does not depend on the intensity target."""
    deep, lin = shims
    p0 = [(planes(deep, r, rd, 0), planes(deep, t, td, 0)) for _, r, t in cs]
    if fixed is None:
        p1 = [(planes(deep, r, rd, 1), planes(deep, t, td, 1)) for _, r, t in cs]
        fixed = ([lin.dssim_maps(r, t, w, h) for r, t in p1], [lin.ssim2_maps(r, t, w, h) for r, t in p0],
                 [lin.ssimulacra2(r, t, w, h, 1) for r, t in p0])
    default = [lin.butteraugli(r, t, w, h, intensity) for r, t in p0]
    lin.set_device_switches(True)
    try:
        on = [lin.butteraugli_map(r, t, w, h, intensity) for r, t in p0]
    finally:
        lin.set_device_switches(False)
    return Reference(on, default, *fixed)
