"""What tests/test_gpu_extreme_shapes.py shares: the two axes that reach the launch code's limits.

Long thin images - a side past 65535, so that a coordinate, a tile row or a strip index needs more than 16 bits - and batches of
more than 65535 pairs, which no grid's y or z holds in one launch.  Content is workloads.make_reference / distort; every
oracle result is computed once per process and handed out unchanged.  The bounds are those of the tests that hold the same
call on ordinary shapes, named beside each check.  A helper, not a test."""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reference_reuse_cases import write_device  # noqa: E402,F401

wl = importlib.import_module("codec-eval_amd.workloads")

GRID_YZ_MAX = 65535           # ce_plan.h: ce_grid_yz_max
SLOTS_MAX = GRID_YZ_MAX       # ce_launch_slots_max: references + pairs of a launch with a main metric
BA_HEIGHT_MAX = 4 * 65535     # ce_ba_height_max
SSIM2_HEIGHT_MAX = 8 * 65535  # ce_ssim2_height_max

# ---- long thin images ------------------------------------------------------------------------------------------------------------
THIN_ALL = [(8, 65537), (65537, 8), (9, 65535), (65535, 9)]  # all three main metrics and PSNR
THIN_DSSIM = [(1, 65537), (65537, 1)]                        # DSSIM takes any size; the others need 8 x 8
THIN_SSIM = [(11, 65537), (65537, 11)]                       # SSIM at one level: one valid position across
THIN_MS_SSIM = [(161, 4099), (4099, 161)]                    # MS-SSIM at five levels: one valid position across at level 4
QUALITIES = (40, 90)
DEVICE_SWITCHES = ("ba_malta_f32", "ba_l2_early")            # tests/test_gpu_butteraugli.py


@functools.lru_cache(maxsize=None)
def thin_images(w, h):
    """-> (reference, [test at each of QUALITIES]), (h, w, 3) uint8, read-only."""
    ref = wl.make_reference(w, h, 7000 + w % 1000 + h % 1000)
    tests = [wl.distort(ref, q) for q in QUALITIES]
    for a in [ref] + tests:
        a.setflags(write=False)
    return ref, tests


_ORACLE = {}


def thin_oracle(O, w, h, metrics):
    """Per test image a dict of the oracle's results for `metrics` (a string of d, s, b): psnr always; dssim; ssimulacra2 and
    its averages; butteraugli (score, 3-norm) of the default oracle and with the two device switches on."""
    key = (w, h, metrics)
    if key not in _ORACLE:
        ref, tests = thin_images(w, h)
        out = []
        for t in tests:
            d = {"psnr": O.psnr(ref, t, w, h)}
            if "d" in metrics:
                d["dssim"] = O.dssim(ref, t, w, h)
            if "s" in metrics:
                d["ssimulacra2"], d["averages"] = O.ssimulacra2_detail(ref, t, w, h, 1)
            if "b" in metrics:
                assert O.variants_all_default()
                d["butteraugli"] = O.butteraugli(ref, t, w, h)
                for v in DEVICE_SWITCHES:
                    O.set_variant(v, 1)
                try:
                    d["butteraugli_device"] = O.butteraugli(ref, t, w, h)
                finally:
                    for v in DEVICE_SWITCHES:
                        O.set_variant(v, 0)
                assert O.variants_all_default()
            out.append(d)
        _ORACLE[key] = out
    return _ORACLE[key]


def check_psnr(got, want, what):
    assert got == want, (what, got, want)  # tests/test_gpu_parity.py: `==` the oracle


def check_dssim(got, want, what):
    # test_dssim_parity_shapes: planes are bit-identical, only the f64 summation order differs
    assert abs(got - want) <= 1e-9 * max(abs(want), 1e-6), (what, got, want)


def check_ssim2(got, got_avg, want, want_avg, what):
    # test_ssim2_parity_shapes
    assert got_avg.shape == want_avg.shape, what
    np.testing.assert_allclose(got_avg, want_avg, rtol=2e-6, atol=1e-12)
    assert abs(got - want) <= 1e-4 * max(abs(want), 1.0), (what, got, want)


def check_butteraugli(got, got_p3, same, base, what):
    # test_device_is_the_oracle_with_two_named_switches_bit_for_bit; got_p3 None: a leaf, which returns the score alone
    assert got == same[0], (what, got, same)
    assert abs(got - base[0]) <= 1e-6 * max(abs(base[0]), 1e-3), (what, got, base)
    if got_p3 is not None:
        assert abs(got_p3 - same[1]) <= 1e-13 * abs(same[1]), (what, got_p3, same)
        assert abs(got_p3 - base[1]) <= 1e-6 * max(abs(base[1]), 1e-3), (what, got_p3, base)


# ---- many pairs ------------------------------------------------------------------------------------------------------------------
MAX_REFS, K_TESTS, TWINS = 3, 7, 21  # pair p: test image p % 7 against reference p % 3, so pair p repeats pair p % 21
MAX_PAIRS = 65540
FITS = 65532                         # with 3 references: 65535 slots, the most a launch with a main metric takes
PAST = (65535, 65536, 65540)         # at and past a grid's y on their own, and past the slots with any reference
TAIL = (65530, 10)                   # first, count of the map readouts: they end at MAX_PAIRS


@functools.lru_cache(maxsize=None)
def many_images(w, h):
    """-> (3 references, 7 tests) (h, w, 3) uint8: test j is reference j % 3 distorted, so every pair differs from its reference
    and 14 of the 21 pairs set a test against another image's reference."""
    refs = [wl.make_reference(w, h, 7100 + r) for r in range(MAX_REFS)]
    tests = [wl.distort(refs[j % MAX_REFS], 30 + 9 * j) for j in range(K_TESTS)]
    return refs, tests


def fill_many(ce, b, refs, tests, n_pairs=MAX_PAIRS):
    """The references through set_reference; the test slab in one device write, K_TESTS images repeated; the bindings."""
    for r, a in enumerate(refs):
        b.set_reference(r, a)
    one = np.stack([np.ascontiguousarray(t).reshape(-1) for t in tests])  # [7, samples]
    slab = np.ascontiguousarray(np.tile(one, ((n_pairs + K_TESTS - 1) // K_TESTS, 1))[:n_pairs])
    write_device(ce, b.test_slab, slab)
    for p in range(n_pairs):
        b.bind_pair(p, p % MAX_REFS)


def score_rows(scores):
    """A list of ce_scores as an [n, 6] uint64 array: status, valid and the four doubles' bits - comparable with ==."""
    n = len(scores)
    out = np.empty((n, 6), np.uint64)
    out[:, 0] = [s.status & 0xFFFFFFFF for s in scores]
    out[:, 1] = [s.valid for s in scores]
    for k, name in enumerate(("dssim", "ssimulacra2", "butteraugli", "psnr")):
        out[:, 2 + k] = np.array([getattr(s, name) for s in scores], np.float64).view(np.uint64)
    return out


def assert_twins(rows, what):
    """Row p of an [n, ...] array equals row p % TWINS bit for bit."""
    rows = np.ascontiguousarray(rows)
    flat = rows.reshape(rows.shape[0], -1).view(np.uint8).reshape(rows.shape[0], -1)
    bad = np.flatnonzero((flat != flat[np.arange(rows.shape[0]) % TWINS]).any(axis=1))
    assert bad.size == 0, (what, len(bad), bad[:8].tolist())


def assert_twin_items(items, fields, what):
    """Results (MsSsim, Ciede2000, HdrFidelity) by their integer `fields`, from which the host finishes every double: item p
    equals item p % TWINS."""
    first = [tuple(getattr(it, f) for f in fields) for it in items[:TWINS]]
    bad = [p for p in range(TWINS, len(items)) if tuple(getattr(items[p], f) for f in fields) != first[p % TWINS]]
    assert not bad, (what, len(bad), bad[:8])


def refused(ce, call, *needles):
    """`call` raises the library's CE_ERR_INVALID_ARG with every needle in its message."""
    try:
        call()
    except ce.CodecEvalError as e:
        assert e.status == ce.CE_ERR_INVALID_ARG, (e.status, str(e))
        for s in needles:
            assert s in str(e), (s, str(e))
        return str(e)
    raise AssertionError("the call was not refused")
