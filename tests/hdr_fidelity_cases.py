"""The pairs the HDR fidelity tests score (tests/test_hdr_fidelity_kernel_host_cpu.py on the host build of the kernel,
tests/test_gpu_hdr_fidelity.py on the device): shapes that take the scalar path (1 x 1, 5 x 3 and 97 x 35: byte sizes that are
no multiple of 16), the wide path (96 x 64) and several blocks a pair (512 x 256), every depth and every white among each
shape's parameters, and for content PQ images as an HDR10 decoder hands them over plus the classes of tests/wide_content.py:
negatives, values above PQ's peak, subnormals.  A helper, not a test."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402
import wide_content as WC  # noqa: E402

# three of the nine (depth, white_nits) pairs per shape, rotated so that every shape meets every depth and every white
PARAMS = [tuple((F.DEPTHS[i], F.WHITES[(i + k) % 3]) for i in range(3)) for k in range(3)]


def pq_pair(w, h, depth, white, seed, noise=40):
    """A BT.2020 PQ pair of `depth` bits as integer code values [h, w, 3] uint16: uniform codes, and uniform noise of +-noise."""
    rng = np.random.default_rng(seed)
    maxv = (1 << depth) - 1
    ref = rng.integers(0, maxv + 1, (h, w, 3))
    test = np.clip(ref + rng.integers(-noise, noise + 1, ref.shape), 0, maxv)
    return ref.astype(np.uint16), test.astype(np.uint16)


def pq_linear(w, h, depth, white, seed, noise=40):
    """... ingested as the library's CICP ingest defines it (tests/cicp_restatement.py): float32 [h, w, 3]."""
    ref, test = pq_pair(w, h, depth, white, seed, noise)
    return R.to_linear(ref, 9, 16, depth, white), R.to_linear(test, 9, 16, depth, white)


def _crop(pair, w, h):
    name, ref, test = pair
    return name, np.ascontiguousarray(ref[:h, :w]), np.ascontiguousarray(test[:h, :w])


@functools.lru_cache(maxsize=None)
def shape_cases():
    """-> [(w, h, params, [(name, ref, test)])]: the pairs of one batch per shape, scored at each of `params`."""
    wide = WC.working_set()
    out = []
    # 1 x 1 and 5 x 3: the corner of every wide-content class (logramp's starts at the smallest subnormal) and a PQ pixel
    for k, (w, h) in enumerate(((1, 1), (5, 3))):
        pairs = [_crop(c, w, h) for c in wide] + [("pq",) + pq_linear(w, h, 12, 203.0, 10 + k)]
        out.append((w, h, PARAMS[k], pairs))
    out.append((WC.ODD_W, WC.ODD_H, PARAMS[2], WC.odd_set() + [("pq",) + pq_linear(WC.ODD_W, WC.ODD_H, 10, 80.0, 12)]))
    out.append((WC.W, WC.H, PARAMS[0], wide + [("pq",) + pq_linear(WC.W, WC.H, 16, 10000.0, 13, noise=300)]))
    # 512 x 256: 128 blocks' worth of four-pixel groups; with 17 pairs a pair gets 64 blocks and a lane two groups
    big = [("pq%d" % i,) + pq_linear(512, 256, 16, 203.0, 20 + i, noise=300) for i in range(2)]
    big += [("hdr_noise",) + tuple(WC.hdr_noise(512, 256)[0][1:]), ("logramp",) + tuple(WC.logramp(512, 256)[0][1:])]
    out.append((512, 256, PARAMS[1], [big[i % len(big)] for i in range(17)]))
    return out


@functools.lru_cache(maxsize=None)
def expected(shape_index: int, depth: int, white: float):
    """The restatement's scores of every pair of a shape, computed once and shared."""
    _, _, _, pairs = shape_cases()[shape_index]
    memo, out = {}, []
    for _, ref, test in pairs:
        key = (id(ref), id(test))
        if key not in memo:
            memo[key] = F.fidelity(ref, test, depth, white)
        out.append(memo[key])
    return out
