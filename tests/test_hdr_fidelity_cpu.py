"""HDR fidelity's host side without a device (include/ce_metrics.h: ce_pq_code_thresholds, ce_hdr_fidelity_matrices; DESIGN.md
section 19): the library's host builders against the numpy restatement (tests/hdr_fidelity_restatement.py) to the bit, the
restatement against numbers from outside this code - ST 2084's published points, the PQ ingest's own table, BT.2100's ICtCp on
greys - and against the plain integer PSNR of the PQ code values it was ingested from."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cicp_restatement as R  # noqa: E402
import hdr_fidelity_restatement as F  # noqa: E402

import codec_eval_amd as ce  # noqa: E402

NINE = [(d, w) for d in F.DEPTHS for w in F.WHITES]


@pytest.mark.parametrize("depth,white", NINE)
def test_thresholds_equal_restatement_increase_and_invert_the_ingest(depth, white):
    t, want = ce.pq_code_thresholds(depth, white), F.thresholds(depth, white)
    maxv = (1 << depth) - 1
    assert t.dtype == np.float32 and t.shape == (maxv,) and np.array_equal(t.view(np.uint32), want.view(np.uint32))
    assert np.all(np.diff(t) > 0)  # strictly increasing in float32
    # the search inverts the PQ ingest exactly, on the library's own decode table
    decode = ce.transfer_table(ce.TRANSFER_PQ, depth, white)
    assert np.array_equal(np.searchsorted(t, decode, side="right"), np.arange(maxv + 1))
    assert np.array_equal(F.code(decode, depth, white), np.arange(maxv + 1))


def test_matrices_equal_restatement_to_the_bit():
    a, b = ce.hdr_fidelity_matrices()
    wa, wb = F.matrices()
    assert a.dtype == b.dtype == np.float32
    assert np.array_equal(a.view(np.uint32), wa.view(np.uint32)) and np.array_equal(b.view(np.uint32), wb.view(np.uint32))
    assert np.array_equal(b.astype(np.float64) * 4096.0, np.array(F.LMS_4096, np.float64))  # n / 4096 is exact in float32
    assert np.array_equal(b.astype(np.float64).sum(axis=1), np.ones(3))  # BT.2100: white stays white
    # A undoes the ingest's BT.2020 matrix: to float32's precision, and rows that keep white white
    assert np.max(np.abs(a.astype(np.float64) @ ce.colour_matrix(9).astype(np.float64) - np.eye(3))) < 2e-7
    assert np.max(np.abs(a.astype(np.float64).sum(axis=1) - 1.0)) < 2e-7


def test_host_builders_refuse_what_the_header_lists():
    out = np.empty(1 << 16, np.float32)
    L = ce.lib()
    for depth, white, n in ((8, 203.0, 255), (11, 203.0, 2047), (10, 203.0, 1024), (10, 0.0, 1023), (10, -1.0, 1023),
                            (10, math.inf, 1023), (10, math.nan, 1023)):
        assert L.ce_pq_code_thresholds(depth, white, out.ctypes.data, n) == ce.CE_ERR_INVALID_ARG, (depth, white, n)
    assert L.ce_pq_code_thresholds(10, 203.0, None, 1023) == ce.CE_ERR_INVALID_ARG
    assert L.ce_hdr_fidelity_matrices(None, out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert C.sizeof(ce.CeHdrScores) == 48
    for name in ("ce_batch_hdr_fidelity", "ce_eval_pair_hdr_fidelity", "ce_pq_code_thresholds", "ce_hdr_fidelity_matrices"):
        assert name in ce.ABI_SYMBOLS and hasattr(L, name)


@pytest.mark.parametrize("depth,white", NINE)
def test_code_anchors(depth, white):
    maxv = (1 << depth) - 1
    w32 = float(np.float32(white))
    assert F.code(np.float32(0.0), depth, white) == 0
    assert np.array_equal(F.code(np.array([-0.0, -1.0, -1024.0, np.nan, 1e-45], np.float32), depth, white), [0, 0, 0, 0, 0])
    assert F.code(np.float32(10000.0 / w32), depth, white) == maxv  # ST 2084's peak
    assert F.code(np.float32(1024.0), depth, white) == maxv  # CE_LINEAR_MAX lies above PQ's peak at every white from 80 up


def test_100_nits_is_code_520_at_depth_10():
    """ST 2084's signal for 100 cd/m2 is 0.508: 0.508 * 1023 = 519.7."""
    for white in F.WHITES:
        assert F.code(np.float32(100.0 / white), 10, white) == 520
    assert abs(R.pq_nits(520 / 1023) - 100.0) < 0.5


@pytest.mark.parametrize("depth,white", NINE)
def test_greys_have_no_chroma_beyond_one_code_step(depth, white):
    """r = g = b: A's and B's rows sum to 1, so L, M and S are the grey value to an ulp or two and their codes differ by at
    most one step; ct and cp of codes that differ by at most one step are bounded by their largest coefficients."""
    g = np.linspace(0.0, 40.0, 1000).astype(np.float32)
    _, lms = F.codes(np.stack([g, g, g], axis=-1), depth, white)
    spread = lms.max(axis=-1) - lms.min(axis=-1)
    assert spread.max() <= 1
    _, ct, cp = F.ictcp(lms)
    assert np.abs(ct).max() <= 13613 and np.abs(cp).max() <= 17933
    print(f"depth {depth} white {white}: spread of the L, M, S codes over 1000 greys up to 40.0: {spread.max()}")
    assert np.all(ct[spread == 0] == 0) and np.all(cp[spread == 0] == 0)  # the coefficients of Ct and of Cp sum to 0


@pytest.mark.parametrize("depth,white", [(10, 80.0), (12, 203.0), (16, 10000.0)])
def test_identical_images_score_nothing(depth, white):
    rng = np.random.default_rng(5)
    img = (rng.random((9, 7, 3), np.float32) * np.float32(30.0) - np.float32(1.0)).astype(np.float32)
    f = F.fidelity(img, img.copy(), depth, white)
    assert (f["pq_sse"], f["itp_sum_q20"], f["itp_max_q20"]) == (0, 0, 0)
    assert f["pq_psnr"] == math.inf and f["delta_e_itp_mean"] == 0.0 and f["delta_e_itp_max"] == 0.0


def test_one_code_step_of_intensity_is_the_published_delta_e():
    """BT.2124: Delta E ITP = 720 * sqrt(dI^2 + dT^2 + dP^2).  A grey that moves by one 10-bit code in L, M and S moves I by
    1 / 1023 and leaves T and P alone: 720 / 1023."""
    t = F.thresholds(10, 203.0)
    a = np.full((1, 1, 3), (t[499] + t[500]) / 2, np.float32)  # inside code 500's interval
    b = np.full((1, 1, 3), (t[500] + t[501]) / 2, np.float32)  # ... and 501's
    f = F.fidelity(a, b, 10, 203.0)
    assert f["pq_sse"] == 3
    assert abs(f["delta_e_itp_max"] - 720.0 / 1023.0) <= 2.0 ** -20 and f["delta_e_itp_mean"] == f["delta_e_itp_max"]


@pytest.mark.parametrize("white", F.WHITES)
def test_pq_psnr_agrees_with_the_integer_psnr_of_the_code_values(white):
    """A 96 x 64 BT.2020 PQ pair at depth 16 - uniform random codes on the reference, uniform noise of +-300 codes on the test,
    the reference drawn from [300, 65235] so that the noise stays uniform - ingested through cicp_restatement.to_linear: the
    restatement's pq_psnr lies within 1e-3 dB of the plain integer PSNR of the code values.  The margin covers codes that
    flip after the float32 matrix round trip (BT.2020 -> sRGB primaries on ingest, A back): a dark channel beside a bright
    one comes back with the bright one's rounding error.  Measured on the definition with this seed: 1.3e-4, 1.4e-4 and
    4.6e-4 dB at white 80, 203 and 10000; over two other seeds 7e-5 .. 7.6e-4."""
    rng = np.random.default_rng(2124)
    for w in F.WHITES:  # one stream for the three whites, so that a white's pair does not depend on which tests ran
        ref = rng.integers(300, 65536 - 300, (64, 96, 3))
        test = ref + rng.integers(-300, 301, ref.shape)
        if w == white:
            break
    f = F.fidelity(R.to_linear(ref.astype(np.uint16), 9, 16, 16, white), R.to_linear(test.astype(np.uint16), 9, 16, 16, white), 16, white)
    mse = float(((ref - test) ** 2).sum()) / ref.size
    plain = 10.0 * math.log10(65535.0 ** 2 / mse)
    print(f"white {white}: pq_psnr {f['pq_psnr']!r}, integer PSNR {plain!r}, apart {abs(f['pq_psnr'] - plain):.2e} dB")
    assert abs(f["pq_psnr"] - plain) <= 1e-3
