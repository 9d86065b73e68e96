"""Butteraugli's LF term formed in the LF column blur (codec-eval_amd/csrc/butteraugli.hip: EPI_LF_TERM and Malta's `lf_term`
argument; ce_plan.h: ce_plan_ba_lf_term_in_blur).  A launch that finds its references' state kept writes one plane per
distorted slot - the finished term - instead of three LF planes, and Malta's epilogue reads it; the float is formed with the
epilogue's expressions in its order, so nothing may change a bit: every comparison here is == on bit patterns.

Per batch (tests/ba_lf_term_cases.py: 3 references, 7 pairs bound 1 / 2 / 4 and interleaved, at the edges of both kernels'
64 x 32 tiles, the smallest image the metric scores and an odd half-resolution level; the same pairs repeated to 64 distorted slots, where the
second launch is in slot order): launch 1 (old path), launch 2 (new path), reference 1 written again (state dropped), launch
3 (old path over planes the new path left), launch 4 (new path) - all four equal each other, equal a child process with
CE_BA_LF_TERM=0, and equal the oracle's diffmap and score with the two device switches on (tests/test_gpu_butteraugli.py),
its 3-norm within the tolerance of tests/test_gpu_ba_slot_order.py.  A depth-10 deep batch, a linear batch and a reference
handle's repeated compare: equal with the knob on and off."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_diffmap_shim as S  # noqa: E402
import ba_lf_term_cases as L  # noqa: E402
from test_gpu_ba_slot_order import PNORM_REL  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD_SCRIPT = r"""
import importlib, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import ba_lf_term_cases as L
ce = importlib.import_module("codec-eval_amd")
wl = importlib.import_module("codec-eval_amd.workloads")
ctx = ce.Context(0)
np.savez(sys.argv[1], **L.everything(ce, wl, ctx))
ctx.close()
""" % (ROOT, os.path.join(ROOT, "tests"))

RGB8 = [(w, h, len(L.BIND)) for w, h in L.SHAPES] + [L.MANY_SHAPE + (len(L.MANY),)]


@pytest.fixture(scope="module")
def knob_off(tmp_path_factory):
    """Every batch of the cases in a fresh context of a child with CE_BA_LF_TERM=0 (read once per process)."""
    npz = str(tmp_path_factory.mktemp("ba_lf_term") / "off.npz")
    env = dict(os.environ)
    env["CE_BA_LF_TERM"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD_SCRIPT, npz], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(npz)


@pytest.fixture(scope="module")
def knob_on(ce, workloads, gpu_ctx):
    assert os.environ.get("CE_BA_LF_TERM", "1")[:1] != "0", "this process must run the default path"
    return L.everything(ce, workloads, gpu_ctx)


@pytest.fixture(scope="module")
def shim(tmp_path_factory, oracle):
    ba = S.Shim(tmp_path_factory.mktemp("ba_lf_term_oracle"))
    ba.set_device_switches(True)
    yield ba
    ba.set_device_switches(False)


@pytest.fixture(scope="module")
def oracle_maps(workloads, shim):
    """The oracle's diffmap of each of the seven pairs, per shape, computed once."""
    out = {}
    for w, h in L.SHAPES:
        refs, tests = L.images(workloads, "rgb8", w, h)
        out[(w, h)] = [shim.diffmap(refs[r], tests[p], w, h) for p, r in enumerate(L.BIND)]
    return out


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def names(kind, w, h, n):
    k = L.key(kind, w, h, n)
    return [["%s-L%d-%s" % (k, launch, what) for what in ("score", "p3", "map")] for launch in range(4)], k + "-builds"


@pytest.mark.parametrize("kind,w,h,n", [("rgb8",) + c for c in RGB8] + [o + (len(L.BIND),) for o in L.OTHER], ids=lambda v: str(v))
def test_four_launches_agree_and_equal_the_knob_off_child(knob_on, knob_off, kind, w, h, n):
    per_launch, builds = names(kind, w, h, n)
    # launches 1 and 3 rebuilt the references' state (old path), 2 and 4 found it kept (new path unless the knob is off)
    assert knob_on[builds].tolist() == [1, 1, 2, 2] == knob_off[builds].tolist()
    for launch in range(4):
        for a, b in zip(per_launch[launch], per_launch[0]):
            assert same(knob_on[a], knob_on[b]), (a, b)
        for a in per_launch[launch]:
            assert same(knob_on[a], knob_off[a]), a
    assert knob_on[per_launch[0][2]].shape == (n, h, w)


@pytest.mark.parametrize("w,h,n", RGB8, ids=lambda v: str(v))
def test_every_launch_is_the_oracle(knob_on, oracle_maps, w, h, n):
    pick = L.MANY if n == len(L.MANY) else list(range(n))
    per_launch, _ = names("rgb8", w, h, n)
    for launch in range(4):
        score, p3, maps = (knob_on[a] for a in per_launch[launch])
        for p, u in enumerate(pick):
            want = oracle_maps[(w, h)][u]
            bad = np.argwhere(maps[p].view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (launch, p, len(bad), bad[:4].tolist())
            assert score.view(np.float64)[p] == float(want.max()), (launch, p)
            w_p3 = S.pnorm3(want)
            assert abs(p3.view(np.float64)[p] - w_p3) <= PNORM_REL["rgb8"] * abs(w_p3), (launch, p)


def test_a_one_pixel_image_is_refused_on_both_paths(ce, gpu_ctx):
    """Butteraugli needs 8 x 8 (the oracle refuses less, too): neither launch of a 1 x 1 batch reaches the kernels."""
    px = np.full((1, 1, 3), 100, np.uint8)
    b = ce.Batch(gpu_ctx, 1, 1, 1, 1)
    try:
        b.set_reference(0, px)
        b.set_test(0, 0, px + 20)
        for launch in range(2):
            s = b.run(1, ce.MetricConfig(butteraugli=True), 80.0, butteraugli_diffmap=True)
            assert s[0].status == ce.CE_ERR_TOO_SMALL, launch
    finally:
        b.close()


def test_a_reference_handle_compared_twice(knob_on, knob_off):
    for a in ("handle-score", "handle-map"):
        assert same(knob_on[a], knob_off[a]), a
    s, m = knob_on["handle-score"], knob_on["handle-map"]
    assert s[0] == s[1] and same(m[0], m[1])  # the compare that builds the state and the one that finds it
    assert s[2] != s[0]
