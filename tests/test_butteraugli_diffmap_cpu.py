"""Butteraugli diffmaps without a GPU: the three entry points and CE_FLAG_BUTTERAUGLI_DIFFMAP agree across the header, the
Rust declarations and the ctypes layer and reject null handles; and the oracle's diffmap (the shim of ba_diffmap_shim.py,
which the GPU parity test compares the device's maps with) reduces to the oracle's own score and p-norm."""
import ctypes
import os
import re

import numpy as np
import pytest

import ba_diffmap_shim as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "ce_metrics.h")).read()
SYS = open(os.path.join(ROOT, "bindings", "rust", "codec-eval-hip", "src", "sys.rs")).read()
NEW = {"ce_calculate_butteraugli_diffmap": 10, "ce_batch_butteraugli_diffmap": 6, "ce_ref_butteraugli_diffmap": 6}


def test_declared_everywhere_with_the_same_arity(ce):
    header = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name, arity in NEW.items():
        c = re.search(r"\b" + name + r"\(([^;]*?)\);", header, flags=re.S)
        r = re.search(r"pub fn " + name + r"\((.*?)\)\s*->", SYS, flags=re.S)
        assert c and r, name
        assert len(c.group(1).split(",")) == arity and len([a for a in r.group(1).split(",") if a.strip()]) == arity, name
        assert name in ce.ABI_SYMBOLS and hasattr(ce.lib(), name)
        assert len(getattr(ce.lib(), name).argtypes) == arity
    assert int(re.search(r"CE_FLAG_BUTTERAUGLI_DIFFMAP\s*=\s*1u\s*<<\s*(\d+)", HEADER).group(1)) == 1
    assert int(re.search(r"pub const CE_FLAG_BUTTERAUGLI_DIFFMAP: u32 = 1 << (\d+);", SYS).group(1)) == 1
    assert ce.FLAG_BUTTERAUGLI_DIFFMAP == 1 << 1


def test_null_handles_are_invalid_arguments(ce):
    L = ce.lib()
    a = np.zeros(16 * 16 * 3, np.uint8)
    out = np.zeros(16 * 16, np.float32)
    score = ctypes.c_double()
    assert L.ce_calculate_butteraugli_diffmap(None, a.ctypes.data, a.size, a.ctypes.data, a.size, 16, 16, 80.0,
                                              ctypes.byref(score), out.ctypes.data) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_butteraugli_diffmap(None, 0, 1, 1, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG
    assert L.ce_ref_butteraugli_diffmap(None, 0, 1, 1, out.ctypes.data, out.size) == ce.CE_ERR_INVALID_ARG


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.Shim(tmp_path_factory.mktemp("ba_shim"))


@pytest.mark.parametrize("switches", [False, True], ids=["default", "device_switches"])
@pytest.mark.parametrize("w,h", [(97, 61), (9, 301), (64, 33)])
def test_shim_map_reduces_to_the_oracle_score(shim, workloads, oracle, w, h, switches):
    ref = workloads.make_reference(w, h, 40 + w)
    t = workloads.distort(ref, 55)
    shim.set_device_switches(switches)
    try:
        dm = shim.diffmap(ref, t, w, h)
        score, p3 = shim.score(ref, t, w, h)
    finally:
        shim.set_device_switches(False)
    assert dm.shape == (h, w) and dm.dtype == np.float32 and np.all(dm >= 0)
    assert float(dm.max()) == score
    assert abs(S.pnorm3(dm) - p3) <= 1e-13 * p3
    if not switches:  # this copy of the oracle is the oracle
        assert (score, p3) == oracle.butteraugli(ref, t, w, h)


def test_block_max_helper():
    dm = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
    got = S.block_max(dm, 4)
    assert got.shape == (2, 2)
    assert got.tolist() == [[dm[:4, :4].max(), dm[:4, 4:].max()], [dm[4:, :4].max(), dm[4:, 4:].max()]]
