"""The reference-state records of a batch (codec-eval_amd/csrc/ce_ref_state.h: plain C++, no device calls) against the
rebuild rules a launch relies on (tests/cpp/test_ref_state.cpp), as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer; and the new calls' place in the ABI."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ref_state_rules(tmp_path):
    exe = str(tmp_path / "test_ref_state")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_ref_state.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ref state OK" in out.stdout, out.stdout + out.stderr


def test_the_new_calls_refuse_null_and_are_bound(ce):
    import ctypes as C

    L = ce.lib()
    for name in ("ce_batch_references_changed", "ce_batch_ref_stats"):
        assert name in ce.ABI_SYMBOLS
    out = (C.c_uint32 * 3)()
    assert L.ce_batch_references_changed(None) == ce.CE_ERR_INVALID_ARG
    assert L.ce_batch_ref_stats(None, C.byref(out)) == ce.CE_ERR_INVALID_ARG
    assert hasattr(ce.Batch, "references_changed") and hasattr(ce.Batch, "ref_stats")
