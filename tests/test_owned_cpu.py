"""The move-only owners of device memory, page-locked memory, events and streams (codec-eval_amd/csrc/ce_owned.h) that the
batch and the metrics' working sets are made of: plain C++ over a handful of HIP calls, checked by tests/cpp/test_owned.cpp
as a stand-alone program, with counting stand-ins for those calls, under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owned(tmp_path):
    exe = str(tmp_path / "test_owned")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_owned.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "owned OK" in out.stdout, out.stdout + out.stderr
