"""The C++ mirror of src/viewing.rs (codec-eval_amd/host/codec_eval.hpp, namespace viewing) and the session's
simulate_viewing switch, compiled with plain g++ against the C ABI (tests/cpp/test_viewing_mirror.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(ce, tmp_path):
    exe = str(tmp_path / "test_viewing_mirror")
    libdir = os.path.dirname(ce.LIB_PATH)
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "host"),
        os.path.join(ROOT, "tests", "cpp", "test_viewing_mirror.cpp"), "-o", exe,
        "-L", libdir, "-lce_metrics_hip", f"-Wl,-rpath,{libdir}", "-pthread",
    ])
    return exe


def test_viewing_mirror_host_logic(ce, tmp_path):
    out = subprocess.run([_build(ce, tmp_path), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_viewing_mirror_on_gpu(ce, tmp_path):
    out = subprocess.run([_build(ce, tmp_path), "gpu"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
