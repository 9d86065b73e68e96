"""The region and rim index logic of Butteraugli's front end (codec-eval_amd/csrc/ba_front_geom.h: plain C++, no device
calls) against the tap-by-tap mirroring it replaces (tests/cpp/test_ba_front_geom.cpp), as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_front_geometry(tmp_path):
    exe = str(tmp_path / "test_ba_front_geom")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_ba_front_geom.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ba front geometry OK" in out.stdout, out.stdout + out.stderr
