"""The launch-id decode of Butteraugli's per-slot kernels (codec-eval_amd/csrc/ba_slot_order.h: plain C++, no device calls):
every (tile, slot) exactly once in both orders, padding ids map to nothing, a slot's tiles share id % 8
(tests/cpp/test_ba_slot_order.cpp), as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ba_slot_order(tmp_path):
    exe = str(tmp_path / "test_ba_slot_order")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_ba_slot_order.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ba slot order OK" in out.stdout, out.stdout + out.stderr
