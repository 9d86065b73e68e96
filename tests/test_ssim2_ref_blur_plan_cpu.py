"""Which blur passes an SSIMULACRA2 launch runs (codec-eval_amd/csrc/ce_plan.h: ce_plan_ssim2_ref_blur) and the record of the
references' final planes (ce_ref_state.h: CE_REF_SSIM2_BLUR), both plain C++ without device calls, checked by
tests/cpp/test_ssim2_ref_blur_plan.cpp as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ssim2_ref_blur_plan(tmp_path):
    exe = str(tmp_path / "test_ssim2_ref_blur_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_ssim2_ref_blur_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ssim2 ref blur plan OK" in out.stdout, out.stdout + out.stderr
