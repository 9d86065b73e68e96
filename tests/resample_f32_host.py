"""Builds and runs tests/cpp/resample_f32_kernel_host.cpp: the float resampler's device code (resample_f32_kernel.h) and
its host table (ce_tables.cpp: ce_build_resample_table_f64) as a stand-alone program under AddressSanitizer and UBSan.
Shared by test_resample_f32_kernel_host_cpu.py (the kernels) and test_resample_linear_cpu.py (the tables)."""
import math
import os
import subprocess

import numpy as np

import resample_linear_restatement as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")  # ce_tables.cpp includes ce_internal.h, which includes the HIP runtime's header


def build(directory):
    exe = os.path.join(str(directory), "resample_f32_kernel_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fno-strict-aliasing",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "codec-eval_amd", "csrc"),
                           "-isystem", os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "tests", "cpp", "resample_f32_kernel_host.cpp"),
                           os.path.join(ROOT, "codec-eval_amd", "csrc", "ce_tables.cpp"), "-o", exe])
    return exe


class Reader:
    def __init__(self, path):
        self.raw, self.pos = np.fromfile(path, np.uint8), 0

    def take(self, count, dt):
        n = count * np.dtype(dt).itemsize
        assert self.pos + n <= self.raw.size, "the harness wrote less than its jobs need"
        a = self.raw[self.pos:self.pos + n].view(dt)
        self.pos += n
        return a


def run(exe, tmp_path, lines, blob):
    (tmp_path / "jobs.txt").write_text("".join(line + "\n" for line in lines))
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "jobs.txt"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    out = r.stdout.split("\n")
    assert out[-2] == f"done {len(lines)}" and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    passes = {}
    for line in out[:-2]:
        tag, job, axis, tiles, grid, lds_bytes, lds, clamp = line.split()
        assert tag == "pass"
        passes[int(job), axis] = dict(tiles=int(tiles), grid=int(grid), lds_bytes=int(lds_bytes), lds=bool(int(lds)), clamp=bool(int(clamp)))
    return Reader(tmp_path / "out.bin"), passes


def check_table(rd, n_in, n_out, filt):
    """One dumped table against the restatement's taps, every weight by its bits; returns ksize."""
    ksize = int(rd.take(1, np.uint32)[0])
    head = rd.take(2 * n_out, np.int32)
    k = rd.take(n_out * ksize, np.float64).reshape(n_out, ksize)
    where = (n_in, n_out, filt)
    assert ksize == 2 * math.ceil(RL.SUPPORT[filt] * max(n_in / n_out, 1.0)) + 1, where
    first, count = head[:n_out], head[n_out:]
    assert (first >= 0).all() and (count <= ksize).all() and (first + count <= n_in).all(), where
    want = RL.taps(n_in, n_out, filt)
    assert first.tolist() == [xmin for xmin, _ in want], where
    assert count.tolist() == [len(ws) for _, ws in want], where
    want_k = np.zeros((n_out, ksize), np.float64)  # zeros in the unused tail
    for xx, (_, ws) in enumerate(want):
        want_k[xx, :len(ws)] = ws
    assert np.array_equal(k.view(np.uint64), want_k.view(np.uint64)), where
    return ksize
