"""Host logic of the zero-right-hand-side path (multigridmc_amd/csrc/mgmc_rhs_zero.hpp), CPU only.

What counts as a zero right-hand side (the OR of the bit patterns: -0.0, denormals, NaN and Inf are not zero)
and which ops of the cycle may take it as a constant (level 0, z-marching kernels, no low-rank part) is a
header without HIP.  tests/cpp/rhs_zero_host.cpp, a stand-alone program, compiles it with g++ under
AddressSanitizer + UBSan and checks both.  The device side -- the k_or_bits reduction, the read-back in
mgmc_set_rhs, the graph rebuild and the kernels themselves -- needs a GPU: tests/test_gpu_rhs_zero.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_detection_and_selection_logic(tmp_path):
    exe = os.path.join(str(tmp_path), "rhs_zero_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "multigridmc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "rhs_zero_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    lines = r.stdout.split()
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAIL" not in lines and lines.count("ok") == 2 + 6 * 3 + 1 + 10
