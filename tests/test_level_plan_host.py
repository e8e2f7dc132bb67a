"""The host-side level plan (multigridmc_amd/csrc/mgmc_level_plan.hpp), CPU only.

Which sweep kernel and which residual + restriction kernel a level runs, and where k_tail starts, is decided
once at mgmc_create by a header without HIP.  tests/cpp/level_plan_host.cpp, a stand-alone program, compiles it
with g++ under AddressSanitizer + UBSan, walks hierarchies by halving and checks the plan against the labels the
GPU tests assert for the same shapes (tests/test_gpu_headline.py, test_gpu_config3.py, test_gpu_fem.py,
test_gpu_parity.py ROW_LENGTH_LABELS), at the thresholds between two instances, and under every MGMC_DISABLE
token that changes the plan.  That the launchers run what the plan names needs a GPU: the label, parity and
variant tests."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_plan_matches_recorded_labels(tmp_path):
    exe = os.path.join(str(tmp_path), "level_plan_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "multigridmc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "level_plan_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    lines = r.stdout.split()
    assert r.returncode == 0, r.stdout + r.stderr
    # 11 + 3 + 3 + 5 + 3 + 6 + 3 hierarchy checks, 6 boundaries, 8 tokens
    assert "FAIL" not in lines and lines.count("ok") == 11 + 3 + 3 + 5 + 3 + 6 + 3 + 6 + 8
