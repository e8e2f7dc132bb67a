"""The host-side level plan (multigridmc_amd/csrc/mgmc_level_plan.hpp), CPU only.

Which sweep kernel and which residual + restriction kernel a level runs, and where k_tail starts, is decided
once at mgmc_create by a header without HIP.  tests/cpp/level_plan_host.cpp, a stand-alone program, compiles it
with g++ under AddressSanitizer + UBSan, walks hierarchies by halving and checks the plan against the labels the
GPU tests assert for the same shapes (tests/test_gpu_headline.py, test_gpu_config3.py, test_gpu_fem.py,
test_gpu_parity.py ROW_LENGTH_LABELS), at the thresholds between two instances, and under every MGMC_DISABLE
token that changes the plan.  The tail's limits are checked there too: on hierarchies whose levels would fit
one workgroup's LDS five and six deep (2D 64^2 ... 1024^2 coarsened to 2^2 cells) the tail never holds more than
the TAIL_MAX_LEVELS levels of its argument block and every level from its start on is in place; the op count of a
run (tail_run_ops) is 183 / 120 / 92 for the W-cycle shapes of tests/test_gpu_cycle_shapes.py, and a run above
TAIL_MAX_OPS starts the tail a level later instead of being cut.  (A tail_start bounded by LDS size alone fails
the ten depth checks of the five 2D hierarchies, the three "tail_from_2" checks and the no-tail one.)  That the launchers run what the plan names needs a GPU: the label, parity and
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
    # 11 + 3 + 3 + 5 + 3 + 6 + 3 hierarchy checks, 6 boundaries, 8 tokens; the tail's limits: the constants, 8 deep
    # hierarchies x 3, the default-cycle overload, 8 op counts, 6 hierarchies by run length
    assert "FAIL" not in lines and lines.count("ok") == 11 + 3 + 3 + 5 + 3 + 6 + 3 + 6 + 8 + 1 + 8 * 3 + 1 + 8 + 6
