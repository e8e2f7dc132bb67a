"""The re-tuned variants of tests/tuning_variants.py on the CPU, before any GPU time is spent on them.

  * every `constexpr int` of multigridmc_amd/csrc/mgmc_tuning.hpp is non-default in at least one variant (a new
    constant cannot be forgotten), and every edit names a constant of the header;
  * the host-side level plan (mgmc_level_plan.hpp), compiled against each variant's header by
    tests/cpp/level_plan_host.cpp's "plan" mode under AddressSanitizer + UBSan, selects the kernel instance each
    case of tests/test_gpu_tuning.py is there for -- and the default header does not;
  * mgmc_check_layout (host code) through each variant library over the case shapes and their hierarchies.
"""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import pytest

from multigridmc_amd import _native
from tests.test_gpu_tuning import CASES
from tests.tuning_variants import VARIANTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multigridmc_amd", "csrc")

_spec = importlib.util.spec_from_file_location("build_tuning_variants",
                                               os.path.join(ROOT, "scripts", "build_tuning_variants.py"))
recipe = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recipe)


def test_every_tuning_constant_is_varied():
    defaults = recipe.header_constants()
    assert len(defaults) >= 27 and defaults["ZR7_WIDE_MIN_TILES"] == 16384
    # nothing escapes the parse: every `constexpr` outside a comment is one of the parsed constants
    code = [line.split("//")[0] for line in recipe.header_text().splitlines()]
    assert sum(line.count("constexpr") for line in code) == len(defaults)
    for name, edits in VARIANTS.items():
        unknown = set(edits) - set(defaults)
        assert not unknown, f"variant {name} edits constants the header does not have: {sorted(unknown)}"
        same = [k for k, v in edits.items() if v == defaults[k]]
        assert not same, f"variant {name} leaves {same} at the default"
        assert recipe.header_constants(recipe.edited_header(edits)) == {**defaults, **edits}
    never = [k for k in defaults if not any(k in edits for edits in VARIANTS.values())]
    assert not never, f"no variant changes {never}: add a non-default value to tests/tuning_variants.py"


@pytest.fixture(scope="module")
def plan_programs(tmp_path_factory):
    """level_plan_host compiled once per header: the default and each variant's."""
    exes = {}
    for name in ["default"] + list(VARIANTS):
        inc = tmp_path_factory.mktemp("plan_" + name)
        # (mgmc_level_plan.hpp includes the tuning header by its quoted name: both from one directory)
        shutil.copy(os.path.join(CSRC, "mgmc_level_plan.hpp"), inc)
        with open(os.path.join(str(inc), "mgmc_tuning.hpp"), "w") as fh:
            fh.write(recipe.edited_header(VARIANTS.get(name, {})))
        exe = os.path.join(str(inc), "level_plan_host")
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined", "-I", str(inc),
                        os.path.join(ROOT, "tests", "cpp", "level_plan_host.cpp"), "-o", exe], check=True)
        exes[name] = exe
    return exes


def plan(exe, shape, nlevel, disable="", vardiag=False):
    nx, ny, nz = (list(shape) + [0])[:3]
    r = subprocess.run([exe, "plan", str(nx), str(ny), str(nz), str(nlevel), disable] + (["vardiag"] if vardiag else []),
                       capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


# (header, shape, nlevel, MGMC_DISABLE, level, what the level's line must contain).  The walk of level_plan_host.cpp
# takes every 3D Galerkin level of an FD hierarchy as a fold level; the rows with "sym" are cubic or bitwise
# reflection-symmetric hierarchies (tests/test_gpu_parity.py test_fold_levels_reference_order_bitwise), the others
# assert nothing that depends on it.
PLANS = [
    # the 512-thread 64 x 8 7-point restriction at 19 coarse rows (8 + 8 + 3), and with the clamped last columns
    ("default", (256, 40, 48), 2, "", 0, "sweep ZSWEEP residual ZMARCH np 7 cx 64 cy 4 nt 256"),
    ("lo", (256, 40, 48), 2, "", 0, "sweep ZSWEEP residual ZMARCH np 7 cx 64 cy 8 nt 512"),
    ("hi", (256, 40, 48), 2, "", 0, "residual ZMARCH np 7 cx 64 cy 4 nt 256"),
    ("lo", (132, 36, 20), 2, "", 0, "sweep COLOUR residual ZMARCH np 7 cx 64 cy 8 nt 512"),
    # 64-pair rows: quads by default, pair passes under lo
    ("default", (256, 128, 64), 3, "", 1, "sweep QUADS lanes residual ZMARCH np 27 cx 64 cy 4 nt 256 sym"),
    ("lo", (256, 128, 64), 3, "", 1, "sweep PAIRS"),
    ("hi", (256, 128, 64), 3, "", 1, "sweep QUADS lanes residual ZMARCH np 27 cx 32 cy 4 nt 256 sym"),
    # fold levels: 64 x 8 tiles and window quads under lo, the 16 x 4 tiles under hi
    ("default", (128, 128, 128), 3, "", 1, "sweep QUADS lanes residual ZMARCH np 27 cx 64 cy 4 nt 256 sym"),
    ("lo", (128, 128, 128), 3, "", 1, "sweep QUADS window residual ZMARCH np 27 cx 64 cy 8 nt 256 sym"),
    ("hi", (128, 128, 128), 3, "", 1, "sweep QUADS lanes residual ZMARCH np 27 cx 16 cy 4 nt 64 small sym"),
    # rows of 128 pairs: j-marching; without it pair passes, quad passes (window) under hi
    ("lo", (512, 16, 24), 3, "", 1, "sweep JSWEEP"),
    ("default", (512, 16, 24), 3, "jsweep", 1, "sweep PAIRS"),
    ("hi", (512, 16, 24), 3, "jsweep", 1, "sweep QUADS window"),
    # JS_ROUNDS acts only where a half's planes x steps exceed one round of 768 workgroups: 28 x 30 on 256 x 58 x 58
    ("default", (512, 116, 116), 3, "", 1, "sweep JSWEEP js 15x2"),
    ("lo", (512, 116, 116), 3, "", 1, "sweep JSWEEP js 30x1"),
    ("hi", (512, 116, 116), 3, "", 1, "sweep JSWEEP js 15x2"),
    ("default", (512, 44, 60), 3, "", 1, "sweep JSWEEP js 12x1"),  # (not on the smaller j-marching cases)
    ("lo", (512, 44, 60), 3, "", 1, "sweep JSWEEP js 12x1"),
    # 80-pair rows
    ("default", (320, 24, 16), 3, "", 1, "sweep PAIRS"),
    ("hi", (320, 24, 16), 3, "", 1, "sweep QUADS window"),
    # ZR_SMALL_NX 16 / 64 moves levels between the 16 x 4 and the 64-wide restriction
    ("default", (64, 64, 64), 4, "", 0, "residual ZMARCH np 7 cx 64 cy 4 nt 256 tail 2"),
    ("default", (64, 64, 64), 4, "", 1, "sweep QUADS lanes residual ZMARCH np 27 cx 16 cy 4 nt 64 small sym tail 2"),
    ("lo", (64, 64, 64), 4, "", 0, "residual ZMARCH np 7 cx 64 cy 8 nt 512 tail 2"),
    ("lo", (64, 64, 64), 4, "", 1, "sweep QUADS window residual ZMARCH np 27 cx 64 cy 8 nt 256 sym tail 2"),
    ("hi", (64, 64, 64), 4, "", 0, "residual ZMARCH np 7 cx 16 cy 4 nt 64 small tail 2"),
    ("lo", (96, 96, 96), 5, "", 1, "sweep QUADS window"),
    ("hi", (96, 96, 96), 5, "", 0, "sweep COLOUR residual ZMARCH np 7 cx 16 cy 4 nt 64 small"),
    ("lo", (136, 136, 136), 4, "", 1, "sweep PAIRS"),
    ("lo", (136, 136, 136), 4, "", 2, "sweep QUADS window"),
    ("hi", (136, 136, 136), 4, "", 0, "residual ZMARCH np 7 cx 64 cy 4 nt 256"),
    ("hi", (136, 136, 136), 4, "", 1, "sweep QUADS window residual ZMARCH np 27 cx 16 cy 4 nt 64 small"),
    # the tail's neighbours (512 x 32 x 32, 5 levels): level 2 of 64-pair rows
    ("default", (512, 32, 32), 5, "", 2, "sweep QUADS lanes"),
    ("lo", (512, 32, 32), 5, "", 2, "sweep PAIRS"),
    ("hi", (512, 32, 32), 5, "", 1, "residual ZMARCH np 27 cx 32 cy 4 nt 256 sym tail 3"),
    # 2D: the plan does not depend on the thread counts
    ("lo", (512, 512), 4, "", 1, "sweep QUADS residual GATHER"),
    ("hi", (200, 120), 4, "", 1, "sweep QUADS residual GATHER"),
]


@pytest.mark.parametrize("header,shape,nlevel,disable,level,want", PLANS,
                         ids=[f"{p[0]}-{'x'.join(map(str, p[1]))}-{p[3] or 'all'}-l{p[4]}" for p in PLANS])
def test_variant_selects_the_instance(plan_programs, header, shape, nlevel, disable, level, want):
    line = plan(plan_programs[header], shape, nlevel, disable)[level]
    assert line.startswith(f"level {level} ") and want in line, line


# The matrix handle of a variable-diagonal fine level (the vd_* cases of tests/test_gpu_tuning.py, the lattices of
# tests/test_gpu_vardiag.py): the VD sweep takes the variant's ZS_TYP rows, the 7-point restriction the 512-thread
# 64 x 8 instance under lo only -- by default only from 16,384 wide tiles up (512^3) -- and level 1 the field kernels.
VD_LEVEL0 = {"default": "sweep ZSWEEP rows 16 residual ZMARCH np 7 cx 64 cy 4 nt 256 vd tail -1",
             "lo": "sweep ZSWEEP rows 12 residual ZMARCH np 7 cx 64 cy 8 nt 512 vd tail -1",
             "hi": "sweep ZSWEEP rows 20 residual ZMARCH np 7 cx 64 cy 4 nt 256 vd tail -1"}
VD_SHAPES = [((64, 22, 10), 2), ((128, 34, 18), 2), ((192, 48, 40), 3)]


@pytest.mark.parametrize("header", list(VD_LEVEL0))
@pytest.mark.parametrize("shape,nlevel", VD_SHAPES, ids=["x".join(map(str, s)) for s, _ in VD_SHAPES])
def test_variant_selects_the_vardiag_instances(plan_programs, header, shape, nlevel):
    lines = plan(plan_programs[header], shape, nlevel, vardiag=True)
    assert lines[0] == "level 0 " + VD_LEVEL0[header], lines
    if nlevel > 2:
        assert lines[1] == "level 1 sweep FIELD residual FIELD tail -1", lines
    # the default header reaches the wide instance at 512^3 only (256^3: 4,064 wide tiles)
    if header == "default":
        assert "cy 8 nt 512 vd" in plan(plan_programs[header], (512, 512, 512), 2, vardiag=True)[0]
        assert "cy 4 nt 256 vd" in plan(plan_programs[header], (256, 256, 256), 2, vardiag=True)[0]
    # MGMC_DISABLE=zsweep leaves the level to the field kernels under every header
    assert plan(plan_programs[header], shape, nlevel, "zsweep", vardiag=True)[0] == \
        "level 0 sweep FIELD residual FIELD tail -1"


def _hierarchy(shape, nlevel):
    out = [tuple(shape)]
    while len(out) < nlevel:
        out.append(tuple(v // 2 for v in out[-1]))
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variant_library_layout_checks(variant):
    """mgmc_check_layout of the variant library (its own tile constants: the j-marching replay with its JS_D and
    JS_ROUNDS, the restriction with every tile width the variant can select) on every level of every case."""
    (path,) = recipe.build([variant])  # (compiles nothing while the library's inputs are unchanged)
    lib = _native.load_library(path)
    widths = sorted({16, 64, VARIANTS[variant].get("ZR27_CX", 64)})
    seen = set()
    for case in CASES:
        for lv in _hierarchy(case["shape"], case["params"].get("nlevel", 3)):
            if lv in seen:
                continue
            seen.add(lv)
            dim = len(lv)
            n = (ctypes.c_int * 3)(*(list(lv) + [0] * (3 - dim)))
            families = (1 | 2 | 4 | 8 | 16) if dim == 3 else (1 | 2 | 32 | 128)
            if dim == 3 and lv[0] in (256, 512) and lv[1] >= 2 and lv[2] >= 2:
                families |= 64
            for cx in widths if dim == 3 else [0]:
                rc = lib.mgmc_check_layout(dim, n, 1, families, cx, 0)
                assert rc == _native.MGMC_OK, (variant, lv, cx, lib.mgmc_last_error(None))
    assert len(seen) > 60
