"""Whole-field energy x^T Q x, f^T x (mgmc_energy*, multigridmc_amd/csrc/mgmc_energy.hpp): what needs no GPU.

  * every new entry point rejects a NULL handle with MGMC_E_INVALID;
  * plan_energy (mgmc_level_plan.hpp) through the stand-alone tests/cpp/energy_plan_host.cpp, built with
    g++ -fsanitize=address,undefined: the z-march for 64 x 22 x 10 and for a variable-diagonal level, a general
    kernel for 24 x 20 x 12, 2D, FEM and field levels;
  * the longdouble reference of tests/energy_ref.py against dense float64 algebra on a small posterior;
  * the chi-square identity on the MULTICOLOUR CPU oracle (which the device reproduces bit for bit): at
    stationarity E = x^T Q x is chi-square with N degrees of freedom, so the mean of n correlated records lies
    within 5 sqrt(2 N tau / n) of N.  64 x 36 x 20 (N = 41,895), FD prior kappa^2 = 25, 3 levels, seed 5418513,
    chain 3, 100 cycles discarded, 600 kept; tau = iact_windowed of that series, floored at 1.  The test prints tau:
    it is the tau tests/test_gpu_energy.py::test_chi_square_on_the_device uses (1.157).
"""
import ctypes
import os
import subprocess

import numpy as np

import multigridmc_amd as mg
from multigridmc_amd import _native
from multigridmc_amd.parameters import MeasurementParameters
from tests import energy_ref as ER
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5418513

CHI_SHAPE, CHI_LEVELS, CHI_CHAIN, CHI_DISCARD = (64, 36, 20), 3, 3, 100


def chi_operator():
    return mg.ShiftedLaplaceFDOperator(mg.Lattice(*CHI_SHAPE), 25.0), mg.MultigridParameters(nlevel=CHI_LEVELS)


def test_new_entries_reject_a_null_handle():
    lib = mg.load_library()
    d = (ctypes.c_double * 4)()
    i, j = ctypes.c_int(), ctypes.c_int()
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    calls = [
        lambda: lib.mgmc_energy(None, 0, d, d),
        lambda: lib.mgmc_energy_record_enable(None, 1, 16),
        lambda: lib.mgmc_energy_record_disable(None),
        lambda: lib.mgmc_energy_record_reset(None),
        lambda: lib.mgmc_energy_record_info(None, ctypes.byref(i), ctypes.byref(j), ctypes.byref(a), ctypes.byref(b)),
        lambda: lib.mgmc_energy_get_series(None, 0, d, d, 1),
        lambda: lib.mgmc_energy_moments(None, 0, d),
    ]
    for call in calls:
        assert call() == _native.MGMC_E_INVALID
    assert "null handle" in _native.last_error()
    names = [s[0] for s in _native.SIGNATURES]
    assert [n for n in names if n.startswith("mgmc_energy")] == [
        "mgmc_energy", "mgmc_energy_record_enable", "mgmc_energy_record_disable", "mgmc_energy_record_reset",
        "mgmc_energy_record_info", "mgmc_energy_get_series", "mgmc_energy_moments"]
    assert lib.mgmc_abi_version() == 5


def test_plan_energy_stand_alone(tmp_path):
    exe = os.path.join(str(tmp_path), "energy_plan_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "multigridmc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "energy_plan_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert not [ln for ln in lines if ln.startswith("FAIL")]
    for name in ["zmarch_64x22x10", "zmarch_vardiag_128x34x18", "general_24x20x12", "general_2d_48x40",
                 "general_fem_64", "field_periodic_32x16x16", "field_2d_squared", "forced_general_64x22x10"]:
        assert "ok " + name in lines
    assert len(lines) == 16


def test_reference_helper_against_dense_algebra():
    """2D 12 x 10 posterior with two point measurements and the global average: the helper's values against
    x^T (A + B Sigma^-1 B^T) x from dense float64 matrices, and S, T, n by their definitions."""
    lat = mg.Lattice(12, 10)
    mp = MeasurementParameters(radius=0.0, variance_scaling=1e-3, measure_global=True, variance_global=0.02)
    mp.measurement_locations = [[0.3, 0.4], [0.7, 0.55]]
    mp.variance = [1.5, 2.5]
    op = mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(lat, 25.0), mp)
    rng = np.random.default_rng(5)
    x, f = rng.standard_normal(op.get_ndof()), rng.standard_normal(op.get_ndof())
    xqx, fx, S, T, n = ER.energy_reference(op, f, x)
    A = op.base_operator.matrix().toarray()
    B = op.get_B().dense()
    Q = A + B @ np.diag(1.0 / op.get_B().sigma) @ B.T
    assert abs(xqx - x @ Q @ x) <= 1e-12 * S
    assert abs(fx - f @ x) <= 1e-13 * T
    w = np.abs(B).T @ np.abs(x)
    assert abs(S - (np.abs(x) @ np.abs(A) @ np.abs(x) + np.sum(w * w / op.get_B().sigma))) <= 1e-12 * S
    assert abs(T - np.abs(f) @ np.abs(x)) <= 1e-13 * T
    assert n == np.count_nonzero(A) + 2 * np.count_nonzero(B) + op.get_ndof() + 4 * 3
    assert S >= abs(xqx) and T >= abs(fx)
    # f None is the zero right-hand side
    assert ER.energy_reference(op, None, x)[1::2] == (0.0, 0.0)
    # the bound is sharp enough to see one dropped coupling at one vertex
    ref = ER.reference(op, f, x)
    assert ER.within_bound(xqx, fx, ref)[0]
    assert not ER.within_bound(xqx - 2 * A[5, 6] * x[5] * x[6], fx, ref)[0]
    w = ER.welford([1.0, 2.0, 4.0])
    assert w[0] == 3.0 and abs(w[1] - 7.0 / 3.0) < 1e-15 and abs(w[2] - 3.0 * np.var([1.0, 2.0, 4.0])) < 1e-14


def oracle_energy_series(ncycles):
    """x^T A x of the MULTICOLOUR oracle chain after each of `ncycles` cycles from x = 0, f = 0 (float64 products;
    their rounding, 1e-11 relative, is far below the statistical bound)"""
    op, p = chi_operator()
    A = op.matrix()
    mc = O.Oracle.fd(CHI_SHAPE, p, 25.0, mode=O.MULTICOLOUR, seed=SEED, chain=CHI_CHAIN)
    n = op.get_ndof()
    mc.set_rhs(np.zeros(n))
    mc.set_state(np.zeros(n))
    out = np.empty(ncycles)
    for t in range(ncycles):
        mc.sample(1)
        x = mc.get_state()
        out[t] = x @ (A @ x)
    return out


def test_chi_square_identity_on_the_oracle():
    kept = 600
    e = oracle_energy_series(CHI_DISCARD + kept)[CHI_DISCARD:]
    N = int(np.prod([m - 1 for m in CHI_SHAPE]))
    assert N == 41895
    tau = max(1.0, ER.iact_windowed(e))
    z = (e.mean() - N) / np.sqrt(2.0 * N * tau / kept)
    print(f"oracle chi-square: mean {e.mean():.1f}, N {N}, tau {tau:.3f}, z {z:+.2f}, var / 2N {e.var() / (2 * N):.3f}")
    assert abs(e.mean() - N) <= 5.0 * np.sqrt(2.0 * N * tau / kept)
