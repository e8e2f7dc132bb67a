"""Rao-Blackwellised field statistics (mgmc_field_stats_enable_cond, multigridmc_amd/csrc/mgmc_fieldcond.hpp): what
needs no GPU.

  * every new entry point rejects a NULL handle with MGMC_E_INVALID, the names are bound, the ABI version is 5;
  * plan_fieldcond (mgmc_level_plan.hpp) and the host-only d builder (mgmc_fieldcond_host.hpp) through the
    stand-alone tests/cpp/fieldcond_plan_host.cpp, built with g++ -fsanitize=address,undefined: the fused z-march
    for 64 x 22 x 10 alone; two passes with 3 chains, a low-rank part, the force flag, MGMC_DISABLE=zsweep, a
    variable-diagonal level, 24 x 20 x 12, 2D, FEM and the 2D squared operator; d of a 2D 12 x 10 posterior with two
    point measurements and the global average, bitwise against the numpy formula;
  * the identity diag Cov(c) + D^-1 = diag(Q^-1) for c = x + D^-1 (f - Q x) on that posterior, dense float64;
  * the estimator on the MULTICOLOUR CPU oracle (which the device reproduces bit for bit): 3D 16^3, FD
    kappa^2 = 25, 3 levels, seed 5418513, chain 7, 200 cycles discarded, 4000 kept, batches of 50.  Over all 3375
    vertices the Rao-Blackwell variance lies within 5 standard errors var(c) sqrt(2 tau / n) of the dense inverse's
    diagonal, the mean of c within 5 sqrt(var(c) tau / n) of 0, and the sample variance of c is below that of x
    (the algebra gives a ratio of at most 0.28).  5 is the project's bound; tau is the batch-means estimate per
    vertex, floored at 1.
"""
import ctypes
import os
import subprocess

import numpy as np

import multigridmc_amd as mg
from multigridmc_amd import _native
from multigridmc_amd.parameters import MeasurementParameters
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5418513

RB_SHAPE, RB_LEVELS, RB_CHAIN, RB_DISCARD, RB_KEPT, RB_BATCH = (16, 16, 16), 3, 7, 200, 4000, 50


def small_posterior():
    """2D 12 x 10, two point measurements and the global average (a dense column)"""
    lat = mg.Lattice(12, 10)
    mp = MeasurementParameters(radius=0.0, variance_scaling=1e-3, measure_global=True, variance_global=0.02)
    mp.measurement_locations = [[0.3, 0.4], [0.7, 0.55]]
    mp.variance = [1.5, 2.5]
    return mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(lat, 25.0), mp)


def conditional_precision(diag, lowrank):
    """d_i = a_ii, then d_i = d_i + (B_ik * B_ik) / Sigma_k for k ascending where B_ik is stored (float64)"""
    d = np.array(diag, dtype=np.float64, copy=True)
    if lowrank is None:
        return d
    for k in range(lowrank.m):
        s = slice(lowrank.colptr[k], lowrank.colptr[k + 1])
        r, v = lowrank.rows[s], lowrank.vals[s]
        d[r] = d[r] + (v * v) / lowrank.sigma[k]  # (rows of a column are distinct)
    return d


def test_new_entries_reject_a_null_handle():
    lib = mg.load_library()
    d = (ctypes.c_double * 4)()
    i, j = ctypes.c_int(), ctypes.c_int()
    calls = [
        lambda: lib.mgmc_field_stats_enable_cond(None, 1, 0, 0),
        lambda: lib.mgmc_field_stats_cond_info(None, ctypes.byref(i), ctypes.byref(j)),
        lambda: lib.mgmc_field_stats_get_cond_precision(None, d, 4),
    ]
    for call in calls:
        assert call() == _native.MGMC_E_INVALID
        assert "null handle" in _native.last_error()
    names = [s[0] for s in _native.SIGNATURES]
    for name in ["mgmc_field_stats_enable_cond", "mgmc_field_stats_cond_info", "mgmc_field_stats_get_cond_precision"]:
        assert name in names
    assert lib.mgmc_abi_version() == 5


def test_plan_and_precision_stand_alone(tmp_path):
    exe = os.path.join(str(tmp_path), "fieldcond_plan_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "multigridmc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "fieldcond_plan_host.cpp"), "-o", exe], check=True)
    op = small_posterior()
    lr = op.get_B()
    n = op.get_ndof()
    diag = op.base_operator.matrix().diagonal()
    assert lr.m == 3 and lr.colptr[3] - lr.colptr[2] == n  # (the last column is dense)
    data = os.path.join(str(tmp_path), "posterior.txt")
    with open(data, "w") as out:
        out.write(f"{n} {lr.m}\n")
        out.write(" ".join(float(v).hex() for v in diag) + "\n")
        out.write(" ".join(str(int(v)) for v in lr.colptr) + "\n")
        out.write(" ".join(str(int(v)) for v in lr.rows) + "\n")
        out.write(" ".join(float(v).hex() for v in lr.vals) + "\n")
        out.write(" ".join(float(v).hex() for v in lr.sigma) + "\n")
    r = subprocess.run([exe, data], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert not [ln for ln in lines if ln.startswith("FAIL")]
    for name in ["fused_64x22x10", "two_pass_three_chains", "two_pass_lowrank", "two_pass_forced",
                 "two_pass_disable_zsweep", "two_pass_vardiag", "two_pass_24x20x12", "two_pass_2d_48x40",
                 "two_pass_fem_16", "two_pass_2d_squared", "d_without_lowrank", "d_two_columns"]:
        assert "ok " + name in lines
    got = np.array([float.fromhex(ln.split()[2]) for ln in lines if ln.startswith("d ")])
    want = conditional_precision(diag, lr)
    assert got.shape == (n,)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(want > diag)  # (the dense column reaches every vertex)


def test_conditional_mean_identity_dense():
    op = small_posterior()
    A = op.base_operator.matrix().toarray()
    B = op.get_B().dense()
    Q = A + B @ np.diag(1.0 / op.get_B().sigma) @ B.T
    d = conditional_precision(np.diag(A), op.get_B())
    assert np.allclose(d, np.diag(Q), rtol=1e-14, atol=0.0)
    Qi = np.linalg.inv(Q)
    n = len(d)
    M = np.eye(n) - Q / d[:, None]  # c - E[c] = (I - D^-1 Q) (x - E[x])
    lhs = np.diag(M @ Qi @ M.T) + 1.0 / d
    assert np.max(np.abs(lhs - np.diag(Qi)) / np.diag(Qi)) < 1e-12
    # and E[c] = E[x]: (I - D^-1 Q) Q^-1 f + D^-1 f = Q^-1 f
    f = np.random.default_rng(3).standard_normal(n)
    assert np.allclose(M @ (Qi @ f) + f / d, Qi @ f, rtol=1e-12, atol=1e-14)
    # the one place that holds the formula
    mean, var = mg.rao_blackwell_estimates(4, np.ones(n), 8.0 * np.ones(n), d)
    assert np.array_equal(mean, np.ones(n)) and np.array_equal(var, 1.0 / d + 2.0)
    try:
        mg.rao_blackwell_estimates(0, np.ones(n), np.ones(n), d)
    except ValueError:
        pass
    else:
        raise AssertionError("n = 0 must raise")


def welford_batch_moments(v, batch):
    """(n, mean, M2, nb, bM2) of the rows of v (float64 sums; statistics, not bits)"""
    n = v.shape[0]
    mean = v.mean(axis=0)
    m2 = ((v - mean) ** 2).sum(axis=0)
    nb = n // batch
    bm = v[:nb * batch].reshape(nb, batch, -1).mean(axis=1)
    bm2 = ((bm - bm.mean(axis=0)) ** 2).sum(axis=0)
    return n, mean, m2, nb, bm2


def rao_blackwell_checks(x, c, d, exact_var, batch, label):
    """the three assertions of the estimator; x, c: one row per recorded state"""
    n, mean_c, m2_c, nb, bm2_c = welford_batch_moments(c, batch)
    _, mean_x, m2_x, _, bm2_x = welford_batch_moments(x, batch)
    _, tau_c = mg.batch_means_estimates(batch, nb, bm2_c, n, m2_c)
    _, tau_x = mg.batch_means_estimates(batch, nb, bm2_x, n, m2_x)
    tau = np.maximum(tau_c, 1.0)
    mean_rb, var_rb = mg.rao_blackwell_estimates(n, mean_c, m2_c, d)
    var_c, var_x = m2_c / n, m2_x / n
    z_var = np.abs(var_rb - exact_var) / (var_c * np.sqrt(2.0 * tau / n))
    z_mean = np.abs(mean_rb) / np.sqrt(var_c * tau / n)
    ratio = var_c / var_x
    rms_rb = np.sqrt(np.mean(((var_rb - exact_var) / exact_var) ** 2))
    rms_x = np.sqrt(np.mean(((var_x - exact_var) / exact_var) ** 2))
    print(f"{label}: max z variance {z_var.max():.2f}, max z mean {z_mean.max():.2f}, "
          f"largest var(c) / var(x) {ratio.max():.3f}, median tau c {np.median(tau_c):.2f} x {np.median(tau_x):.2f}, "
          f"RMS relative error of the variance RB {rms_rb:.4f} / plain {rms_x:.4f} = {rms_rb / rms_x:.3f}")
    assert z_var.max() < 5.0
    assert z_mean.max() < 5.0
    assert np.all(var_c < var_x)


def test_rao_blackwell_on_the_oracle():
    op = mg.ShiftedLaplaceFDOperator(mg.Lattice(*RB_SHAPE), 25.0)
    p = mg.MultigridParameters(nlevel=RB_LEVELS)
    mc = O.Oracle.fd(RB_SHAPE, p, 25.0, mode=O.MULTICOLOUR, seed=SEED, chain=RB_CHAIN)
    n = op.get_ndof()
    assert n == 3375
    A = mc.csr_matrix(0)  # the oracle's own level 0
    d = A.diagonal()
    mc.set_rhs(np.zeros(n))
    mc.set_state(np.zeros(n))
    mc.sample(RB_DISCARD)
    x = np.empty((RB_KEPT, n))
    for t in range(RB_KEPT):
        mc.sample(1)
        x[t] = mc.get_state()
    c = x + (0.0 - (A @ x.T).T) / d
    exact = np.diag(np.linalg.inv(op.matrix().toarray()))
    rao_blackwell_checks(x, c, d, exact, RB_BATCH, "oracle 16^3")
