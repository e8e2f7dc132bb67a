"""The variable-diagonal fine level on the CPU (no GPU touched).

* mgmc_vardiag_of_csr (host only) recognises a matrix that is a constant, symmetric axis-neighbour stencil
  truncated at the boundary plus an arbitrary positive diagonal -- ShiftedLaplaceFDOperator with any
  correlation-length model -- and returns the six couplings bit for bit with a zero centre; everything else is
  MGMC_E_UNSUPPORTED and keeps the field kernels.  mgmc_create_csr runs the same check on its fine matrix.
* tests/cpp/vardiag_plan_host.cpp, a stand-alone program compiled with g++ under AddressSanitizer + UBSan: the
  level plan (mgmc_level_plan.hpp) gives such a level the z-marching sweep and residual + restriction, and the
  field kernels under MGMC_DISABLE=zsweep / zrestrict and on every shape the z-sweep does not take.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import multigridmc_amd as mg
from multigridmc_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIODIC = mg.PeriodicCorrelationLengthModel(0.2, 0.4)


def axis_matrix(shape, couplings, diag):
    """CSR of the 3D lattice's interior vertices (x fastest): `couplings` = (cx, cy, cz) to the axis neighbours in
    either direction, `diag` per vertex."""
    mats = []
    for d, n in enumerate(shape):
        T = sp.diags([np.ones(n - 2), np.ones(n - 2)], [-1, 1], shape=(n - 1, n - 1))
        eyes = [sp.identity(m - 1) for m in shape]
        eyes[d] = T
        mats.append(couplings[d] * sp.kron(eyes[2], sp.kron(eyes[1], eyes[0])))
    A = sp.csr_matrix(mats[0] + mats[1] + mats[2] + sp.diags(np.asarray(diag, dtype=np.float64)))
    A.sort_indices()
    return A


def dominant_matrix(shape, couplings=(-1.25, -0.75, -2.5), seed=11):
    """The hand-made anisotropic matrix of the tests: three distinct couplings and a random diagonal that keeps
    every row strictly diagonally dominant."""
    n = int(np.prod([m - 1 for m in shape]))
    rng = np.random.default_rng(seed)
    diag = 2.0 * sum(abs(c) for c in couplings) * (1.05 + rng.random(n))
    return axis_matrix(shape, couplings, diag)


def vardiag_of(lattice, rowptr, col, val):
    op = mg.SparseMatrixOperator(lattice, mg.sampler_csr_matrix(rowptr, col, val, lattice.Nvertex))
    cfg = mg.make_config(op, mg.MultigridParameters(nlevel=2))
    rowptr, col, val = op.get_csr()
    st = np.full(27, np.nan)
    rc = mg.load_library().mgmc_vardiag_of_csr(ctypes.byref(cfg), len(rowptr) - 1,
                                               rowptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                               col.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               val.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                               st.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return rc, st, op, cfg


def expect_stencil(st, cx, cy, cz):
    want = np.zeros(27)
    want[[12, 14]], want[[10, 16]], want[[4, 22]] = cx, cy, cz
    assert np.array_equal(st.view(np.uint64), want.view(np.uint64)), st


@pytest.mark.parametrize("shape", [(64, 22, 10), (16, 12, 8)])
def test_periodic_fd_operator_is_recognised(shape):
    lat = mg.Lattice(*shape)
    fd = mg.ShiftedLaplaceFDOperator(lat, PERIODIC)
    rowptr, col, val = fd.get_csr()
    rc, st, op, cfg = vardiag_of(lat, rowptr, col, val)
    assert rc == _native.MGMC_OK, mg.load_library().mgmc_last_error(None)
    # the couplings as the matrix stores them: the centre row's -x, -y, -z entries
    A = fd.matrix().tocsr()
    nxi, nyi = shape[0] - 1, shape[1] - 1
    r = ((shape[2] // 2 - 1) * nyi + (shape[1] // 2 - 1)) * nxi + (shape[0] // 2 - 1)
    expect_stencil(st, A[r, r - 1], A[r, r - nxi], A[r, r - nxi * nyi])
    assert len(np.unique(A.diagonal())) > 1, "the periodic model's diagonal is not constant"
    assert np.array_equal(op.vardiag_stencil(cfg), st)
    assert op.constant_stencil(cfg) is None


def test_hand_made_anisotropic_matrix_is_recognised():
    shape = (16, 12, 8)
    A = dominant_matrix(shape)
    rc, st, op, cfg = vardiag_of(mg.Lattice(*shape), A.indptr, A.indices, A.data)
    assert rc == _native.MGMC_OK, mg.load_library().mgmc_last_error(None)
    expect_stencil(st, -1.25, -0.75, -2.5)


def test_constant_diagonal_passes_too():
    lat = mg.Lattice(16, 12, 8)
    rowptr, col, val = mg.ShiftedLaplaceFDOperator(lat, 25.0).get_csr()
    rc, st, _, _ = vardiag_of(lat, rowptr, col, val)
    assert rc == _native.MGMC_OK and st[13] == 0.0 and st[12] == st[14] != 0.0


def _fd(shape=(16, 12, 8)):
    lat = mg.Lattice(*shape)
    rowptr, col, val = mg.ShiftedLaplaceFDOperator(lat, PERIODIC).get_csr()
    return lat, rowptr.copy(), col.copy(), val.copy()


def _entry(rowptr, col, r, c):
    (q,) = [q for q in range(rowptr[r], rowptr[r + 1]) if col[q] == c]
    return q


def _refused(lat, rowptr, col, val):
    rc, st, _, _ = vardiag_of(lat, rowptr, col, val)
    return rc == _native.MGMC_E_UNSUPPORTED


def test_refuses_the_fem_operator():
    lat = mg.Lattice(16, 12, 8)
    assert _refused(lat, *mg.ShiftedLaplaceFEMOperator(lat, PERIODIC).get_csr())


def test_refuses_a_2d_lattice():
    lat = mg.Lattice(32, 32)
    assert _refused(lat, *mg.ShiftedLaplaceFDOperator(lat, PERIODIC).get_csr())


def test_refuses_one_off_diagonal_changed_in_the_last_bit():
    lat, rowptr, col, val = _fd()
    q = _entry(rowptr, col, 700, 701)
    val[q] = np.nextafter(val[q], 0.0)
    assert _refused(lat, rowptr, col, val)
    assert b"row 700" in mg.load_library().mgmc_last_error(None)


def test_refuses_unequal_x_couplings():
    lat, rowptr, col, val = _fd()
    nrow = len(rowptr) - 1
    for r in range(nrow):  # every +x entry scaled: each offset still one number, -x != +x
        for q in range(rowptr[r], rowptr[r + 1]):
            if col[q] == r + 1:
                val[q] *= 1.5
    assert _refused(lat, rowptr, col, val)
    assert b"symmetric" in mg.load_library().mgmc_last_error(None)


def test_refuses_a_missing_interior_coupling():
    lat, rowptr, col, val = _fd()
    A = mg.sampler_csr_matrix(rowptr, col, val, lat.Nvertex).tolil()
    nxi = lat.shape[0] - 1
    A[700, 700 + nxi] = 0.0
    A = A.tocsr()
    A.eliminate_zeros()
    assert A.nnz == len(val) - 1
    assert _refused(lat, A.indptr, A.indices, A.data)


def test_refuses_an_edge_neighbour_entry():
    lat, rowptr, col, val = _fd()
    A = mg.sampler_csr_matrix(rowptr, col, val, lat.Nvertex).tolil()
    nxi = lat.shape[0] - 1
    A[700, 700 + nxi + 1] = -0.125
    A = A.tocsr()
    assert _refused(lat, A.indptr, A.indices, A.data)


def test_refuses_a_non_positive_diagonal():
    lat, rowptr, col, val = _fd()
    val[_entry(rowptr, col, 5, 5)] = -1.0
    assert _refused(lat, rowptr, col, val)


def test_level_plan_of_a_vardiag_level(tmp_path):
    exe = os.path.join(str(tmp_path), "vardiag_plan_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "multigridmc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "vardiag_plan_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    lines = r.stdout.split()
    assert r.returncode == 0, r.stdout + r.stderr
    # default + tokens, 5 checks on each of 3 shapes, wide tiles, 5 ineligible shapes, the constant level
    assert "FAIL" not in lines and lines.count("ok") == 2 + 5 * 3 + 1 + 5 + 1
