"""User stencils on the CPU: the stencil hierarchy and the oracle that the GPU tests of
tests/test_gpu_user_stencil.py rest on (fixtures: tests/user_stencils.py).

* tests/cpp/user_stencil_host.cpp, a stand-alone program (g++, AddressSanitizer + UBSan, linked with
  mgmc_hierarchy.cpp), prints build_hierarchy(cfg, fine_st)'s level stencils as bit patterns.  For every fixture
  they equal the interior rows of the oracle's own SpGEMM R A R^T (Oracle.stencil) bit for bit, and the bitwise
  reflection-symmetry flag (fold / SYM on the device) is set on every 27-point level of S7 / S27 and on none of
  C27 / C7 / P27.
* The same stencils against R A R^T in exact rational arithmetic: S7 / S27 (dyadic) exactly, every other fixture
  within gamma_m sum |terms|, gamma_m = m u / (1 - m u), u = 2^-53, m the number of terms of the two-step sum
  (3^d + 5^d): the worst case of any summation order, not a tuned figure.
* Oracle.stencil against Oracle.csr on the assembled matrix (bitwise for C27; for S27 everything but the fold
  levels' residuals), mgmc_stencil_of_csr on every fixture, the oracle's operator product and residual +
  restriction against np.longdouble on the GPU tests' C27 / C5 cases, and that exchanging any two coefficients of
  C27 / S27 changes the oracle's cycle (so each bitwise assertion of the GPU tests sees every coefficient)."""
import itertools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import multigridmc_amd as mg
from tests import oracle_lib as O
from tests import user_stencils as US

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {3: (48, 32, 64), 2: (48, 32)}  # 4 levels: the coarsest, 6 x 4 x 8 cells, still has the interior row (2,2,2)
NLEVEL = 4


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("user_stencil") / "user_stencil_host")
    csrc = os.path.join(ROOT, "multigridmc_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                    "-I", csrc, os.path.join(ROOT, "tests", "cpp", "user_stencil_host.cpp"),
                    os.path.join(csrc, "mgmc_hierarchy.cpp"), "-o", exe], check=True)
    return exe


def host_levels(exe, shape, nlevel, st):
    """[(npoints, ncolours, refl, stencil as 27 uint64)] per level from the host program."""
    n = list(shape) + [0] * (3 - len(shape))
    args = [exe, str(len(shape)), *map(str, n), str(nlevel), *(f"{int(b):016x}" for b in st.view(np.uint64))]
    r = subprocess.run(args, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for l, line in enumerate(r.stdout.splitlines()):
        w = line.split()
        assert w[0] == "level" and int(w[1]) == l and w[12] == "st" and len(w) == 13 + 27
        out.append((int(w[7]), int(w[9]), int(w[11]), np.array([int(v, 16) for v in w[13:]], dtype=np.uint64)))
    assert len(out) == nlevel
    return out


def params(**kw):
    return mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **kw})


def oracle_interior_stencil(orc, level, shape):
    """The row of vertex (2,2[,2]) of an oracle level as a 27-entry stencil (absent entries +0.0)."""
    dim = len(shape)
    ni = [n - 1 for n in shape]
    assert min(shape) >= 4
    # interior vertices are numbered from Euclidean (1,1[,1]), x fastest: (2,2[,2]) is 0-based (1,1[,1])
    row = (ni[1] + 1) * ni[0] + 1 if dim == 3 else ni[0] + 1
    col, val = orc.csr_row(level, row)
    st = np.zeros(27)
    for c, v in zip(col, val):
        c = int(c)
        i = c % ni[0]
        j = (c // ni[0]) % ni[1] if dim == 3 else c // ni[0]
        k = c // (ni[0] * ni[1]) if dim == 3 else 0
        st[(k * 9 if dim == 3 else 0) + j * 3 + i] = v  # offsets (i - 1, j - 1, k - 1) in {-1, 0, 1}
    return st


@pytest.mark.parametrize("name", list(US.STENCILS))
def test_hierarchy_equals_oracle_interior_rows(host_exe, name):
    st = US.STENCILS[name]()
    dim = US.dim_of(st)
    shape = SHAPES[dim]
    levels = host_levels(host_exe, shape, NLEVEL, st)
    orc = O.Oracle.stencil(shape, params(nlevel=NLEVEL), st)
    axis = name in ("C7", "C5", "S7")
    for l, (npoints, ncolours, refl, bits) in enumerate(levels):
        lshape = tuple(n >> l for n in shape)
        assert npoints == ((2 * dim + 1) if axis and l == 0 else 3 ** dim)
        assert ncolours == (2 if axis and l == 0 else 2 ** dim)
        want = oracle_interior_stencil(orc, l, lshape).view(np.uint64)
        assert np.array_equal(bits, want), (name, l, np.flatnonzero(bits != want))
        if l == 0:
            assert np.array_equal(bits[:len(st)], st.view(np.uint64))
        assert refl == US.reflection_symmetric(bits.view(np.float64)) * (dim == 3 and npoints == 27)
        if name in ("S7", "S27"):
            assert refl == (1 if npoints == 27 else 0), (name, l)
        else:
            assert refl == 0, (name, l)


@pytest.mark.parametrize("name", list(US.STENCILS))
def test_hierarchy_against_exact_rational_galerkin(host_exe, name):
    """Each level against R A R^T of the level above it (its computed stencil, an exact rational) evaluated in
    Fractions.  galerkin_stencil sums at most 3^d terms per entry of R A and at most 5^d per entry of (R A) R^T,
    all weights powers of two, so |computed - exact| <= gamma_m sum |terms| with m = 3^d + 5^d in any summation
    order.  The dyadic S7 / S27 are exact: their whole chain equals the exact Galerkin chain of the fixture."""
    st = US.STENCILS[name]()
    dim = US.dim_of(st)
    levels = host_levels(host_exe, SHAPES[dim], NLEVEL, st)
    np_ = 3 ** dim
    g = float(US.gamma(3 ** dim + 5 ** dim))
    worst = 0.0
    chain = [Fraction(float(v)) for v in st]
    for l in range(1, NLEVEL):
        fine = levels[l - 1][3].view(np.float64)[:np_]
        got = [Fraction(float(v)) for v in levels[l][3].view(np.float64)[:np_]]
        exact, mag = US.galerkin_exact(dim, fine)
        for a, b, m in zip(got, exact, mag):
            assert abs(a - b) <= Fraction(g) * m
            worst = max(worst, float(abs(a - b) / (Fraction(g) * m)))
        if name in ("S7", "S27"):
            chain, _ = US.galerkin_exact(dim, [float(v) for v in chain])
            assert got == chain, (name, l)
    print(f"{name}: max |error| / (gamma_m sum |terms|) = {worst:.3g}")
    if name in ("S7", "S27"):
        assert worst == 0.0


def _cycles(orc, f, ncycle=2):
    x = np.zeros(len(f))
    for _ in range(ncycle):
        orc.apply(f, x)
    return x


def test_oracle_stencil_equals_oracle_csr_c27():
    """No fold level: the stencil constructor is the CSR constructor on the assembled matrix, bit for bit."""
    shape, p = (24, 20, 12), params(nlevel=3)
    st = US.C27()
    A = US.csr(shape, st)
    a = O.Oracle.stencil(shape, p, st, seed=77)
    b = O.Oracle.csr(shape, p, A.indptr, A.indices, A.data, mode=O.MULTICOLOUR, seed=77)
    for l in range(3):
        ma, mb = a.csr_matrix(l), b.csr_matrix(l)
        assert np.array_equal(ma.indptr, mb.indptr) and np.array_equal(ma.indices, mb.indices)
        assert np.array_equal(ma.data.view(np.uint64), mb.data.view(np.uint64))
    f = np.random.default_rng(5).standard_normal(a.ndof())
    xa, xb = _cycles(a, f), _cycles(b, f)
    assert np.all(np.isfinite(xa)) and np.array_equal(xa.view(np.uint64), xb.view(np.uint64))


def test_oracle_stencil_folds_s27_residuals_only():
    """S27's levels are reflection-symmetric: Oracle.stencil sums their residuals class-folded, Oracle.csr (the
    device's matrix path) in CSR order.  Everything else is the same arithmetic, the folded residuals agree to
    rounding, and with set_no_fold the two constructors agree bit for bit again."""
    shape, p = (24, 20, 16), params(nlevel=3, smoother="SSOR", omega=1.1)
    st = US.S27()
    A = US.csr(shape, st)
    a = O.Oracle.stencil(shape, p, st, seed=78)
    b = O.Oracle.csr(shape, p, A.indptr, A.indices, A.data, mode=O.MULTICOLOUR, seed=78)
    O.set_no_fold(True)
    try:
        c = O.Oracle.stencil(shape, p, st, seed=78)
    finally:
        O.set_no_fold(False)
    rng = np.random.default_rng(6)
    differ = 0
    for l in range(3):
        n = a.ndof(l)
        assert np.array_equal(a.csr_matrix(l).data.view(np.uint64), b.csr_matrix(l).data.view(np.uint64))
        x, f = rng.standard_normal(n), rng.standard_normal(n)
        assert np.array_equal(a.operator_apply(l, x), b.operator_apply(l, x))
        for d in (mg.FORWARD, mg.BACKWARD):
            assert np.array_equal(a.smoother_apply(l, d, 2, f, x), b.smoother_apply(l, d, 2, f, x))
            assert np.array_equal(a.sor_sampler_apply(l, d, 3, 9, f, x), b.sor_sampler_apply(l, d, 3, 9, f, x))
        if l < 2:
            ra, rb = a.residual_restrict(l, f, x), b.residual_restrict(l, f, x)
            differ += not np.array_equal(ra, rb)
            assert O.residual_tolerance_ok(ra, rb, b.csr_matrix(l), f, x, lambda v: b.restrict(l, v))
            assert np.array_equal(c.residual_restrict(l, f, x), rb)
    assert differ == 2
    f = rng.standard_normal(a.ndof())
    xa, xb, xc = _cycles(a, f), _cycles(b, f), _cycles(c, f)
    assert np.array_equal(xb, xc) and not np.array_equal(xa, xb)
    assert np.max(np.abs(xa - xb)) < 1e-12 * np.max(np.abs(xb))


@pytest.mark.parametrize("name", list(US.STENCILS))
def test_stencil_of_csr_returns_the_fixture(name):
    """mgmc_stencil_of_csr (SparseMatrixOperator.constant_stencil, the adapter's fast path) recovers every
    fixture from its assembled matrix bit for bit, on a lattice with odd and even interior extents."""
    from multigridmc_amd.sampler import make_config
    st = US.STENCILS[name]()
    shape = (12, 10, 8) if US.dim_of(st) == 3 else (12, 10)
    op = mg.SparseMatrixOperator(mg.Lattice(*shape), US.csr(shape, st))
    got = op.constant_stencil(make_config(op, params(nlevel=2)))
    assert got is not None
    want = np.zeros(27)
    want[:len(st)] = st
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", ["C27", "S27"])
def test_exchanging_two_coefficients_changes_the_cycle(name):
    """Every pair of unequal off-centre coefficients exchanged in the oracle's stencil gives a different cycle: a
    kernel that reads one coefficient for another cannot pass the GPU tests' bitwise comparison.  (An exchange
    with the centre makes the diagonal negative and the Gibbs noise NaN.)"""
    shape, p = (8, 8, 8), params(nlevel=2)
    st = US.STENCILS[name]()
    f = np.random.default_rng(8).standard_normal(7 ** 3)
    base = _cycles(O.Oracle.stencil(shape, p, st), f, 1)
    assert np.all(np.isfinite(base))
    npairs = 0
    for i, j in itertools.combinations(range(27), 2):
        if st[i] == st[j] or 13 in (i, j):
            continue
        sw = st.copy()
        sw[i], sw[j] = st[j], st[i]
        npairs += 1
        assert not np.array_equal(_cycles(O.Oracle.stencil(shape, p, sw), f, 1), base), (i, j)
    # 26 * 25 / 2 pairs; S27's classes of 2, 2, 2, 4, 4, 4 and 8 equal entries take 3 + 18 + 28 of them
    assert npairs == (325 if name == "C27" else 325 - 49)


# measured: A x at <= 0.39 (27-point) / 0.54 (5-point) of its bound, R (f - A x) at <= 0.13 / 0.34; the GPU test
# asserts the same bound on the device's results
@pytest.mark.parametrize("case", US.HIGHPREC)
def test_oracle_against_longdouble(case):
    """The oracle's A x and R (f - A x) on every level of the GPU tests' C27 / C5 cases against the level's CSR
    product in np.longdouble (user_stencils.highprec_ratios, where the bound is derived)."""
    sname, shape, kw = US.CASES[case]
    p = params(**kw)
    O.set_threads(O.cpu_share())
    try:
        orc = O.Oracle.stencil(shape, p, US.STENCILS[sname]())
        rng = np.random.default_rng(19)
        worst = [0.0, 0.0]
        for l in range(p.nlevel):
            lshape = tuple(n >> l for n in shape)
            n = orc.ndof(l)
            x, f = rng.standard_normal(n), rng.standard_normal(n)
            st = oracle_interior_stencil(orc, l, lshape)[:3 ** len(shape)] if min(lshape) >= 4 else None
            if st is None:
                continue
            fc = orc.residual_restrict(l, f, x) if l + 1 < p.nlevel else None
            r = US.highprec_ratios(lshape, st, x, f, orc.operator_apply(l, x), fc)
            worst = [max(worst[0], r[0]), max(worst[1], r[1] or 0.0)]
    finally:
        O.set_threads(1)
    print(f"{case}: max |error| / bound: operator {worst[0]:.3f}, residual + restriction {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0
