"""GPU parity of the variable-diagonal fine level (-m gpu): a matrix handle whose fine matrix is a constant
symmetric 7-point stencil plus a diagonal field (mgmc_vardiag_of_csr: ShiftedLaplaceFDOperator with any
correlation-length model) runs k_zsweep_rb7<...,VD> and k_zresrestrict<7,64,4|8> with the diagonal streamed per
vertex instead of k_fsweep / k_fresidual + k_restrict.  Everything is compared bit for bit (np.array_equal) with
the CPU oracle's MULTICOLOUR replay of the same matrix, which the field kernels equal too (test_gpu_varcoef.py):

  labels; level-0 components with random x and f; whole cycles and a QoI series (random and zero right-hand side);
  the fallbacks under MGMC_DISABLE=zsweep / zrestrict (the same oracle results, hence the fast path's);
  a low-rank posterior; batched chains; NaN-poisoned LDS; and, independent of the oracle's replay, one noisy
  sweep per direction against the red-black SOR relation evaluated in numpy from the operator's matrix and the
  device's normals, within tests/algebra.py's C_TOL on its ratio.

  case  lattice      parameters
  A     64x22x10     nlevel 2: one x tile, a one-row last y tile, short z chunks in an up / down pair, a 64 x 4
                     restriction tile wider than the level
  B     128x34x18    nlevel 2, omega 0.9, coarse_scaling 0.9: the smallest z-sweep algebra shape
  C     192x48x40    nlevel 3, SSOR, 2 pre-sweeps, W-cycle: nx no multiple of 128, field coarse levels
  D     128x34x18    a hand-made matrix, cx != cy != cz and a random dominant diagonal: a coefficient mix-up shows
  E     128x18x3042  nlevel 2: z-chunks of 32 planes on 256 compute units, as at 256^3 (test_deep_chunks_bitwise)
  A_p_q, C_sor_W     A's lattice with (npresmooth, npostsmooth) = (0, 1), (1, 0), (0, 0), (3, 2); C's with a SOR
                     W-cycle (test_cycle_shapes_bitwise)

Measured on MI355X (test_sweep_against_the_red_black_relation, case B): worst ratio 2.93 forward, 3.07
backward, against C_TOL = 8.  Case E reports tz=32 on the MI355X's 256 compute units; its test takes 8.5 s, nearly
all of it the host's assembly, Galerkin product and the oracle's replay of 6.6 M unknowns (16 threads)."""
import functools

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd.parameters import MeasurementParameters
from tests import algebra as AL
from tests import oracle_lib as O
from tests.test_vardiag_host import dominant_matrix

pytestmark = pytest.mark.gpu

SEED = 5418513
PERIODIC = mg.PeriodicCorrelationLengthModel(0.2, 0.4)
CASES = {
    "A": ((64, 22, 10), dict(nlevel=2)),
    "B": ((128, 34, 18), dict(nlevel=2, omega=0.9, coarse_scaling=0.9)),
    "C": ((192, 48, 40), dict(nlevel=3, smoother="SSOR", npresmooth=2, cycle=2)),
    "D": ((128, 34, 18), dict(nlevel=2)),
    # the z-chunk depth of the 256^3 workload (test_deep_chunks_bitwise)
    "E": ((128, 18, 3042), dict(nlevel=2)),
    # cycle shapes (test_cycle_shapes_bitwise): A's and C's lattices
    "A_0_1": ((64, 22, 10), dict(nlevel=2, npresmooth=0, npostsmooth=1)),
    "A_1_0": ((64, 22, 10), dict(nlevel=2, npresmooth=1, npostsmooth=0)),
    "A_0_0": ((64, 22, 10), dict(nlevel=2, npresmooth=0, npostsmooth=0)),
    "A_3_2": ((64, 22, 10), dict(nlevel=2, npresmooth=3, npostsmooth=2)),
    "C_sor_W": ((192, 48, 40), dict(nlevel=3, cycle=2)),
}
SMALL = ["A", "B", "C", "D"]
SHAPES = ["A_0_1", "A_1_0", "A_0_0", "A_3_2", "C_sor_W"]
FIELD_SWEEP, FIELD_RES = "k_fsweep<3>", "k_fresidual + k_restrict"


def params(name):
    return mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **CASES[name][1]})


def operator(name, lowrank=False):
    return build_operator(CASES[name][0], name == "D", lowrank)


def build_operator(shape, dominant=False, lowrank=False):
    """(operator, lattice): the periodic-kappa^2 FD operator or the hand-made dominant matrix on `shape` cells (also
    what tests/tuning_worker.py and tests/test_gpu_tuning.py build for their variable-diagonal cases)."""
    lat = mg.Lattice(*shape)
    op = mg.SparseMatrixOperator(lat, dominant_matrix(shape)) if dominant else mg.ShiftedLaplaceFDOperator(lat, PERIODIC)
    if lowrank:  # 3 point measurements and the global average, as test_gpu_varcoef.make(lowrank=True)
        rng = np.random.default_rng(3)
        mp = MeasurementParameters(radius=0.0, variance_scaling=1e-3, measure_global=True, variance_global=0.02)
        mp.measurement_locations = [list(rng.uniform(0.15, 0.85, lat.dim)) for _ in range(3)]
        mp.variance = list(1.0 + 2.0 * rng.random(3))
        op = mg.MeasuredOperator(op, mp)
    return op, lat


def sampler(name, lowrank=False, chain=0, nchains=1):
    op, lat = operator(name, lowrank)
    return mg.MultigridMCSampler(op, SEED, params(name), device=0, chain_id=chain, nchains=nchains), lat


def oracle(name, lowrank=False, chain=0):
    op, lat = operator(name, lowrank)
    rowptr, col, val = getattr(op, "base_operator", op).get_csr()
    mc = O.Oracle.csr(CASES[name][0], params(name), rowptr, col, val, mode=O.MULTICOLOUR, seed=SEED)
    if chain:
        mc.reseed(SEED, chain)
    if lowrank:
        mc.set_lowrank(op.get_B())
    return mc


def rhs(name, zero):
    n = int(np.prod([m - 1 for m in CASES[name][0]]))
    return np.zeros(n) if zero else np.random.default_rng(7).standard_normal(n)


def qoi(lat):
    return mg.measurement_vector_index(lat, [0.5] * lat.dim)


# ---- the oracle's results, computed once per (case, ...) and shared by the tests that compare with them ----
@functools.lru_cache(maxsize=None)
def ref_cycles(name, zero=False, lowrank=False, chain=0):
    """(state after two apply(f, x) from zero, the 5-sample QoI series after it, the final state)"""
    mc = oracle(name, lowrank, chain)
    f = rhs(name, zero)
    x = np.zeros(len(f))
    for _ in range(2):
        mc.apply(f, x)
    mc.set_rhs(f)
    mc.set_state(x)
    series = mc.sample(5, qoi(mg.Lattice(*CASES[name][0])))
    out = (x, series, mc.get_state())
    for v in out:
        v.setflags(write=False)
    return out


def component_inputs(name):
    n = int(np.prod([m - 1 for m in CASES[name][0]]))
    rng = np.random.default_rng(5)
    return rng.standard_normal(n), rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def ref_components(name):
    mc = oracle(name)
    x, b = component_inputs(name)
    out = {"apply": mc.operator_apply(0, x), "residual": mc.residual_restrict(0, b, x)}
    for d in (mg.FORWARD, mg.BACKWARD):
        out["smoother", d] = mc.smoother_apply(0, d, 2, b, x)
        out["sampler", d] = mc.sor_sampler_apply(0, d, 3, 19, b, x)
    return out


def check_cycles(s, lat, name, zero=False, lowrank=False, chain=0):
    x_ref, series_ref, final_ref = ref_cycles(name, zero, lowrank, chain)
    f = rhs(name, zero)
    x = np.zeros(lat.Nvertex)
    for _ in range(2):
        s.apply(f, x)
    assert np.array_equal(x, x_ref), "two cycles"
    s.fix_rhs(f)
    s.set_state(x)
    assert np.array_equal(s.sample(5, qoi(lat)), series_ref), "QoI series"
    assert np.array_equal(s.get_state(), final_ref), "final state"


def check_components(s, name):
    ref = ref_components(name)
    x, b = component_inputs(name)
    for d in (mg.FORWARD, mg.BACKWARD):
        assert np.array_equal(s.sor_sampler_apply(0, d, 3, 19, b, x), ref["sampler", d]), f"sampler {d}"
        assert np.array_equal(s.smoother_apply(0, d, 2, b, x), ref["smoother", d]), f"smoother {d}"
    assert np.array_equal(s.residual_restrict(0, b, x), ref["residual"]), "residual + restriction"
    assert np.array_equal(s.operator_apply(0, x), ref["apply"]), "operator"


def assert_fast_labels(s):
    k0 = s.level_kernels(0)
    assert k0["sweep"].startswith("k_zsweep_rb7<") and k0["residual_restrict"].startswith("k_zresrestrict<7,"), k0
    assert k0.get("diag") == "field" and "post_sweep" not in k0 and "rhs" not in k0, k0
    assert s.level_desc(0)["varcoef"]


# 1
@pytest.mark.parametrize("name", SMALL)
def test_labels(hip_device, name):
    s, lat = sampler(name)
    assert_fast_labels(s)
    s.fix_rhs(np.zeros(lat.Nvertex))  # a variable-diagonal level is never marked rhs=zero
    assert_fast_labels(s)
    if s.nlevel > 2:  # (with two levels, level 1 is the coarse sampler's)
        k1 = s.level_kernels(1)
        assert k1["sweep"] == FIELD_SWEEP and k1["residual_restrict"] == FIELD_RES and "diag" not in k1, k1
    s.close()


# 2
@pytest.mark.parametrize("name", SMALL)
def test_components_bitwise(hip_device, name):
    s, lat = sampler(name)
    assert_fast_labels(s)
    check_components(s, name)
    s.close()


# 3
@pytest.mark.parametrize("name,zero", [(n, False) for n in SMALL] + [("A", True), ("B", True)])
def test_cycles_bitwise(hip_device, name, zero):
    s, lat = sampler(name)
    check_cycles(s, lat, name, zero)
    assert_fast_labels(s)
    s.close()


# 4
@pytest.mark.parametrize("name", ["A", "B", "D"])
@pytest.mark.parametrize("token", ["zrestrict", "zsweep"])
def test_fallbacks_bitwise(hip_device, monkeypatch, name, token):
    monkeypatch.setenv("MGMC_DISABLE", token)
    s, lat = sampler(name)
    k0 = s.level_kernels(0)
    if token == "zrestrict":
        assert k0["sweep"].startswith("k_zsweep_rb7<") and k0.get("diag") == "field", k0
    else:
        assert k0["sweep"] == FIELD_SWEEP and "diag" not in k0, k0
    assert k0["residual_restrict"] == FIELD_RES, k0
    check_cycles(s, lat, name)
    check_components(s, name)
    s.close()


# 5
def test_posterior_bitwise(hip_device):
    s, lat = sampler("B", lowrank=True)
    assert_fast_labels(s)
    assert "rhs_inplace" not in s.level_kernels(0)["lowrank"], s.level_kernels(0)
    check_cycles(s, lat, "B", lowrank=True)
    s.close()


# 6
def test_batched_chains_bitwise(hip_device):
    s, lat = sampler("B", chain=5, nchains=3)
    assert_fast_labels(s)
    f = rhs("B", False)
    s.fix_rhs(f)
    s.set_state(np.zeros(lat.Nvertex))
    series = s.sample(5, qoi(lat), chain=None)
    for c in range(3):
        mc = oracle("B", chain=5 + c)
        mc.set_rhs(f)
        mc.set_state(np.zeros(lat.Nvertex))
        assert np.array_equal(series[c], mc.sample(5, qoi(lat))), f"chain {c} series"
        assert np.array_equal(s.get_state(c), mc.get_state()), f"chain {c} final state"
    assert not np.array_equal(series[0], series[1])
    s.close()


# 7
@pytest.mark.parametrize("name", ["A", "C"])
def test_poisoned_lds_bitwise(hip_device, monkeypatch, name):
    monkeypatch.setenv("MGMC_POISON", "1")
    s, lat = sampler(name)
    assert_fast_labels(s)
    check_components(s, name)
    f = rhs(name, False)
    x = np.zeros(lat.Nvertex)
    s.apply(f, x)
    mc = oracle(name)
    xr = np.zeros(lat.Nvertex)
    mc.apply(f, xr)
    assert np.array_equal(x, xr)
    s.close()


# 8
def test_sweep_against_the_red_black_relation(hip_device):
    """One noisy sweep per direction on case B against the red-black SOR relation, in numpy from op.get_csr() and
    s.normals(): first colour x' = x + (omega / d)(f + sd xi - A x), second colour the same with the first colour
    updated -- in the splitting form M (x' - x) = f + sd xi - A x, M = D / omega + the couplings towards the
    first colour (tests/algebra.py A / B), with its ratio |lhs - rhs| / (EPS sum |terms|) and its bound C_TOL.
    Measured on MI355X: 2.93 forward, 3.07 backward (the constant-stencil z-sweep: at most 5.6)."""
    name = "B"
    s, lat = sampler(name)
    assert_fast_labels(s)
    shape, p = CASES[name][0], params(name)
    nx, ny, nz = shape
    rowptr, col, val = operator(name)[0].get_csr()
    A = mg.sampler_csr_matrix(rowptr, col, val, lat.Nvertex).tocsr()
    i, j, k = AL.coords(shape)
    colour = (i + j + k) & 1
    pair = ((k - 1) * (ny - 1) + (j - 1)) * (nx // 2) + (i - 1) // 2
    index = 2 * pair + (1 - (i & 1))  # the cos branch belongs to odd i
    npairs = (nz - 1) * (ny - 1) * (nx // 2)
    assert len(np.unique(index)) == lat.Nvertex and index.max() < 2 * npairs
    d = A.diagonal()
    sd = np.sqrt(d * (2.0 - p.omega) / p.omega)
    Mf, Mb = AL.splitting(A, colour, p.omega)
    absA = abs(A)
    rng = np.random.default_rng(13)
    worst = {}
    for direction, M in ((mg.FORWARD, Mf), (mg.BACKWARD, Mb)):
        f, x = rng.standard_normal(lat.Nvertex), rng.standard_normal(lat.Nvertex)
        tag, sample = 40 + direction, 23
        xn = s.sor_sampler_apply(0, direction, tag, sample, f, x)
        assert np.all(np.isfinite(xn))
        xi = s.normals(0, 2 * npairs, tag, sample)[index]
        lhs = M @ (xn - x) - (f - A @ x)
        scale = abs(M) @ (np.abs(xn) + np.abs(x)) + np.abs(f) + absA @ np.abs(x)
        worst[direction] = float(np.max(np.abs(lhs - sd * xi) / (AL.EPS * scale)))
    print("vardiag z-sweep against the red-black relation: worst ratio forward %.2f backward %.2f"
          % (worst[mg.FORWARD], worst[mg.BACKWARD]))
    assert max(worst.values()) <= AL.C_TOL, worst
    s.close()


def assert_same(got, ref, what):
    bad = np.flatnonzero(got != ref)
    assert got.shape == ref.shape and bad.size == 0, \
        f"{what}: {bad.size} of {ref.size} values differ, first at {bad[:1]}, last at {bad[-1:]}"


# 9
def test_deep_chunks_bitwise(hip_device):
    """Case E, 128 x 18 x 3042: the smallest lattice on which the VD sweep keeps the z-chunk depth ZS_TZ = 32 of the
    256^3 workload on 256 compute units (zsweep_depth halves it while 4 tiles_xy nchunks < 6 num_cu): two x tiles, a
    full and a one-row y tile of ZS_TYP = 16 rows, 96 chunks of which the last is a single plane -- 4 * 4 * 96 =
    1536 = 3 * 2 * 256.  Every other VD case of the suite runs 8-plane chunks.  Noisy sweeps, the smoother, the
    residual + restriction and one cycle, bit for bit against the oracle."""
    from tests.tuning_worker import num_cu
    name = "E"
    s, lat = sampler(name)
    O.set_threads(min(16, O.cpu_share()))
    try:
        assert_fast_labels(s)
        k0 = s.level_kernels(0)
        assert k0["tz"] == "32", f"{k0}: the lattice is sized for 256 compute units, the device reports {num_cu()}"
        mc = oracle(name)
        x, b = component_inputs(name)
        for d in (mg.FORWARD, mg.BACKWARD):
            assert_same(s.sor_sampler_apply(0, d, 3, 19, b, x), mc.sor_sampler_apply(0, d, 3, 19, b, x), f"sampler {d}")
            assert_same(s.smoother_apply(0, d, 2, b, x), mc.smoother_apply(0, d, 2, b, x), f"smoother {d}")
        assert_same(s.residual_restrict(0, b, x), mc.residual_restrict(0, b, x), "residual + restriction")
        f = rhs(name, False)
        got, ref = np.zeros(lat.Nvertex), np.zeros(lat.Nvertex)
        s.apply(f, got)
        mc.apply(f, ref)
        assert_same(got, ref, "one cycle")
    finally:
        O.set_threads(1)
        s.close()


# 10
@pytest.mark.parametrize("name", SHAPES)
def test_cycle_shapes_bitwise(hip_device, name):
    """A VD level has no fused prolongation and is never rhs=zero: its out-of-place sweeps (x -> x2) alternate with
    a separate prolongation, so the buffer a cycle ends in depends on the sweep counts.  (npresmooth, npostsmooth)
    = (0, 1), (1, 0), (0, 0), (3, 2) on A's lattice and a SOR W-cycle above a field level on C's: two cycles and a
    5-sample series."""
    s, lat = sampler(name)
    try:
        assert_fast_labels(s)
        check_cycles(s, lat, name)
        assert_fast_labels(s)
        if s.nlevel > 2:
            k1 = s.level_kernels(1)
            assert k1["sweep"] == FIELD_SWEEP and k1["residual_restrict"] == FIELD_RES, k1
    finally:
        s.close()
