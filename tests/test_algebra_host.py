"""The identities of tests/algebra.py on the CPU oracle's MULTICOLOUR mode (no GPU).

The GPU suite proves "device == MULTICOLOUR replay" bit for bit; these tests prove that the replayed algorithm is a
sampler of N(Q^-1 f, Q^-1): every sweep is the SOR splitting it claims to be (A), adds exactly one unit normal per
vertex and per measurement with the right scale (B), whole cycles leave Q^-1 invariant and draw nothing outside the
counter contract (C), and a cycle is the composition of those sweeps with the intergrid operators (D).  No
statistics: everything holds to rounding.  tests/test_gpu_algebra.py runs the same bodies on the device, at the
shapes that reach its fast kernels.

Largest ratios |lhs - rhs| / (EPS s) measured on the oracle (bound C_TOL = 8), per case: A / B / A and B at once:
    3d_24x20x12_w11 1.88 / 6.84 / 2.43    2d_34x18_w08 2.07 / 2.36 / 1.84    3d16 2.40 / 4.83 / 2.81
    2d32_point_global 0.45 / 0.68 / 0.34  3d32_ball_global 0.07 / 0.15 / 0.11
    fem2d32 2.09 / 3.57 / 2.25            c27_24x20x12 4.17 / 4.45 / 3.54
(B of 2d32_point_global is 75.7 at the three measured vertices without the Woodbury term of s,
algebra.LevelAlgebra._lowrank_terms; the two low-rank cases were 0.57 / 0.85 / 0.78 and 0.08 / 0.21 / 0.12 before s
took the rounding of u = B_bar (B^T y) as well, tests/test_lowrank_shapes_host.py.)  Whole cycles: CYCLE_REFERENCE below.
Matrix-built problems (Oracle.csr on the oracle's own assembly; the device takes them through mgmc_create_csr):
    m_fd_periodic_24x20x12_w11 2.09 / 4.32 / 2.59   m_fd_periodic_34x18_w08 1.53 / 3.79 / 2.18
    m_fem_periodic_16 2.52 / 5.31 / 2.77            m_squared_32 2.39 / 4.32 / 2.61 (9 colours on all 3 levels)
    m_squared_32_periodic 1.87 / 3.52 / 2.47 (9 colours, not symmetric)   m_dominant_16x12x8 2.33 / 3.48 / 2.32
  R (residual + restriction against P^T (b - A_l x) in scipy; bound: largest row + 1 + 3^d = 15 .. 55): ratio 0.00
  on every level of all six; G (A_l against P^T A_(l-1) P, bound 64 EPS max |A_l|): 0.0 on every level of all six.
Composition: m_fd_periodic_24x20x12_w11 9.68e-16, m_squared_32_ssor_W 1.60e-14; apply() equals the replay bit for
bit in both.

What the checks catch, shown on mutated copies of the oracle (never committed): the noise scale times 1.01 on
odd vertices -> B 8.9e13 (bound 8), stationarity 1.7e-2; the sweep tag & ~1 (two sweeps share a tag) ->
stationarity 0.34; the backward colour order ascending -> A 8.5e15; sqrt(1 / Sigma) replaced by 1 / Sigma in the
low-rank noise -> B 4.9e13, stationarity 24.  On m_fd_periodic_24x20x12_w11: the residual's row sum with the
diagonal of the pair's other vertex -> R 1.7e13 / 3.5e12 on levels 0 / 1 (bounds 35 / 55), composition 1.7e-2
(bound 1e-12); with one constant diagonal -> R 7.0e12 / 7.4e12, composition 4.1e-3; the noise scale times 1.01 ->
B 8.9e13 (A, R, G and the composition unchanged).
"""
import numpy as np
import pytest

from tests import algebra as AL
from tests import oracle_lib as O

# every high word set: seed and sample index above 2^32, a non-zero chain id, tags >= 2
SEED = 5418513 + (7 << 32)
CHAIN = 5
TAG = 3
SAMPLE = (1 << 32) + 17

SWEEP_CASES = {
    "3d_24x20x12_w11": dict(kind="fd", shape=(24, 20, 12), kw=dict(nlevel=3, omega=1.1)),
    "2d_34x18_w08": dict(kind="fd", shape=(34, 18), kw=dict(nlevel=3, omega=0.8)),
    "3d16": dict(kind="fd", shape=(16, 16, 16), kw=dict(nlevel=3)),
    "2d32_point_global": dict(kind="fd", shape=(32, 32), kw=dict(nlevel=3), meas=(0.0, 3, True)),
    "3d32_ball_global": dict(kind="fd", shape=(32, 32, 32), kw=dict(nlevel=3, ncoarsesmooth=2, omega=1.2),
                             meas=(0.1, 2, True)),
    "fem2d32": dict(kind="fem", shape=(32, 32), kw=dict(nlevel=3, omega=0.9)),
    "c27_24x20x12": dict(kind="stencil", shape=(24, 20, 12), kw=dict(nlevel=3), stencil="C27", symmetric=False),
    # matrix-built problems (mgmc_create_csr on the device): per-vertex coefficients, the squared operator's reach-2
    # levels in 9 colours (with periodic kappa^2 its matrix is not symmetric), a hand-made anisotropic matrix
    "m_fd_periodic_24x20x12_w11": dict(kind="matrix", pde="fd", shape=(24, 20, 12), kw=dict(nlevel=3, omega=1.1)),
    "m_fd_periodic_34x18_w08": dict(kind="matrix", pde="fd", shape=(34, 18), kw=dict(nlevel=3, omega=0.8)),
    "m_fem_periodic_16": dict(kind="matrix", pde="fem", shape=(16, 16, 16), kw=dict(nlevel=3)),
    "m_squared_32": dict(kind="matrix", pde="squared", model="constant", shape=(32, 32), kw=dict(nlevel=3)),
    "m_squared_32_periodic": dict(kind="matrix", pde="squared", shape=(32, 32), kw=dict(nlevel=3), symmetric=False),
    "m_dominant_16x12x8": dict(kind="matrix", pde="dominant", shape=(16, 12, 8), kw=dict(nlevel=2)),
}
MATRIX_CASES = [name for name, case in SWEEP_CASES.items() if case["kind"] == "matrix"]
NINE_COLOUR_CASES = ["m_squared_32", "m_squared_32_periodic"]


def problem(case):
    case = dict(case)
    case.pop("symmetric", None)
    return AL.Problem(**case)


def test_sweep_tags_follow_the_recursion():
    import multigridmc_amd as mg
    P = mg.MultigridParameters
    assert AL.sweep_tags(P(nlevel=1, ncoarsesmooth=3)) == 6
    assert AL.sweep_tags(P(nlevel=3, npresmooth=1, npostsmooth=1, ncoarsesmooth=2)) == 8
    assert AL.sweep_tags(P(nlevel=3, cycle=2, smoother="SSOR", npresmooth=1, npostsmooth=1, ncoarsesmooth=1)) == 16
    assert AL.sweep_tags(P(nlevel=3, coarse_solver="Cholesky", npresmooth=2, npostsmooth=0)) == 5


@pytest.mark.parametrize("name", ["2d32_point_global", "3d32_ball_global"])
def test_interpolation_and_coarse_measurements_from_the_definition(name):
    """P assembled from its definition is the oracle's prolongation, P^T its restriction, and B_l = P^T B_(l-1)
    are the oracle's coarse measurement columns."""
    prob = problem(SWEEP_CASES[name])
    mc = prob.oracle()
    rng = np.random.default_rng(2)
    lrs = prob.lowrank_levels()
    for level in range(prob.params.nlevel):
        B, sig, cnt = lrs[level]
        colptr, rows, vals = mc.lowrank(level)
        ref = AL.sp.csc_matrix((vals, rows, colptr), shape=B.shape)
        assert abs(ref - B).max() <= 4 * AL.EPS * abs(ref).max()
        assert np.array_equal(cnt, np.diff(colptr)) and np.array_equal(sig, prob.lowrank().sigma)
        if level + 1 < prob.params.nlevel:
            P = AL.interpolation(prob.level_shape(level))
            xc, r = rng.standard_normal(P.shape[1]), rng.standard_normal(P.shape[0])
            assert np.allclose(mc.prolongate_add(level, 1.0, xc, np.zeros(P.shape[0])), P @ xc, rtol=0, atol=1e-15)
            assert np.allclose(mc.restrict(level, r), P.T @ r, rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", list(SWEEP_CASES))
def test_sweeps_are_the_sor_splitting_with_unit_noise(name):
    """A and B on every level, both directions."""
    case = SWEEP_CASES[name]
    prob = problem(case)
    be = prob.oracle(seed=SEED, chain=CHAIN)
    ratios = AL.check_sweeps(prob, be, AL.oracle_normals(SEED, CHAIN), TAG, SAMPLE, np.random.default_rng(1),
                             symmetric=case.get("symmetric", True))
    worst = AL.report(name, ratios)
    assert worst <= AL.C_TOL, ratios


def check_matrix_levels(prob, be, symmetric, nine_colours, algebras=None):
    """R on every level of a matrix-built problem through `be`, G on its FAITHFUL matrices, and the colour count
    of the squared operator's levels (shared with tests/test_gpu_algebra.py)."""
    las = algebras or AL.level_algebras(prob, symmetric)
    if nine_colours:
        assert all(len(np.unique(la.colour)) == 9 for la in las), [len(np.unique(la.colour)) for la in las]
    for level, (ratio, bound) in AL.check_residuals(prob, be, np.random.default_rng(8), las).items():
        assert ratio <= bound, (level, ratio, bound)
    defects = AL.galerkin_defects(prob)
    assert len(defects) == prob.params.nlevel - 1 and max(defects) <= AL.GALERKIN_TOL, defects


@pytest.mark.parametrize("name", MATRIX_CASES)
def test_matrix_levels_restrict_residuals_and_are_galerkin_products(name):
    """R and G: the residual + restriction against P^T (b - A_l x) in scipy, and A_l = P^T A_(l-1) P."""
    case = SWEEP_CASES[name]
    prob = problem(case)
    check_matrix_levels(prob, prob.oracle(seed=SEED, chain=CHAIN), case.get("symmetric", True),
                        name in NINE_COLOUR_CASES)


# a batch's chain c draws the stream of chain id CHAIN + c.  With coarse_scaling 0 the coarse correction drops out
# of the cycle exactly, so one cycle with (npresmooth, npostsmooth) = (1, 0) is the forward sweep under tag 0 and
# with (0, 1) the backward sweep under the first tag after the coarse sampler's: B (and A) through the cycle itself
BATCH_SHAPE = (24, 20, 12)
BATCH_NCHAINS = 3


def batch_problem(shape, pre):
    return AL.Problem("fd", shape, dict(nlevel=2, npresmooth=pre, npostsmooth=1 - pre, ncoarsesmooth=2,
                                        coarse_scaling=0.0, omega=1.1))


def check_batch_chains(prob, states, f, x):
    """states[c]: chain c's state after one cycle at sample index SAMPLE from (f, x); the largest ratio."""
    p = prob.params
    direction, tag = (AL.FORWARD, 0) if p.npresmooth else (AL.BACKWARD, 2 * p.ncoarsesmooth)
    la = AL.level_algebras(prob)[0]
    worst = 0.0
    for c, xn in enumerate(states):
        worst = max(worst, la.noise_ratio(None, AL.oracle_normals(SEED, CHAIN + c), direction, tag, SAMPLE, f, x, xn=xn))
    assert not np.array_equal(states[0], states[1])
    return worst


@pytest.mark.parametrize("pre", [1, 0])
def test_chain_ids_of_a_batch_draw_their_own_unit_noise(pre):
    prob = batch_problem(BATCH_SHAPE, pre)
    rng = np.random.default_rng(4)
    f, x = rng.standard_normal(prob.lat.Nvertex), rng.standard_normal(prob.lat.Nvertex)
    states = [AL.cycle(prob.oracle(seed=SEED, chain=CHAIN + c), SAMPLE, x, f) for c in range(BATCH_NCHAINS)]
    worst = check_batch_chains(prob, states, f, x)
    print(f"algebra batch pre={pre}: max ratio {worst:.2f}")
    assert worst <= AL.C_TOL


# ------------------------------------------------------------------------------------------------
# C: whole cycles on tiny lattices (coarse_scaling 1: other values are not stationary by design)
# ------------------------------------------------------------------------------------------------
CYCLE_CASES = {
    "2d8_3lvl_cs2": dict(kind="fd", shape=(8, 8), kw=dict(nlevel=3, ncoarsesmooth=2)),
    "2d8_ssor_W": dict(kind="fd", shape=(8, 8), kw=dict(nlevel=3, cycle=2, smoother="SSOR", omega=1.1)),
    "2d8_chol": dict(kind="fd", shape=(8, 8), kw=dict(nlevel=3, coarse_solver="Cholesky", omega=0.9)),
    "2d8_ball_global": dict(kind="fd", shape=(8, 8), kw=dict(nlevel=3), meas=(0.2, 4, True)),
    "3d8_2lvl_cs2": dict(kind="fd", shape=(8, 8, 8), kw=dict(nlevel=2, ncoarsesmooth=2)),
    "fem2d8": dict(kind="fem", shape=(8, 8), kw=dict(nlevel=3, npresmooth=2)),
    "2d8_fd_periodic": dict(kind="matrix", pde="fd", shape=(8, 8), kw=dict(nlevel=3, ncoarsesmooth=2)),
    "2d8_fem_periodic_ssor_W": dict(kind="matrix", pde="fem", shape=(8, 8),
                                    kw=dict(nlevel=3, cycle=2, smoother="SSOR", omega=1.1)),
    "2d8_squared": dict(kind="matrix", pde="squared", model="constant", shape=(8, 8), kw=dict(nlevel=2)),
    "3d8_fd_periodic": dict(kind="matrix", pde="fd", shape=(8, 8, 8), kw=dict(nlevel=2, ncoarsesmooth=2)),
}
# (max |S + G Q - I|, max |W W^T - (Q^-1 - S Q^-1 S^T)| / max |Q^-1|) of the CPU oracle, the reference of both
# files; the bound is CYCLE_SLACK times it (conditioning of the fit), at least ten orders below the smallest defect
# worth catching (1e-6)
CYCLE_REFERENCE = {
    "2d8_3lvl_cs2": (1.62e-15, 1.32e-15),    # K 896, 560 columns, 8 tags, fit 1.1e-15
    "2d8_ssor_W": (1.89e-15, 1.16e-15),      # K 1613, 1008 columns, 16 tags, fit 1.2e-15
    "2d8_chol": (2.19e-15, 1.65e-15),        # K 628, 392 columns, 5 tags, fit 1.1e-15
    "2d8_ball_global": (5.75e-14, 2.00e-15),  # K 781, 488 columns, 6 tags, fit 1.3e-15 (Q carries B Sigma^-1 B^T)
    "3d8_2lvl_cs2": (1.95e-15, 1.52e-15),    # K 5018, 3136 columns, 6 tags, fit 1.4e-15
    "fem2d8": (1.47e-15, 1.68e-15),          # K 896, 560 columns, 8 tags, fit 1.0e-15
    "2d8_fd_periodic": (1.60e-15, 1.40e-15),          # K 896, 560 columns, 8 tags, fit 1.1e-15
    "2d8_fem_periodic_ssor_W": (1.25e-15, 1.93e-15),  # K 1613, 1008 columns, 16 tags, fit 1.3e-15
    "2d8_squared": (8.37e-14, 1.32e-15),              # K 538, 336 columns, 4 tags, fit 1.3e-15 (max |Q| = 1.6e5)
    "3d8_fd_periodic": (1.79e-15, 1.92e-15),          # K 5018, 3136 columns, 6 tags, fit 1.5e-15
}
CYCLE_SLACK = 100.0
FIT_TOL = 1e-11  # fit residual / max |eta|; also the bound of the rows of W that must vanish (a least-squares
#                  coefficient of unit-variance columns cannot exceed the residual it would otherwise leave)


def cycle_samples(ncolumns):
    """K = 1.6 x columns (chain, sample index) pairs, the sample indices straddling 2^32."""
    K = int(np.ceil(1.6 * ncolumns))
    return [(CHAIN, (1 << 32) - K // 2 + q) for q in range(K)]


def check_cycle_case(name, be):
    """C for one case on a backend built with (SEED, CHAIN); prints and returns the figures."""
    prob = problem(CYCLE_CASES[name])
    n = prob.lat.Nvertex
    lr = prob.lowrank()
    _, npairs = AL.normal_index(prob.shape)
    columns = (AL.sweep_tags(prob.params) + 2) * (2 * npairs + (lr.m if lr is not None else 0))
    samples = cycle_samples(columns)
    SG = AL.probe_cycle(be, n, samples[0][1])
    out = AL.cycle_identities(prob, lambda q, x, f: AL.cycle(be, samples[q][1], x, f),
                              lambda chain: AL.oracle_normals(SEED, chain), samples, SG)
    print(f"algebra cycle {name}: " + "  ".join(f"{k} {v:.3g}" for k, v in out.items()))
    ref_c, ref_s = CYCLE_REFERENCE[name]
    assert out["fit"] <= FIT_TOL, out
    assert out["extra_rows"] <= FIT_TOL, out
    assert out["consistency"] <= CYCLE_SLACK * ref_c, out
    assert out["stationarity"] <= CYCLE_SLACK * ref_s, out
    return out


@pytest.mark.parametrize("name", list(CYCLE_CASES))
def test_cycle_leaves_the_target_invariant(name):
    check_cycle_case(name, problem(CYCLE_CASES[name]).oracle(seed=SEED, chain=CHAIN))


# ------------------------------------------------------------------------------------------------
# D: cycles as the composition of the pieces, at shapes the CPU replays in a moment
# ------------------------------------------------------------------------------------------------
COMPOSITION_CASES = {
    "3d_24x20x12_w11": SWEEP_CASES["3d_24x20x12_w11"],
    "2d_34x18_ssor_W": dict(kind="fd", shape=(34, 18), kw=dict(nlevel=3, cycle=2, smoother="SSOR", npresmooth=2,
                                                               omega=0.8)),
    "2d32_point_global": SWEEP_CASES["2d32_point_global"],
    "m_fd_periodic_24x20x12_w11": SWEEP_CASES["m_fd_periodic_24x20x12_w11"],
    "m_squared_32_ssor_W": dict(kind="matrix", pde="squared", model="constant", shape=(32, 32),
                                kw=dict(nlevel=3, cycle=2, smoother="SSOR", npresmooth=2)),
}
CONSISTENCY_TOL = 1e-12  # the project's fixed-point tolerance


@pytest.mark.parametrize("name", list(COMPOSITION_CASES))
def test_cycle_is_the_composition_of_its_pieces(name):
    prob = problem(COMPOSITION_CASES[name])
    be = prob.oracle(seed=SEED, chain=CHAIN)
    consistency, same, diff = AL.composition(prob, be, SAMPLE, np.random.default_rng(6))
    print(f"algebra composition {name}: consistency {consistency:.3g}  replay max diff {diff:.3g}")
    assert consistency <= CONSISTENCY_TOL
    assert same, f"apply() differs from the replay over the component entry points by {diff:.3g}"
