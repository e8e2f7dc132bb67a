"""The identities of tests/algebra.py on the device (-m gpu), at the smallest shapes that reach each fast kernel.

Every other GPU test compares device bits with the oracle's MULTICOLOUR replay or is statistical at sizes where
only k_tail, k_coarse_ssor_lds and the generic passes run.  Here the device itself is held to exact sparse linear
algebra: each sweep of each level is the SOR splitting it claims to be (A), adds one unit normal per vertex and
measurement with the right scale (B, and A and B at once through the kernel the cycle runs on the level), whole
cycles leave Q^-1 invariant and draw nothing outside the counter contract (C), and fast-path cycles are the
composition of the sweeps with the intergrid operators (D).  The matrices come from the FAITHFUL oracle and the
operators' own data, never from the device; the oracle's MULTICOLOUR mode is not used.  Every case asserts the
kernel labels it exists for.  Bounds and tiny-lattice cases are those of tests/test_algebra_host.py.

Largest ratios |lhs - rhs| / (EPS s) measured on the MI355X (bound C_TOL = 8): A / B / A and B at once:
    3d_128x34x18 3.31 / 5.32 / 3.61   3d_192x48x40 2.95 / 5.58 / 4.51        3d_512x16x24 3.41 / 5.38 / 3.64
    3d_96x48x48 3.37 / 5.16 / 3.63    3d_96x48x48_points 3.37 / 5.16 / 3.63  3d_320x24x16 3.35 / 4.83 / 3.45
    2d_200x120 2.76 / 4.45 / 2.72     2d_256x128 2.55 / 4.54 / 2.44          fem2d64 2.48 / 4.31 / 2.69
    c27_24x20x12 4.17 / 4.45 / 3.54   2d32_point_global 0.57 / 0.85 / 0.78   3d32_ball_global 0.08 / 0.21 / 0.12
    three batched chains through the cycle: 3.05 (pre-sweep), 3.32 (post-sweep)
Whole cycles (consistency / stationarity; reference and bound in test_algebra_host.CYCLE_REFERENCE):
    2d8_3lvl_cs2 1.62e-15 / 1.32e-15  2d8_ssor_W 1.89e-15 / 1.49e-15  2d8_chol 2.19e-15 / 1.49e-15
    2d8_ball_global 5.75e-14 / 1.45e-15  3d8_2lvl_cs2 1.95e-15 / 2.08e-15  fem2d8 1.47e-15 / 1.68e-15
    fit residuals 1.0e-15 .. 1.6e-15, rows of W under tags T, T + 1 below 8e-17 of max |eta|
Composition: T_k(mu, Q mu) - T_k(0, 0) = mu to 2.08e-15 (3d_jsweep_tail), 1.36e-15 (2d_200x120), 8.13e-14
(3d_96x48x48_points); apply() equals the replay bit for bit in all three, no op needed the componentwise bound.

Matrix handles (mgmc_create_csr: Problem kind "matrix"; the matrices from the oracle's own assembly and scipy
products, the reach-2 colours from the rule in mgmc_field.hpp), measured on the MI355X, A / B / A and B at once:
    vd_128x34x18 2.66 / 5.35 / 3.36   vd_192x48x40 4.18 / 5.19 / 3.57   vd_dominant_128x34x18 4.42 / 6.04 / 4.28
    field2d_fd_periodic_64 1.92 / 3.93 / 2.22   field3d_fem_periodic_16 2.52 / 5.31 / 2.77
    field2d_squared_32 2.39 / 4.32 / 2.61       field2d_squared_32_periodic 1.87 / 3.52 / 2.47
  R (residual_restrict against P^T (b - A_l x) in scipy; bound: largest row + 1 + 3^d = 15 .. 55): ratio 0.00 on every
  level of all seven (k_zresrestrict<7,64,4,...,VD>, k_fresidual + k_restrict: separate multiplies and adds in
  ascending column order, the order scipy sums in); G: 0.0 on every level.
  Whole cycles: 2d8_fd_periodic 1.60e-15 / 1.40e-15  2d8_fem_periodic_ssor_W 1.25e-15 / 1.59e-15
  2d8_squared 8.37e-14 / 1.02e-15  3d8_fd_periodic 1.79e-15 / 1.54e-15 (fit 1.1e-15 .. 1.3e-15, extra rows < 8e-17).
  Composition: vd_192x48x40_ssor_W 2.97e-15, field2d_squared_32_ssor_W 1.53e-14, bit for bit both.
The vd_* cases run with every high word of seed, chain, tag and sample index set: the VD sweep's noise is held to
the full 64-bit counter contract here.
"""
import numpy as np
import pytest

from tests import algebra as AL
from tests import test_algebra_host as H

pytestmark = pytest.mark.gpu

SEED, CHAIN, TAG, SAMPLE = H.SEED, H.CHAIN, H.TAG, H.SAMPLE

ZS = {"sweep^": "k_zsweep_rb7<", "post_sweep^": "k_zsweep_rb7<"}
VD = {"sweep^": "k_zsweep_rb7<", "sweep$": ",VD>", "residual_restrict^": "k_zresrestrict<7,", "diag": "field"}
FIELD3 = {"sweep": "k_fsweep<3>", "residual_restrict": "k_fresidual + k_restrict"}
# name: (problem, labels per level: {key: value}, "key^" a prefix)
SWEEP_CASES = {
    # k_zsweep_rb7, plain and fused-prolongation instance; partial tiles in y and z
    "3d_128x34x18": (dict(kind="fd", shape=(128, 34, 18), kw=dict(nlevel=2, omega=0.9)), {0: ZS}),
    "3d_192x48x40": (dict(kind="fd", shape=(192, 48, 40), kw=dict(nlevel=2)), {0: ZS}),
    # j-marching half-sweeps of 128 pairs on level 1 below a z-marching 27-point residual + restriction
    "3d_512x16x24": (dict(kind="fd", shape=(512, 16, 24), kw=dict(nlevel=3, omega=1.1)),
                     {0: ZS, 1: {"sweep": "k_jsweep_half<128>", "residual_restrict^": "k_zresrestrict<27,"}}),
    # three-load window quad passes (24-pair rows), prior and with 4 point measurements
    "3d_96x48x48": (dict(kind="fd", shape=(96, 48, 48), kw=dict(nlevel=3)),
                    {1: {"sweep": "k_sweep_quads<3>", "quads": "window"}}),
    "3d_96x48x48_points": (dict(kind="fd", shape=(96, 48, 48), kw=dict(nlevel=3), meas=(0.0, 4, False)),
                           {1: {"sweep": "k_sweep_quads<3>", "quads": "window", "lowrank": "small"},
                            0: {"lowrank": "small"}}),
    # colour-pair passes of 80 pairs
    "3d_320x24x16": (dict(kind="fd", shape=(320, 24, 16), kw=dict(nlevel=3, omega=1.2)),
                     {0: ZS, 1: {"sweep": "k_sweep_pairs<3>"}}),
    # k_rb2d, the 2D quad passes with the fused last pre-sweep + restriction, 2D tails
    "2d_200x120": (dict(kind="fd", shape=(200, 120), kw=dict(nlevel=4, omega=0.8)),
                   {0: {"sweep": "k_rb2d"}, 1: {"sweep^": "k_sweep_quads<2>", "residual_restrict": "k_quads_restrict2d"},
                    2: {"sweep": "k_tail<2>"}, 3: {"sweep": "k_tail<2>"}}),
    "2d_256x128": (dict(kind="fd", shape=(256, 128), kw=dict(nlevel=3)),
                   {0: {"sweep": "k_rb2d"}, 1: {"sweep^": "k_sweep_quads<2>", "residual_restrict": "k_quads_restrict2d"}}),
    # a 9-point fine level (FEM) in the quad passes
    "fem2d64": (dict(kind="fem", shape=(64, 64), kw=dict(nlevel=4, cycle=2)), {0: {"sweep^": "k_sweep_quads<2>"}}),
    # a user stencil with 26 distinct off-centre coefficients (not symmetric): window quads, odd-extent tails
    "c27_24x20x12": (H.SWEEP_CASES["c27_24x20x12"],
                     {0: {"sweep": "k_sweep_quads<3>", "quads": "window"}, 1: {"sweep": "k_tail<3>"},
                      2: {"sweep": "k_tail<3>"}}),
    # low-rank levels: the small path and the dense global column
    "2d32_point_global": (H.SWEEP_CASES["2d32_point_global"],
                          {0: {"sweep": "k_rb2d", "lowrank": "small"}, 1: {"sweep": "k_tail<2>", "lowrank": "small"},
                           2: {"sweep": "k_tail<2>", "lowrank": "small"}}),
    "3d32_ball_global": (H.SWEEP_CASES["3d32_ball_global"],
                         {0: {"lowrank": "dense"}, 1: {"sweep": "k_sweep_pairs<3>", "lowrank": "small"},
                          2: {"lowrank": "small"}}),
    # ---- matrix handles (mgmc_create_csr); these also run R on every level and G (H.check_matrix_levels) ----
    # the variable-diagonal z-marching instances: periodic kappa^2 and the hand-made anisotropic matrix; with three
    # levels a field level (k_fsweep, k_fresidual + k_restrict) below them
    "vd_128x34x18": (dict(kind="matrix", pde="fd", shape=(128, 34, 18), kw=dict(nlevel=2, omega=0.9)), {0: VD}),
    "vd_192x48x40": (dict(kind="matrix", pde="fd", shape=(192, 48, 40), kw=dict(nlevel=3)), {0: VD, 1: FIELD3}),
    "vd_dominant_128x34x18": (dict(kind="matrix", pde="dominant", shape=(128, 34, 18), kw=dict(nlevel=2)), {0: VD}),
    # the field kernels with 2 (red-black), 8 (parities) and 9 (coordinates mod 3) colours
    "field2d_fd_periodic_64": (dict(kind="matrix", pde="fd", shape=(64, 64), kw=dict(nlevel=4)),
                               {0: {"sweep": "k_fsweep<2>", "ncolours": 2}}),
    "field3d_fem_periodic_16": (dict(kind="matrix", pde="fem", shape=(16, 16, 16), kw=dict(nlevel=3)),
                                {0: {"sweep": "k_fsweep<3>", "ncolours": 8}}),
    "field2d_squared_32": (H.SWEEP_CASES["m_squared_32"], {0: {"sweep": "k_fsweep<2>", "ncolours": 9}, 1: {"ncolours": 9}}),
    "field2d_squared_32_periodic": (H.SWEEP_CASES["m_squared_32_periodic"],
                                    {0: {"sweep": "k_fsweep<2>", "ncolours": 9}, 1: {"ncolours": 9}}),
}
NINE_COLOUR_CASES = ["field2d_squared_32", "field2d_squared_32_periodic"]


def assert_labels(s, nlevel, labels, name):
    """key^: a prefix, key$: a suffix; ncolours is the level description's colour count."""
    got = [s.level_kernels(level) for level in range(nlevel)]
    print(f"algebra {name} kernels:", *(";".join(f"{k}={v}" for k, v in d.items()) for d in got), sep="\n  ")
    for level, want in labels.items():
        k = got[level]
        for key, value in want.items():
            if key == "ncolours":
                assert s.level_desc(level)["ncolours"] == value, (name, level, s.level_desc(level))
            elif key.endswith("^"):
                assert k.get(key[:-1], "").startswith(value), (name, level, k)
            elif key.endswith("$"):
                assert k.get(key[:-1], "").endswith(value), (name, level, k)
            else:
                assert k.get(key) == value, (name, level, k)


@pytest.mark.parametrize("name", list(SWEEP_CASES))
def test_sweeps_are_the_sor_splitting_with_unit_noise(hip_device, name):
    """A and B on every level of the hierarchy, both directions; the k_tail-range levels come along."""
    case, labels = SWEEP_CASES[name]
    prob = H.problem(case)
    s = prob.sampler(seed=SEED, chain=CHAIN)
    assert_labels(s, prob.params.nlevel, labels, name)
    las = AL.level_algebras(prob, case.get("symmetric", True))
    ratios = AL.check_sweeps(prob, s, s.normals, TAG, SAMPLE, np.random.default_rng(1), algebras=las)
    try:
        worst = AL.report(name, ratios)
        assert worst <= AL.C_TOL, ratios
        if case["kind"] == "matrix":  # R on every level through the device, G on the matrices it is held to
            H.check_matrix_levels(prob, s, case.get("symmetric", True), name in NINE_COLOUR_CASES, algebras=las)
    finally:
        s.close()


@pytest.mark.parametrize("pre", [1, 0])
def test_chain_ids_of_a_batch_draw_their_own_unit_noise(hip_device, pre):
    """Three chains in one handle, through the cycle's own batched fine sweeps (the z-sweep's plain instance for
    the pre-sweep, its fused-prolongation instance for the post-sweep): chain c satisfies A and B with the
    normals of chain id CHAIN + c."""
    prob = H.batch_problem((128, 34, 18), pre)
    s = prob.sampler(seed=SEED, chain=CHAIN, nchains=H.BATCH_NCHAINS)
    assert_labels(s, 2, {0: ZS}, f"batch pre={pre}")
    rng = np.random.default_rng(4)
    f, x = rng.standard_normal(prob.lat.Nvertex), rng.standard_normal(prob.lat.Nvertex)
    s.fix_rhs(f)
    s.set_state(x)
    s.set_sample_index(SAMPLE)
    s.sample(1)
    states = [s.get_state(c) for c in range(H.BATCH_NCHAINS)]
    s.close()
    worst = H.check_batch_chains(prob, states, f, x)
    print(f"algebra batch pre={pre}: max ratio {worst:.2f}")
    assert worst <= AL.C_TOL


@pytest.mark.parametrize("name", list(H.CYCLE_CASES))
def test_cycle_leaves_the_target_invariant(hip_device, name):
    """C on the device, against the oracle's reference values (never the device's own)."""
    s = H.problem(H.CYCLE_CASES[name]).sampler(seed=SEED, chain=CHAIN)
    try:
        H.check_cycle_case(name, s)
    finally:
        s.close()


COMPOSITION_CASES = {
    # z-sweep + j-marching + quads + tail, prior
    "3d_jsweep_tail": (dict(kind="fd", shape=(512, 32, 32), kw=dict(nlevel=5)),
                       {0: ZS, 1: {"sweep^": "k_jsweep_half<128"}, 2: {"sweep": "k_sweep_quads<3>"},
                        3: {"sweep": "k_tail<3>"}, 4: {"sweep": "k_tail<3>"}}),
    "2d_200x120": SWEEP_CASES["2d_200x120"],
    "3d_96x48x48_points": SWEEP_CASES["3d_96x48x48_points"],
    # matrix handles: the VD level's out-of-place sweeps alternating with the separate prolongation above a field
    # level, and the 9-colour field levels; SSOR, W-cycles
    "vd_192x48x40_ssor_W": (dict(kind="matrix", pde="fd", shape=(192, 48, 40),
                                 kw=dict(nlevel=3, cycle=2, smoother="SSOR", npresmooth=2)), {0: VD, 1: FIELD3}),
    "field2d_squared_32_ssor_W": (dict(kind="matrix", pde="squared", model="constant", shape=(32, 32),
                                       kw=dict(nlevel=3, cycle=2, smoother="SSOR")),
                                  {0: {"sweep": "k_fsweep<2>", "ncolours": 9}}),
}


@pytest.mark.parametrize("name", list(COMPOSITION_CASES))
def test_cycle_is_the_composition_of_its_pieces(hip_device, name):
    """D: T_k(mu, Q mu) - T_k(0, 0) = mu, and apply() equals the reference recursion over the component entry
    points bit for bit (after + 0.0: the fused prolongation may differ in the sign of an exact zero)."""
    case, labels = COMPOSITION_CASES[name]
    prob = H.problem(case)
    s = prob.sampler(seed=SEED, chain=CHAIN)
    assert_labels(s, prob.params.nlevel, labels, name)
    consistency, same, diff = AL.composition(prob, s, SAMPLE, np.random.default_rng(6))
    s.close()
    print(f"algebra composition {name}: consistency {consistency:.3g}  replay max diff {diff:.3g}")
    assert consistency <= H.CONSISTENCY_TOL
    assert same, f"apply() differs from the replay over the component entry points by {diff:.3g}"
