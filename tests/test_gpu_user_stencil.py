"""User stencils on the GPU (-m gpu): every hand-written stencil kernel with coefficients that are all distinct.

The stencil kernels take their 5 / 7 / 9 / 27 coefficients as arguments and index them by offset.  The other GPU
suites feed them the shifted-Laplace FD / FEM stencils and their Galerkin products only, whose mirror partners
a(-d), a(+d) are bitwise equal or one ulp apart: a kernel reading a mirrored or permuted coefficient passes there
wherever the pair happens to be equal, and the SYM / fold instances run exactly where every extent is a power of
two.  Here the fixtures of tests/user_stencils.py (no symmetry: C27, C9, C7, C5; symmetric matrix only: P27;
dyadic and reflection-symmetric on every level at any shape: S7, S27) go through the user-stencil fast path --
MultigridMCSampler(SparseMatrixOperator(lattice, A)) -> mgmc_stencil_of_csr -> mgmc_create_stencil_batch, the path
the reference-side adapter takes for a constant-coefficient get_sparse() -- at the smallest shapes of the existing
suites that reach each instance (user_stencils.CASES).  Per case:

  * the handle took the stencil path (varcoef == 0), and every level reports the kernels and the fold flag the
    case is there for (a plan change that moves a case off its kernel fails here);
  * components on every level -- operator, both directions of the deterministic and the noisy sweep, restriction,
    prolongation, residual + restriction -- and whole cycles (2 x apply, then sample(5, qoi), then the state) equal
    Oracle.stencil's MULTICOLOUR replay, compared as uint64 (signed zeros count).  The oracle forms its own levels
    by SpGEMM; tests/test_user_stencil_host.py pins them, and that exchanging any two coefficients changes the
    oracle's cycle;
  * independent of the oracle: A x and R (f - A x) on every level of the C27 and C5 cases against the level's CSR
    product in np.longdouble, within the derived bound of user_stencils.highprec_ratios.

Crossings, cycles only: the generic kernels (every MGMC_DISABLE token), MGMC_DISABLE=fold, two batched chains,
poisoned LDS."""
import functools

import numpy as np
import pytest

import multigridmc_amd as mg
from tests import oracle_lib as O
from tests import user_stencils as US
from tests.test_gpu_parity import ALL_PATHS

pytestmark = pytest.mark.gpu

SEED = 5418513
COARSE = "k_coarse_ssor_lds (or separate colour passes)"
ZSWEEP = {"sweep^": "k_zsweep_rb7<", "post_sweep^": "k_zsweep_rb7<", "residual_restrict": "k_zresrestrict<7,64,4>"}


def _lv(sweep, residual_restrict=None, quads=None, noise=None):
    return {"sweep": sweep, "residual_restrict": residual_restrict, "quads": quads, "noise": noise, "post_sweep": None}


Q3, Q2, T3, T2, P3 = "k_sweep_quads<3>", "k_sweep_quads<2>", "k_tail<3>", "k_tail<2>", "k_sweep_pairs<3>"
QR = "k_quads_restrict2d"
Z27, Z27S, Z7 = "k_zresrestrict<27,64,4>", "k_zresrestrict<27,16,4>", "k_zresrestrict<7,64,4>"
# per case: (labels per level, fold flag per level).  A None value asserts the key's absence, "key^" a prefix.
EXPECT = {
    # 12-pair window quads on a 27-point fine level, the small restriction onto 11 columns, an odd-extent tail
    "c27_24x20x12": ([_lv(Q3, Z27S, "window"), _lv(T3), _lv(T3)], [0, 0, 0]),
    # window quads of 48 / 24 pairs, restriction- and tail-drawn noise
    "c27_96x48x48": ([_lv(Q3, Z27, "window"), _lv(Q3, Z27S, "window", "restriction+tail"), _lv(T3), _lv(T3)], [0] * 4),
    # lane-shift quads and a tail at a power-of-two shape without SYM
    "c27_64": ([_lv(Q3, Z27), _lv(Q3, Z27S, None, "restriction+tail"), _lv(T3), _lv(T3), _lv(T3)], [0] * 5),
    # colour-pair passes of 160 and 80 pairs
    "c27_320x24x16": ([_lv(P3, Z27), _lv(P3, Z27), _lv(COARSE)], [0] * 3),
    # j-marching half-sweeps of 256 and 128 pairs, both directions
    "c27_512x24x20_ssor": ([_lv("k_jsweep_half<256>", Z27), _lv("k_jsweep_half<128>", Z27), _lv(COARSE)], [0] * 3),
    # 7 distinct coefficients: not FD-symmetric, so the colour passes and not the z-sweep; 27-point coarse SSOR in LDS
    "c7_64x44x40": ([_lv("k_sweep_rb<3>", Z7), _lv(COARSE)], [0, 0]),
    # the z-sweep folding an anisotropic stencil, plain and fused-prolongation instances
    "s7_192x48x40": ([ZSWEEP, _lv(COARSE)], [0, 1]),
    "s7_128x36x24_ssor": ([ZSWEEP, _lv(COARSE)], [0, 1]),
    # z-sweep, the SYM j-marching instance, fold27 in the tuned restriction tile with partial y / z tiles, quads
    "s7_512x24x24": ([ZSWEEP, _lv("k_jsweep_half<128,sym>", Z27), _lv(Q3, Z27, None, "restriction"), _lv(COARSE)],
                     [0, 1, 1, 1]),
    # SYM / fold with window quads, 80-pair colour pairs, odd tails, partial restriction tiles
    "s27_96x48x48": ([_lv(Q3, Z27, "window"), _lv(Q3, Z27S, "window", "restriction+tail"), _lv(T3), _lv(T3)], [1] * 4),
    "s27_80x48x40_ssor_W": ([_lv(Q3, Z27, "window"), _lv(Q3, Z27S, "window", "restriction"), _lv(COARSE)], [1] * 3),
    "s27_24x20x12": ([_lv(Q3, Z27S, "window"), _lv(T3), _lv(T3)], [1] * 3),
    "s27_320x24x16": ([_lv(P3, Z27), _lv(P3, Z27), _lv(COARSE)], [1] * 3),
    # dense coarse factors of a user stencil
    "p27_32_chol": ([_lv(Q3, Z27S), _lv(Q3, Z27S), _lv("k_coarse_chol")], [0] * 3),
    # k_rb2d with a(-x) != a(+x), the fused 2D last pre-sweep + restriction, a 2D tail
    "c5_200x120": ([_lv("k_rb2d", "k_residual_restrict<2,5>"),
                    _lv(Q2 + " (last pre-sweep: k_quads_restrict2d)", QR), _lv(T2), _lv(T2)], [0] * 4),
    # a 9-point fine level in the quad passes
    "c9_256x128_ssor_W": ([_lv(Q2, "k_residual_restrict<2,9>"),
                           _lv(Q2 + " (last pre-sweep: k_quads_restrict2d)", QR), _lv(COARSE)], [0] * 3),
    "c9_100x60": ([_lv(Q2, "k_residual_restrict<2,9>"), _lv(T2), _lv(T2)], [0] * 3),
}
assert set(EXPECT) == set(US.CASES)


def same(a, b):
    """Bit for bit: float64 arrays compared as uint64, so +0.0 and -0.0 differ."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


@functools.lru_cache(maxsize=2)
def assembled(sname, shape):
    """The fixture's truncated CSR on the lattice, built once per module for consecutive uses."""
    return US.csr(shape, US.STENCILS[sname]())


def params_of(name):
    return mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **US.CASES[name][2]})


def device(name, chain=0, nchains=1):
    sname, shape, _ = US.CASES[name]
    lat = mg.Lattice(*shape)
    s = mg.MultigridMCSampler(mg.SparseMatrixOperator(lat, assembled(sname, shape)), SEED, params_of(name), device=0,
                              chain_id=chain, nchains=nchains)
    assert s.level_desc(0)["varcoef"] == 0  # the stencil path, not the matrix path
    return s, lat


def oracle(name, chain=0):
    sname, shape, _ = US.CASES[name]
    return O.Oracle.stencil(shape, params_of(name), US.STENCILS[sname](), mode=O.MULTICOLOUR, seed=SEED, chain=chain)


@pytest.fixture(scope="module", autouse=True)
def oracle_threads():
    O.set_threads(O.cpu_share())
    yield
    O.set_threads(1)


@pytest.fixture(scope="module", params=list(US.CASES))
def case(request, hip_device):
    """(name, device handle, oracle) of one case, shared by the tests below (pytest runs them case by case)."""
    name = request.param
    s, lat = device(name)
    mc = oracle(name)
    yield name, s, mc
    s.close()


def test_labels_and_fold_flags(case):
    name, s, mc = case
    labels, folds = EXPECT[name]
    p = params_of(name)
    assert len(labels) == p.nlevel
    for level, want in enumerate(labels):
        k = s.level_kernels(level)
        for key, value in want.items():
            if key.endswith("^"):
                assert k[key[:-1]].startswith(value), (name, level, k)
            else:
                assert k.get(key) == value, (name, level, key, k)
        desc = s.level_desc(level)
        assert desc["ndof"] == mc.ndof(level)
        assert O.fold_level(desc) == bool(folds[level]), (name, level)


def test_components_bitwise(case):
    name, s, mc = case
    p = params_of(name)
    rng = np.random.default_rng(42)
    for level in range(p.nlevel):
        n = s.level_desc(level)["ndof"]
        x, f = rng.standard_normal(n), rng.standard_normal(n)
        assert same(s.operator_apply(level, x), mc.operator_apply(level, x)), (level, "operator")
        for direction in (mg.FORWARD, mg.BACKWARD):
            assert same(s.smoother_apply(level, direction, 2, f, x), mc.smoother_apply(level, direction, 2, f, x)), \
                (level, direction, "smoother")
            assert same(s.sor_sampler_apply(level, direction, 5 + level, 77, f, x),
                        mc.sor_sampler_apply(level, direction, 5 + level, 77, f, x)), (level, direction, "sampler")
        if level + 1 < p.nlevel:
            xc = rng.standard_normal(s.level_desc(level + 1)["ndof"])
            assert same(s.residual_restrict(level, f, x), mc.residual_restrict(level, f, x)), (level, "residual")
            assert same(s.restrict(level, f), mc.restrict(level, f)), (level, "restrict")
            assert same(s.prolongate_add(level, 1.3, xc, x), mc.prolongate_add(level, 1.3, xc, x)), (level, "prolong")


def _cycles_equal(s, mc, lat, f, chain=None):
    """The cycle body of test_gpu_parity.test_mgmc_cycles_bitwise: 2 x apply, then the device-resident loop with
    its QoI series, then the state."""
    n = lat.Nvertex
    x_dev, x_orc = np.zeros(n), np.zeros(n)
    mc.set_sample_index(0)
    for _ in range(2):
        s.apply(f, x_dev)
        mc.apply(f, x_orc)
        assert np.all(np.isfinite(x_orc)) and same(x_dev, x_orc)
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    s.fix_rhs(f)
    s.set_state(x_dev)
    mc.set_rhs(f)
    mc.set_state(x_orc)
    assert same(s.sample(5, qoi), mc.sample(5, qoi))
    assert same(s.get_state(), mc.get_state())
    assert s.get_sample_index() == 7


def test_cycles_bitwise(case):
    name, _, mc = case
    s, lat = device(name)  # a handle of its own: the cycle counts its samples from 0
    _cycles_equal(s, mc, lat, np.random.default_rng(11).standard_normal(lat.Nvertex))
    s.close()


@pytest.mark.parametrize("name", ["s7_192x48x40", "s7_128x36x24_ssor"])
def test_cycles_bitwise_zero_rhs(hip_device, name):
    """f = 0 on the z-sweep levels: the sweeps and the residual + restriction take the right-hand side as a
    constant (rhs=zero) and must still fold the anisotropic stencil as the oracle does."""
    s, lat = device(name)
    _cycles_equal(s, oracle(name), lat, np.zeros(lat.Nvertex))
    assert s.level_kernels(0).get("rhs") == "zero"
    s.close()


@pytest.mark.parametrize("name", US.HIGHPREC)
def test_against_longdouble(hip_device, name):
    """Independent of the oracle: A x and R (f - A x) on every level against the level's CSR -- the level's
    stencil truncated on its lattice -- in np.longdouble, within the bound derived in
    user_stencils.highprec_ratios.  (The oracle alone: <= 0.54 and <= 0.34 of the bound on the same inputs,
    tests/test_user_stencil_host.py.)"""
    s, _ = device(name)
    p = params_of(name)
    dim = len(US.CASES[name][1])
    rng = np.random.default_rng(19)
    worst = [0.0, 0.0]
    for level in range(p.nlevel):
        desc = s.level_desc(level)
        x, f = rng.standard_normal(desc["ndof"]), rng.standard_normal(desc["ndof"])
        fc = s.residual_restrict(level, f, x) if level + 1 < p.nlevel else None
        r = US.highprec_ratios(desc["shape"], desc["stencil"][:3 ** dim], x, f, s.operator_apply(level, x), fc)
        worst = [max(worst[0], r[0]), max(worst[1], r[1] or 0.0)]
    s.close()
    print(f"{name}: max |error| / bound: operator {worst[0]:.3f}, residual + restriction {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0


# ---- crossings: one case each, cycles only ----

@pytest.mark.parametrize("name,paths", [("c27_64", ALL_PATHS), ("c5_200x120", ALL_PATHS), ("s27_96x48x48", "fold")])
def test_variant_cycles_bitwise(hip_device, monkeypatch, name, paths):
    """MGMC_DISABLE = every token: the generic colour passes and per-point kernels read the same coefficients;
    MGMC_DISABLE=fold: S27's residuals in the reference's CSR order, the oracle with set_no_fold."""
    monkeypatch.setenv("MGMC_DISABLE", paths)
    s, lat = device(name)
    O.set_no_fold("fold" in paths.split(","))
    try:
        mc = oracle(name)
    finally:
        O.set_no_fold(False)
    if paths == ALL_PATHS:
        assert not any(s.level_kernels(l)["sweep"].startswith(("k_tail", "k_sweep_quads", "k_rb2d", "k_sweep_pairs"))
                       for l in range(params_of(name).nlevel))
    _cycles_equal(s, mc, lat, np.random.default_rng(7).standard_normal(lat.Nvertex))
    s.close()


def test_batched_chains_bitwise(hip_device):
    """Two chains in one handle against two one-chain handles and the oracle's chains."""
    name, chain0 = "c27_96x48x48", 11
    b, lat = device(name, chain=chain0, nchains=2)
    rng = np.random.default_rng(17)
    f, x0 = rng.standard_normal(lat.Nvertex), 0.1 * rng.standard_normal(lat.Nvertex)
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    b.fix_rhs(f)
    b.set_state(x0)
    zb = b.sample(5, qoi, chain=None)
    assert not same(zb[0], zb[1])
    for c in range(2):
        s, _ = device(name, chain=chain0 + c)
        mc = oracle(name, chain=chain0 + c)
        s.fix_rhs(f)
        s.set_state(x0)
        mc.set_rhs(f)
        mc.set_state(x0)
        z = mc.sample(5, qoi)
        assert same(s.sample(5, qoi), z) and same(zb[c], z), c
        assert same(s.get_state(), mc.get_state()) and same(b.get_state(c), mc.get_state()), c
        s.close()
    b.close()


def test_poisoned_lds_cycles_bitwise(hip_device, monkeypatch):
    """MGMC_POISON=1 (NaN-filled LDS before every op of the cycle): the j-marching half-sweeps with all
    coefficients distinct read no LDS slot they did not write."""
    monkeypatch.setenv("MGMC_POISON", "1")
    name = "c27_512x24x20_ssor"
    s, lat = device(name)
    _cycles_equal(s, oracle(name), lat, np.random.default_rng(11).standard_normal(lat.Nvertex))
    s.close()
