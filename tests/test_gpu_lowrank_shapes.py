"""The low-rank posterior path at its documented limits (-m gpu): m = 64, 16 chains, dense and multi-block columns.

The ABI takes 1 <= m <= 64 columns, any CSC B and up to 16 chains; the other posterior tests stay at m <= 9 and 4
chains, with at most one mask bit above bit 8 and one constant dense column.  The families of tests/lowrank_shapes.py
reach what that leaves out: the m <= 8 edge of lr_small_launch (mgmc_capi.hip: `if (lr.m <= 8)` takes
k_lr_small_pf<8, 2>, else the general k_lr_small -- no label tells them apart, P8 / P9 sit on either side), the
second round of the 16-wave column loops (k_lr_small, the tail's lr_dots: P17, m = 64), LDS tables sized by LR_MAX_M
and LR_MAX_CH full (ws, dt, lr_s: m = 64 with 16 chains), the tail's saved rows of B with 64 columns, rows of B with
mask bits 31 / 32 / 33 / 63 set together (OV64), entry lists over more than one LR_BLK block (BLK), a dense column
that is not one number (DV: dense path without split_g) and two dense columns (D2: the row lists over every vertex).

Every comparison is a uint64 view against the CPU oracle's MULTICOLOUR replay with the same B (fd_own, then
set_lowrank), never against a second device run except for the path-on / path-off states of the fallback test;
tests/test_lowrank_shapes_host.py holds that oracle to exact algebra at the same (lattice, family) pairs, and
test_device_sweeps_are_the_sor_splitting holds the device to it directly.  The `lowrank` label of every level is
asserted (level 0) or checked against the documented values and printed (below level 0) before anything runs.

The tail: on F2 (3 levels) the plan starts k_tail<2> at level 1 for every small family (a run of 6 ops, about 53 KB
of LDS with the saved rows), so no extra case with another ncoarsesmooth / cycle is needed; F3 and FZ have two
levels and no tail (a tail needs a level below its first).
"""
import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd import _native
from multigridmc_amd.measured import LowRankUpdate
from tests import algebra as AL
from tests import energy_ref as ER
from tests import lowrank_shapes as LS
from tests import oracle_lib as O
from tests import test_algebra_host as H

pytestmark = pytest.mark.gpu

SEED = 5418513
CHAIN0 = 11
DOCUMENTED = ("small", "rows", "dense", "dense,rhs_inplace")  # MultigridMCSampler.level_kernels
IDS = [f"{lat}-{fam}" for lat, fam in LS.PAIRS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def level0_label(lattice, family):
    if family in LS.SMALL_FAMILIES:
        return "small"
    if family == "DC64":
        return "dense,rhs_inplace" if lattice == "FZ" else "dense"
    return {"BLK": "rows", "DV": "dense", "D2": "rows"}[family]


def sampler(lattice, family, chain=0, nchains=1, **kw):
    shape, _ = LS.LATTICES[lattice]
    lat = mg.Lattice(*shape)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, LS.KAPPA_SQ), SEED, LS.params(lattice, **kw), device=0,
                              chain_id=chain, nchains=nchains)
    s.set_lowrank(LS.build(family, shape))
    return s, lat


def oracle(lattice, family, chain=0, **kw):
    shape, _ = LS.LATTICES[lattice]
    mc = O.Oracle.fd_own(shape, LS.params(lattice, **kw), LS.KAPPA_SQ, mode=O.MULTICOLOUR, seed=SEED, chain=chain)
    mc.set_lowrank(LS.build(family, shape))
    return mc


def assert_paths(s, lattice, family, level0=None):
    """The `lowrank` label of every level: level 0 as the family is there for, every level of a small family
    `small`, below level 0 one of the documented values; FZ: level 0 runs the z-sweep.  Prints the plan."""
    kernels = [s.level_kernels(level) for level in range(s.nlevel)]
    labels = [k.get("lowrank") for k in kernels]
    print(f"lowrank plan {lattice} {family}: lowrank {labels}  sweep {[k['sweep'] for k in kernels]}")
    assert labels[0] == (level0 or level0_label(lattice, family)), kernels[0]
    assert all(v in DOCUMENTED for v in labels), labels
    if family in LS.SMALL_FAMILIES and level0 is None:
        assert all(v == "small" for v in labels), labels
    if lattice == "FZ":
        assert kernels[0]["sweep"].startswith("k_zsweep_rb7<"), kernels[0]
    m = LS.build(family, LS.LATTICES[lattice][0]).m
    for level in range(s.nlevel):
        for direction in (mg.FORWARD, mg.BACKWARD):
            mm, rows = s.lowrank_info(level, direction)
            assert mm == m and rows > 0, (level, direction, mm, rows)
    return kernels


def check_components(s, mc):
    """test_gpu_lowrank.test_lowrank_components_bitwise's body."""
    rng = np.random.default_rng(3)
    for level in range(s.nlevel):
        n = s.level_desc(level)["ndof"]
        x = rng.standard_normal(n)
        b = rng.standard_normal(n)
        assert same_bits(s.operator_apply(level, x), mc.operator_apply(level, x)), f"level {level} apply"
        for direction in (mg.FORWARD, mg.BACKWARD):
            assert same_bits(s.smoother_apply(level, direction, 2, b, x),
                             mc.smoother_apply(level, direction, 2, b, x)), f"level {level} dir {direction} smoother"
            assert same_bits(s.sor_sampler_apply(level, direction, 9 + level, 31, b, x),
                             mc.sor_sampler_apply(level, direction, 9 + level, 31, b, x)), \
                f"level {level} dir {direction} sampler"
        if level + 1 < s.nlevel:
            assert same_bits(s.residual_restrict(level, b, x), mc.residual_restrict(level, b, x)), \
                f"level {level} residual"


def check_cycles(s, mc, lat, ncycles=3):
    """Two apply(f, x) with a random f, then sample(ncycles, qoi) from that state: states and the QoI series."""
    f = np.random.default_rng(11).standard_normal(lat.Nvertex)
    x_dev, x_orc = np.zeros(lat.Nvertex), np.zeros(lat.Nvertex)
    for q in range(2):
        s.apply(f, x_dev)
        mc.apply(f, x_orc)
        assert np.all(np.isfinite(x_dev)) and same_bits(x_dev, x_orc), f"apply {q}"
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    s.fix_rhs(f)
    s.set_state(x_dev)
    mc.set_rhs(f)
    mc.set_state(x_orc)
    assert same_bits(s.sample(ncycles, qoi), mc.sample(ncycles, qoi)), "QoI series"
    assert same_bits(s.get_state(), mc.get_state()), "state"


# ---- a, c: components ----

@pytest.mark.parametrize("lattice,family", LS.PAIRS, ids=IDS)
def test_components_bitwise(hip_device, lattice, family):
    """operator_apply, two noise-free sweeps and one noisy sweep per direction, residual + restriction, on every
    level with random vectors.  P8 / P9 / P17: see the module docstring for the dispatch line they straddle."""
    s, lat = sampler(lattice, family)
    assert_paths(s, lattice, family)
    if family == "OV64":  # overlapping balls reach more vertices than 64 points
        p64, _ = sampler(lattice, "P64")
        for direction in (mg.FORWARD, mg.BACKWARD):
            assert s.lowrank_info(0, direction)[1] > p64.lowrank_info(0, direction)[1]
        p64.close()
    check_components(s, oracle(lattice, family))
    s.close()


# ---- b, c: whole cycles ----

@pytest.mark.parametrize("lattice,family", LS.PAIRS, ids=IDS)
def test_cycles_bitwise(hip_device, lattice, family):
    """On F2 the small families run levels 1 and 2 in k_tail<2>: the tail with up to 64 columns, its dots in four
    rounds of 16 waves and its saved rows of B in LDS."""
    s, lat = sampler(lattice, family)
    kernels = assert_paths(s, lattice, family)
    if lattice == "F2" and family in LS.SMALL_FAMILIES:
        assert [k["sweep"] for k in kernels[1:]] == ["k_tail<2>", "k_tail<2>"], kernels
    check_cycles(s, oracle(lattice, family), lat)
    s.close()


# ---- d: chains at the maximum ----

@pytest.mark.parametrize("lattice,family,nchains", [("F2", "OV64", 16), ("F2", "DC64", 16), ("FZ", "DC64", 16),
                                                    ("F3", "P17", 5), ("F3", "BLK", 5), ("F3", "DV", 5)])
def test_batched_chains_bitwise(hip_device, lattice, family, nchains):
    """nchains chains with ids CHAIN0 .. in one handle, one f, a start state per chain: after 3 cycles chain c's QoI
    series, state and QoI moments are those of the oracle created with chain id CHAIN0 + c."""
    s, lat = sampler(lattice, family, chain=CHAIN0, nchains=nchains)
    assert_paths(s, lattice, family)
    rng = np.random.default_rng(17)
    f = rng.standard_normal(lat.Nvertex)
    x0 = 0.1 * rng.standard_normal((nchains, lat.Nvertex))
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    s.fix_rhs(f)
    for c in range(nchains):
        s.set_state(x0[c], chain=c)
    z = s.sample(3, qoi, chain=None)
    assert z.shape == (nchains, 3) and np.all(np.isfinite(z))
    for c in range(nchains):
        mc = oracle(lattice, family, chain=CHAIN0 + c)
        mc.set_rhs(f)
        mc.set_state(x0[c])
        zo = mc.sample(3, qoi)
        assert same_bits(z[c], zo), f"chain {c}: QoI series"
        assert same_bits(s.get_state(c), mc.get_state()), f"chain {c}: state"
        assert same_bits(s.qoi_moments(c), ER.welford(zo)), f"chain {c}: moments"
    assert not np.array_equal(z[0], z[nchains - 1])
    s.close()


# ---- e: fallback paths ----

FALLBACKS = ([("F2", fam, q) for fam in LS.SMALL_FAMILIES for q in ("lr_small", "lr_merge", "tail")] +
             [("F2", "DC64", "lr_dense"), ("FZ", "DC64", "lr_dense"), ("F2", "DV", "lr_dense")] +
             [("F2", fam, "lr_small,lr_merge,tail") for fam in ("BLK", "D2")])


@pytest.mark.parametrize("lattice,family,paths", FALLBACKS)
def test_fallback_paths_match(hip_device, lattice, family, paths, monkeypatch):
    """A low-rank kernel path switched off (MGMC_DISABLE, the values of test_gpu_lowrank.test_lowrank_paths_match):
    3 cycles against the oracle with the path off and with it on; the two device states are equal."""
    states = []
    for env in (paths, None):
        if env:
            monkeypatch.setenv("MGMC_DISABLE", env)
        else:
            monkeypatch.delenv("MGMC_DISABLE", raising=False)
        s, lat = sampler(lattice, family)
        if env == "lr_small" or env == "lr_dense":  # the row lists instead
            kernels = assert_paths(s, lattice, family, level0="rows")
        else:
            kernels = assert_paths(s, lattice, family)
        if env and "tail" in env.split(","):
            assert not any(k["sweep"].startswith("k_tail") for k in kernels), kernels
        mc = oracle(lattice, family)
        qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
        assert same_bits(s.sample(3, qoi), mc.sample(3, qoi))
        states.append(s.get_state())
        assert same_bits(states[-1], mc.get_state())
        s.close()
    assert same_bits(states[0], states[1])


# ---- f: poisoned LDS ----

@pytest.mark.parametrize("lattice,family", [("F2", "OV64"), ("FZ", "DC64")])
def test_poisoned_lds_sixteen_chains(hip_device, lattice, family, monkeypatch):
    """MGMC_POISON=1 (NaN into every compute unit's LDS before every op; tests/test_gpu_poison.py): ws, dt and lr_s
    are written for nchains * m words only, so a read beyond them -- or before the barrier -- computes with NaN.
    One apply and two cycles of 16 chains, every chain against its oracle."""
    monkeypatch.setenv("MGMC_POISON", "1")
    nchains = 16
    s, lat = sampler(lattice, family, chain=CHAIN0, nchains=nchains)
    assert_paths(s, lattice, family)
    rng = np.random.default_rng(19)
    f = rng.standard_normal(lat.Nvertex)
    x0 = rng.standard_normal(lat.Nvertex)
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    x = x0.copy()
    s.apply(f, x)  # every chain starts from x0
    s.fix_rhs(f)
    first = [s.get_state(c) for c in range(nchains)]
    z = s.sample(2, qoi, chain=None)
    for c in range(nchains):
        mc = oracle(lattice, family, chain=CHAIN0 + c)
        xo = x0.copy()
        mc.apply(f, xo)
        assert np.all(np.isfinite(first[c])) and same_bits(first[c], xo), f"chain {c}: apply"
        mc.set_rhs(f)
        mc.set_state(xo)
        assert same_bits(z[c], mc.sample(2, qoi)), f"chain {c}: QoI series"
        assert same_bits(s.get_state(c), mc.get_state()), f"chain {c}: state"
    assert same_bits(x, first[0])
    s.close()


# ---- g: validation ----

def test_sixty_five_columns_are_refused_and_change_nothing(hip_device):
    """m = 65 raises with a message that names m and leaves the handle as it was: lowrank_info unchanged and the
    next 2 cycles those of the B installed before (P17); m = 64 is accepted."""
    lattice = "F2"
    shape, _ = LS.LATTICES[lattice]
    s, lat = sampler(lattice, "P17")
    before = s.lowrank_info(0, mg.FORWARD)
    assert before[0] == 17
    p64 = LS.build("P64", shape)
    taken = set(int(v) for v in p64.rows)
    extra = next(v for v in range(lat.Nvertex) if v not in taken)
    cols = [(p64.rows[k:k + 1], p64.vals[k:k + 1]) for k in range(64)] + [(np.array([extra]), np.array([1.0]))]
    lr65 = LowRankUpdate.from_columns(lat.Nvertex, cols, np.append(p64.sigma, 1e-3))
    assert lr65.m == 65
    with pytest.raises(mg.MgmcError) as e:
        s.set_lowrank(lr65)
    assert e.value.code == _native.MGMC_E_INVALID
    assert "m_lowrank" in str(e.value) and "64" in str(e.value) and "m_lowrank" in _native.last_error(s.handle)
    assert s.lowrank_info(0, mg.FORWARD) == before
    mc = oracle(lattice, "P17")
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    assert same_bits(s.sample(2, qoi), mc.sample(2, qoi))
    assert same_bits(s.get_state(), mc.get_state())
    s.set_lowrank(p64)
    assert s.lowrank_info(0, mg.FORWARD)[0] == 64
    s.close()


# ---- h: the other readers of B ----

class Posterior:
    """What tests/energy_ref.py reads of an operator: the prior's matrix and the low-rank part."""

    def __init__(self, base, lr):
        self.base_operator, self.lr = base, lr

    def get_m_lowrank(self):
        return self.lr.m

    def get_B(self):
        return self.lr

    def get_ndof(self):
        return self.lr.n


@pytest.mark.parametrize("lattice,family", [("F2", "OV64"), ("F3", "D2")])
def test_conditional_precision_and_energy(hip_device, lattice, family):
    """field_conditional_precision() bit for bit against the contract of include/mgmc.h replayed in numpy (d_i =
    a_ii, then for k ascending with B_ik stored d_i = d_i + (B_ik * B_ik) / Sigma_k; a_ii from the FAITHFUL oracle's
    level-0 matrix), and energy()'s xqx, fx of a random state within the bound of tests/energy_ref.py, as
    tests/test_gpu_energy.py applies it."""
    shape, _ = LS.LATTICES[lattice]
    lr = LS.build(family, shape)
    s, lat = sampler(lattice, family)
    s.field_stats(1, conditional=True)
    d = s.field_conditional_precision()
    faithful = O.Oracle.fd(shape, LS.params(lattice), LS.KAPPA_SQ, mode=O.FAITHFUL)
    want = faithful.csr_matrix(0).diagonal().astype(np.float64)
    for k in range(lr.m):
        rows = lr.rows[lr.colptr[k]:lr.colptr[k + 1]]
        v = lr.vals[lr.colptr[k]:lr.colptr[k + 1]]
        want[rows] = want[rows] + (v * v) / lr.sigma[k]
    assert np.any(want != want[0]) and same_bits(d, want)
    s.field_stats_off()
    rng = np.random.default_rng(23)
    f, x = rng.standard_normal(lat.Nvertex), rng.standard_normal(lat.Nvertex)
    s.fix_rhs(f)
    s.set_state(x)
    xqx, fx = s.energy(chain=0)
    ref = ER.reference(Posterior(mg.ShiftedLaplaceFDOperator(lat, LS.KAPPA_SQ), lr), f, x)
    ok, rq, rf = ER.within_bound(xqx, fx, ref)
    print(f"energy ratio {lattice} {family}: xqx {rq:.1e} fx {rf:.1e} (relative bound {2 * ref[4] * ER.U:.2e})")
    assert ok, (xqx, fx, ref, rq, rf)
    assert ref[2] > 0 and xqx > 0
    s.close()


# ---- i: exact algebra on the device ----

@pytest.mark.parametrize("lattice,family", [("F2", "P64"), ("F2", "OV64"), ("F2", "DV"), ("F2", "D2"), ("FZ", "DC64")])
def test_device_sweeps_are_the_sor_splitting(hip_device, lattice, family):
    """Identities A and B of tests/algebra.py with the device as backend, bound C_TOL with the scale as
    tests/test_lowrank_shapes_host.py documents it: independent of the replay order, so a rule that the device and
    the oracle share and that is wrong would show here."""
    prob = LS.problem(lattice, family)
    s = prob.sampler(seed=H.SEED, chain=H.CHAIN)
    try:
        assert_paths(s, lattice, family)
        ratios = AL.check_sweeps(prob, s, s.normals, H.TAG, H.SAMPLE, np.random.default_rng(1))
        worst = AL.report(f"{lattice} {family} (device)", ratios)
        assert worst <= AL.C_TOL, ratios
    finally:
        s.close()
