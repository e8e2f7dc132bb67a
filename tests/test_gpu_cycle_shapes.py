"""Cycle shape as part of the parity contract (-m gpu): whole cycles against the CPU oracle, bit for bit, where
the host-side op list (mgmc_capi.hip: build_ops_level, push_sweep, build_tails_only, fuse_sweep_restrict,
mark_zero_inputs, mark_rhs_zero, plan_drawn_noise) takes branches the shapes of tests/test_gpu_parity.py do not:

  * npresmooth = 0 / npostsmooth = 0: a restriction followed directly by the next restriction (no pre-sweep to
    take the known-zero x or the restriction-drawn noise), a prolongation that is an op of its own, a W-cycle's
    later visit whose first sweep after a tail is a pre-sweep, empty timed segments;
  * an odd number of out-of-place sweeps on Galerkin levels (SOR 2/1, 1/2, 3/0): OP_COPY on k_sweep_quads and
    k_jsweep_half levels;
  * hierarchies coarsened to 2^d cells: by LDS size their tails would be five and six levels deep, TailArgs holds
    TAIL_MAX_LEVELS = 4 (mgmc_level_plan.hpp tail_start: the tail starts later);
  * tail runs above TAIL_MAX_OPS = 96 ops (183, 120): the tail starts a level later, where a whole run fits.

Every case: FD prior, kappa^2 = 25, seed 5418513, chain 0, SOR smoother and SSOR coarse sampler unless stated; the
oracle builds its own hierarchy (Oracle.fd_own, MULTICOLOUR).  Two apply() cycles from x = 0 with a random f, then
fix_rhs / set_state and a 6-sample QoI series at the lattice centre; np.array_equal on the state after each apply,
on the series and on the final state; get_sample_index() == 8.  The oracle's results are computed once per case and
shared by the variant, poison and batch tests.  tests/test_level_plan_host.py pins the limits on the CPU."""
import numpy as np
import pytest

import multigridmc_amd as mg
from tests import oracle_lib as O
from tests.test_gpu_parity import ALL_PATHS

pytestmark = pytest.mark.gpu

SEED = 5418513
KAPPA_SQ = 25.0
COARSE_LDS = "k_coarse_ssor_lds (or separate colour passes)"


def _kw(npre, npost, **extra):
    return dict(npresmooth=npre, npostsmooth=npost, **extra)


# ---- the groups: shape, nlevel, {level: {label key: value}} (a "sweep^" key asserts a prefix, None an absence) ----
GROUPS = {
    # z-sweep fine level with fused prolongation, lane-shift quads on 32^3, tail of 16^3 / 8^3 / 4^3
    "z64": ((64, 64, 64), 5, {0: {"sweep^": "k_zsweep_rb7<"}, 1: {"sweep": "k_sweep_quads<3>", "quads": None},
                              2: {"sweep": "k_tail<3>"}, 3: {"sweep": "k_tail<3>"}, 4: {"sweep": "k_tail<3>"}}),
    # k_jsweep_half<128> on level 1, 64-pair quads on level 2, no tail
    "j512": ((512, 24, 24), 4, {0: {"sweep^": "k_zsweep_rb7<"}, 1: {"sweep^": "k_jsweep_half<128"},
                                2: {"sweep": "k_sweep_quads<3>", "quads": None}, 3: {"sweep": COARSE_LDS}}),
    # in-place k_sweep_rb fine level, 24-pair window quads, tail of 24 x 12 x 12 / 12 x 6 x 6
    "c96": ((96, 48, 48), 4, {0: {"sweep": "k_sweep_rb<3>"}, 1: {"sweep": "k_sweep_quads<3>", "quads": "window"},
                              2: {"sweep": "k_tail<3>"}, 3: {"sweep": "k_tail<3>"}}),
    # no tail, quads on two levels, coarse LDS sampler
    "q128": ((128, 64, 64), 4, {0: {"sweep^": "k_zsweep_rb7<"}, 1: {"sweep": "k_sweep_quads<3>"},
                                2: {"sweep": "k_sweep_quads<3>"}, 3: {"sweep": COARSE_LDS}}),
    # k_rb2d, one k_quads_restrict2d level, tail
    "r256": ((256, 128), 4, {0: {"sweep": "k_rb2d"}, 1: {"residual_restrict": "k_quads_restrict2d"},
                             2: {"sweep": "k_tail<2>"}, 3: {"sweep": "k_tail<2>"}}),
    # two k_quads_restrict2d levels; the fused restriction onto the coarsest draws the coarse sampler's noise
    "r512": ((512, 512), 4, {0: {"sweep": "k_rb2d"}, 1: {"residual_restrict": "k_quads_restrict2d"},
                             2: {"residual_restrict": "k_quads_restrict2d"}, 3: {"sweep": COARSE_LDS}}),
}
SSOR_02 = _kw(0, 2, smoother="SSOR", omega=1.1, coarse_scaling=0.9)
SWEEP_COUNTS = {
    "z64": [_kw(0, 1), _kw(1, 0), _kw(0, 0), _kw(2, 1), _kw(1, 2), _kw(3, 0), _kw(0, 1, cycle=2), _kw(1, 0, cycle=2),
            _kw(2, 1, smoother="SSOR"), SSOR_02],
    "j512": [_kw(0, 1), _kw(1, 0), _kw(2, 1), _kw(1, 2, smoother="SSOR")],
    "c96": [_kw(0, 1), _kw(2, 1), _kw(1, 0, cycle=2)],
    "q128": [_kw(2, 1), _kw(0, 1)],
    "r256": [_kw(0, 1), _kw(1, 0), _kw(2, 1), _kw(2, 1, cycle=2), _kw(1, 2, smoother="SSOR")],
    "r512": [_kw(0, 1), _kw(2, 1)],
}


def _name(group, kw):
    s = f"{group}_{kw['npresmooth']}_{kw['npostsmooth']}"
    if kw.get("cycle", 1) != 1:
        s += f"_cycle{kw['cycle']}"
    if kw.get("smoother") == "SSOR":
        s += "_ssor"
    return s


def _tail(dim, first, nlevel):
    return {level: {"sweep": f"k_tail<{dim}>"} for level in range(first, nlevel)}


# name: (shape, MultigridParameters keywords, labels)
CASES = {}
for _g, _list in SWEEP_COUNTS.items():
    for _k in _list:
        CASES[_name(_g, _k)] = (GROUPS[_g][0], dict(nlevel=GROUPS[_g][1], **_k), GROUPS[_g][2])
SWEEP_COUNT_CASES = list(CASES)

QR = {"residual_restrict": "k_quads_restrict2d"}
DEEP = {
    # coarsened to 2^d cells: the tail holds the last TAIL_MAX_LEVELS = 4 levels, the levels before it run their
    # own kernels (by LDS size the 2D tails would start at level 1)
    "deep_2d64_6lvl": ((64, 64), dict(nlevel=6), {0: {"sweep": "k_rb2d"}, 1: QR, **_tail(2, 2, 6)}),
    "deep_2d64_6lvl_cycle2": ((64, 64), dict(nlevel=6, cycle=2), {1: QR, **_tail(2, 2, 6)}),
    "deep_2d64_6lvl_ssor": ((64, 64), dict(nlevel=6, smoother="SSOR"), {1: QR, **_tail(2, 2, 6)}),
    "deep_2d96x64_6lvl": ((96, 64), dict(nlevel=6), {1: QR, **_tail(2, 2, 6)}),  # coarsest 3 x 2
    "deep_2d128_7lvl": ((128, 128), dict(nlevel=7), {1: QR, 2: QR, **_tail(2, 3, 7)}),
    "deep_3d32_5lvl": ((32, 32, 32), dict(nlevel=5), {0: {"sweep": "k_sweep_rb<3>"}, **_tail(3, 1, 5)}),  # coarsest 2^3
    "deep_3d64_6lvl": ((64, 64, 64), dict(nlevel=6), {1: {"sweep": "k_sweep_quads<3>"}, **_tail(3, 2, 6)}),
    # one coarse unknown, and a fine level smaller than any tile
    "deep_2d4_2lvl": ((4, 4), dict(nlevel=2), {0: {"sweep": "k_rb2d"}, 1: {"sweep": COARSE_LDS}}),
    "deep_3d4_2lvl": ((4, 4, 4), dict(nlevel=2), {0: {"sweep": "k_sweep_rb<3>"}, 1: {"sweep": COARSE_LDS}}),
}
CASES.update(DEEP)

Q3 = {"sweep": "k_sweep_quads<3>"}
LONG = {
    # a run of levels 1-4 would be 183 / 183 / 120 ops (tail_run_ops): the tail starts at level 2 (57 / 57 / 52
    # ops) and level 1 runs its own kernels, not k_tail
    "long_3d32_cycle3": ((32, 32, 32), dict(nlevel=5, cycle=3), {1: Q3, **_tail(3, 2, 5)}),
    "long_2d64_cycle3": ((64, 64), dict(nlevel=5, cycle=3), {1: QR, **_tail(2, 2, 5)}),
    "long_3d32_ssor_2_1_W": ((32, 32, 32), dict(nlevel=5, cycle=2, smoother="SSOR", npresmooth=2),
                             {1: Q3, **_tail(3, 2, 5)}),
    # control: 92 ops stay in one k_tail launch from level 1
    "long_3d32_ssor_W_control": ((32, 32, 32), dict(nlevel=5, cycle=2, smoother="SSOR"), _tail(3, 1, 5)),
}
CASES.update(LONG)


def params(name):
    return mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **CASES[name][1]})


def make(name, chain=0, nchains=1):
    """The device handle of a case (MGMC_DISABLE / MGMC_POISON are read from the environment at creation)."""
    lat = mg.Lattice(*CASES[name][0])
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, KAPPA_SQ), SEED, params(name), device=0, chain_id=chain,
                              nchains=nchains)
    return s, lat


def rhs(lat):
    return np.random.default_rng(11).standard_normal(lat.Nvertex)


def protocol(h, lat):
    """Two apply() cycles from x = 0, then the device-resident (oracle: host) loop of 6 samples from that state:
    (state after apply 1, state after apply 2, QoI series, final state)."""
    f = rhs(lat)
    x = np.zeros(lat.Nvertex)
    h.apply(f, x)
    x1 = x.copy()
    h.apply(f, x)
    x2 = x.copy()
    h.set_rhs(f) if isinstance(h, O.Oracle) else h.fix_rhs(f)
    h.set_state(x2)
    z = h.sample(6, mg.measurement_vector_index(lat, [0.5] * lat.dim))
    return x1, x2, np.array(z), h.get_state()


_ORACLE = {}


def expected(name, no_fold=False):
    """The oracle's protocol results, computed once per (case, fold setting) and never modified."""
    key = (name, bool(no_fold))
    if key not in _ORACLE:
        lat = mg.Lattice(*CASES[name][0])
        O.set_no_fold(bool(no_fold))
        try:
            mc = O.Oracle.fd_own(lat.shape, params(name), KAPPA_SQ, mode=O.MULTICOLOUR, seed=SEED, chain=0)
        finally:
            O.set_no_fold(False)
        out = protocol(mc, lat)
        for a in out:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def assert_labels(s, labels, name):
    for level, want in labels.items():
        got = s.level_kernels(level)
        for key, value in want.items():
            if key.endswith("^"):
                assert got[key[:-1]].startswith(value), (name, level, got)
            else:
                assert got.get(key) == value, (name, level, got)


def assert_protocol(name, got, want, what=""):
    for part, g, w in zip(("apply 1", "apply 2", "QoI series", "final state"), got, want):
        assert np.all(np.isfinite(g)), f"{name}{what}: {part} not finite"
        assert np.array_equal(g, w), f"{name}{what}: {part} differs from the oracle " \
                                     f"({int(np.sum(g != w))} of {g.size} entries, max |d| {np.max(np.abs(g - w)):.3e})"


def check_case(name, no_fold=False, what=""):
    s, lat = make(name)
    try:
        print(name + what, *(";".join(f"{k}={v}" for k, v in s.level_kernels(level).items())
                             for level in range(params(name).nlevel)), sep="\n  ")
        if not what:
            assert_labels(s, CASES[name][2], name)
        assert_protocol(name, protocol(s, lat), expected(name, no_fold), what)
        assert s.get_sample_index() == 8
    finally:
        s.close()


@pytest.mark.parametrize("name", SWEEP_COUNT_CASES)
def test_sweep_count_cycles_bitwise(hip_device, name):
    """Zero and odd sweep counts on every kernel family's levels (the module docstring's first two items)."""
    check_case(name)


@pytest.mark.parametrize("name", list(DEEP))
def test_deep_hierarchy_cycles_bitwise(hip_device, name):
    """Hierarchies coarsened to 2^d cells (and 4^d fine levels with one coarse unknown): the tail holds at most
    four levels, asserted through the labels."""
    check_case(name)


@pytest.mark.parametrize("name", list(LONG))
def test_long_tail_run_cycles_bitwise(hip_device, name):
    """Runs above TAIL_MAX_OPS ops leave level 1 to its own kernels (it does not claim k_tail) and run levels 2-4
    as one whole run per k_tail launch; the 92-op control keeps levels 1-4 in k_tail."""
    check_case(name)


# ---- what the sweeps of (64,64,64) nlevel=5 level 1 read (plan_drawn_noise) ----

def _noise(name):
    s, _ = make(name)
    try:
        return s.level_kernels(1).get("noise", "")
    finally:
        s.close()


def test_drawn_noise_labels_without_pre_or_post_sweeps(hip_device):
    """Level 1 (32^3 quad passes, a 7-point restriction above it, the tail below): with no pre-sweep nothing reads
    restriction-drawn noise, and in a V-cycle with no post-sweep nothing reads tail-drawn noise.  The W-cycle with
    no post-sweep is printed: its later visit's pre-sweep follows a tail (whether reading the tail's draws there
    is right is the oracle's verdict, test_sweep_count_cycles_bitwise[z64_1_0_cycle2])."""
    for name in ("z64_0_1", "z64_0_0", "z64_0_1_cycle2", "z64_0_2_ssor"):
        assert "restriction" not in _noise(name), name
    for name in ("z64_1_0", "z64_3_0", "z64_0_0"):
        assert "tail" not in _noise(name), name
    print("z64_1_0_cycle2 level 1 noise:", repr(_noise("z64_1_0_cycle2")))


# ---- cross-checks: one z-sweep, one j-sweep, one 2D, one deep-tail and one over-long case ----
SUBSET = ["z64_0_1", "j512_2_1", "r256_2_1_cycle2", "deep_2d64_6lvl", "long_3d32_cycle3"]
DISABLE = [ALL_PATHS, "xzero", "post_noise", "tail", "fuse_prolong"]


@pytest.mark.parametrize("name", SUBSET)
@pytest.mark.parametrize("paths", DISABLE)
def test_cycle_shape_variants_bitwise(hip_device, monkeypatch, paths, name):
    """The same protocol with fast paths turned off (test_gpu_parity.test_variant_cycles_bitwise): the fallbacks'
    op lists (no tail, separate prolongation, restriction-zeroed x, sweeps drawing their own noise) equal the
    oracle too."""
    monkeypatch.setenv("MGMC_DISABLE", paths)
    check_case(name, no_fold="fold" in paths.split(","), what=f" [MGMC_DISABLE={paths}]")


@pytest.mark.parametrize("name", SUBSET)
def test_cycle_shape_poisoned_bitwise(hip_device, monkeypatch, name):
    """MGMC_POISON=1 (tests/test_gpu_poison.py): NaN-filled allocations and LDS, the known-zero x of a coarse
    level poisoned where its write is skipped.  Series and states equal the unpoisoned handle's: no OP_COPY and no
    zero-taken input reads a buffer nobody wrote."""
    plain, lat = make(name)
    want = protocol(plain, lat)
    plain.close()
    monkeypatch.setenv("MGMC_POISON", "1")
    s, _ = make(name)
    got = protocol(s, lat)
    s.close()
    assert_protocol(name, got, want, " [MGMC_POISON=1 against the unpoisoned handle]")
    assert_protocol(name, got, expected(name), " [MGMC_POISON=1]")


@pytest.mark.parametrize("name", ["deep_2d64_6lvl", "z64_0_1", "long_3d32_cycle3"])
def test_cycle_shape_two_chains_equal_one_chain_handles(hip_device, name):
    """nchains = 2 (one workgroup per chain in k_tail, no tail- or restriction-drawn noise) against two one-chain
    handles with chain ids 0 and 1."""
    b, lat = make(name, nchains=2)
    f = rhs(lat)
    x0 = 0.1 * np.random.default_rng(17).standard_normal(lat.Nvertex)
    q = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    b.fix_rhs(f)
    b.set_state(x0)
    zb = b.sample(4, q, chain=None)
    states = [b.get_state(c) for c in range(2)]
    b.close()
    for c in range(2):
        s, _ = make(name, chain=c)
        s.fix_rhs(f)
        s.set_state(x0)
        z = s.sample(4, q)
        assert np.all(np.isfinite(z))
        assert np.array_equal(zb[c], z), f"{name} chain {c}: QoI series"
        assert np.array_equal(states[c], s.get_state()), f"{name} chain {c}: state"
        s.close()
    assert not np.array_equal(zb[0], zb[1])


@pytest.mark.parametrize("name,empty", [("z64_0_1", "npre"), ("z64_1_0", "npost")])
def test_sample_timed_with_an_empty_fine_segment(hip_device, name, empty):
    """mgmc_sample_timed with no fine pre-sweeps (no fine post-sweeps): the empty segment counts 0 sweeps, every
    segment time is finite and non-negative, and the chain is the plain loop's bit for bit -- or the call refuses
    with an MgmcError that says so; never a NaN time or another chain."""
    s, lat = make(name)
    t, _ = make(name)
    q = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    try:
        r = s.sample_timed(4, q, stride=1)
    except mg.MgmcError as e:
        assert "timed" in str(e), str(e)
        s.close()
        t.close()
        return
    print(name, r)
    other = "npost" if empty == "npre" else "npre"
    assert r[empty] == 0 and r[other] == 4
    for key in ("pre_ms", "post_ms", "total_ms"):
        assert np.isfinite(r[key]) and r[key] >= 0.0, (key, r)
    assert r[empty[1:] + "_ms"] <= r["total_ms"] and r[other[1:] + "_ms"] > 0.0
    assert np.array_equal(s.get_series(4), t.sample(4, q))
    assert np.array_equal(s.get_state(), t.get_state())
    s.close()
    t.close()
