"""Parity with every 64-bit RNG word in use (-m gpu): seed, chain id and sample index whose high halves are set.

Every normal is a pure function of a Philox key and counter (philox_normal.h):

    key     = (lo32(seed), lo32(chain) ^ hi32(seed))
    counter = (pair id, sweep tag, lo32(sample), hi32(sample))

The device assembles these words at every call site of philox4x32_10 / point_normal and rebuilds chain c's key of
a batched handle as (chain0 + c) ^ seed_hi at every chain-key site; the oracle does both once (refcpu.cpp).  The
other GPU modules run with a seed below 2^32, chain ids below 16 and sample indices below 100, where a site that
drops hi32(seed), passes lo32(sample) twice or leaves a struct's seed_hi zero gives the same bits as a correct one.
Here the same configurations, imported from those modules, run with

    SEED64  hi32 = 0x9E3779B9 and low bits set, so the xor changes the chain word's low bits
    CHAIN_H a batch of 4 reaches 2^32 - 2: high bits of lo32(chain), no wrap
    S_CARRY 6 cycles run at 2^32 - 3 ... 2^32 + 2: the low word carries into the high one mid-run, on the device
    S_HIGH  hi32(sample) != 0 from the first cycle, and another carry of the low word

  A  whole cycles of one chain against the oracle, one configuration per noise site (labels assert the reach);
     three single-word sets on the cheapest configurations make a failure name the word
  B  component sweeps (their own kernel choice) with the tag's top bit and a high sample word
  C  batched handles: chain c against the one-chain handle CHAIN_H + c (the chain-key sites), chain 0 against the
     oracle
  D  unrolled graphs and timed sampling across the carry, field statistics, the non-finite guard's 64-bit index
"""
import re

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd import _native
from tests import oracle_lib as O
from tests import test_gpu_batch as BAT
from tests import test_gpu_cholesky as CH
from tests import test_gpu_fem as FEM
from tests import test_gpu_field_stats as FS
from tests import test_gpu_lowrank as LR
from tests import test_gpu_parity as PAR
from tests import test_gpu_varcoef as VC

pytestmark = pytest.mark.gpu

SEED64 = 0x9E3779B97F4A7C15
CHAIN_H = 2 ** 32 - 5
S_CARRY = 2 ** 32 - 3
S_HIGH = 2 ** 40 + 2 ** 32 - 2
ALL = (SEED64, CHAIN_H, S_CARRY)
SINGLE = {"seed": (SEED64, 0, 0), "chain": (PAR.SEED, CHAIN_H, 0), "sample": (PAR.SEED, 0, S_HIGH)}

# the label of every coarsest SSOR level, whether k_coarse_ssor_lds runs it or -- when x and f do not fit LDS -- the
# level's colour passes do: asserted below only where the level fits (at most a few thousand unknowns)
COARSE_SSOR = "k_coarse_ssor_lds"
BLOCKED_SMALLEST = "2d_aniso_nl1"  # 15,105 unknowns: the smallest blocked case of test_gpu_cholesky.py
FIELD_SMALLEST = "2d_squared"  # 31^2 unknowns, three field levels
FEM_SMALLEST = "2d64_W"


def _build(family, name, words, lowrank=False):
    """(device handle, oracle, parameters, lattice) of a configuration of the module `family` names, with the
    seed and chain id of `words`."""
    seed, chain, _ = words
    if family == "fd":
        shape, kw = PAR.CONFIGS[name]
        s, p, lat = PAR.make(shape, chain=chain, seed=seed, **kw)
        return s, PAR.oracle_for(s, p, lat, chain=chain, seed=seed), p, lat
    if family == "chol":
        shape, kw = CH.CONFIGS[name]
        s, p, lat = CH._make(shape, kw, chain=chain, seed=seed)
        return s, CH._oracle(s, p, lat, chain=chain, seed=seed), p, lat
    if family == "lr":
        s, mc, p, lat, _ = LR.make(name, chain=chain, seed=seed)
        return s, mc, p, lat
    if family == "fem":
        return FEM.make(name, chain=chain, seed=seed)
    if family == "field":
        return VC.make(name, lowrank, chain=chain, seed=seed)
    raise KeyError(family)


def _build_with_paths(monkeypatch, family, name, words, paths):
    """_build under MGMC_DISABLE=paths, the oracle in the matching mode (test_variant_cycles_bitwise)."""
    if paths:
        monkeypatch.setenv("MGMC_DISABLE", paths)
    tokens = paths.split(",") if paths else []
    O.set_chol_blocked("chol_dense" in tokens)
    O.set_no_fold("fold" in tokens)
    try:
        return _build(family, name, words)
    finally:
        O.set_chol_blocked(False)
        O.set_no_fold(False)


def _check_labels(s, p, name, labels):
    """labels: [(level, {key: value})]; level -1 = the coarsest, "key^" a prefix, value None the key's absence,
    "any" in place of a level: some level carries them (ROW_LENGTH_LABELS' conventions)."""
    got = [s.level_kernels(level) for level in range(p.nlevel)]
    print(name, *(";".join(f"{k}={v}" for k, v in d.items()) for d in got), sep="\n  ")

    def holds(k, want):
        for key, value in want.items():
            if key.endswith("^"):
                if not k.get(key[:-1], "").startswith(value):
                    return False
            elif k.get(key) != value:
                return False
        return True

    for level, want in labels:
        if level == "any":
            assert any(holds(k, want) for k in got), (name, want, got)
        else:
            assert holds(got[level], want), (name, level, want, got)


def _welford(z):
    """k_qoi_record's moment update in float64 (mgmc_kernels.hpp), from an empty record"""
    n, mean, m2 = 0.0, 0.0, 0.0
    for v in z:
        cnt = n + 1.0
        delta = float(v) - mean
        new = mean + delta / cnt
        m2 = m2 + delta * (float(v) - new)
        mean, n = new, cnt
    return int(n), mean, m2


def _check_cycles(s, mc, lat, s0):
    """test_mgmc_cycles_bitwise's body from sample index s0: two apply, then sample(6, qoi); state, series, the
    sample index and the QoI moments bit for bit"""
    s.set_sample_index(s0)
    mc.set_sample_index(s0)
    rng = np.random.default_rng(11)
    f = rng.standard_normal(lat.Nvertex)
    x_dev = np.zeros(lat.Nvertex)
    x_orc = np.zeros(lat.Nvertex)
    for _ in range(2):
        s.apply(f, x_dev)
        mc.apply(f, x_orc)
        assert np.array_equal(x_dev, x_orc)
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    s.fix_rhs(f)
    s.set_state(x_dev)
    mc.set_rhs(f)
    mc.set_state(x_orc)
    z_dev = s.sample(6, qoi)
    z_orc = mc.sample(6, qoi)
    assert np.array_equal(z_dev, z_orc)
    assert np.array_equal(s.get_state(), mc.get_state())
    assert s.get_sample_index() == s0 + 8
    assert tuple(s.qoi_moments()) == _welford(z_orc)


ZS = [(0, {"sweep^": "k_zsweep_rb7<32,", "post_sweep^": "k_zsweep_rb7<32,"})]
JSWEEP_TAIL = [(1, {"sweep^": "k_jsweep_half<128"}), (2, {"sweep": "k_sweep_quads<3>", "noise": "restriction+tail"}),
               (3, {"sweep": "k_tail<3>"}), (0, {"noise": None}), (1, {"noise": None})]
QR = [(0, {"sweep": "k_rb2d"}), (1, {"residual_restrict": "k_quads_restrict2d"})]
LOWRANK = [(0, {"lowrank^": ""})]
# family, configuration, MGMC_DISABLE, labels: one row per noise site (the module docstring's section A)
CYCLES = [
    # k_zsweep_rb7 plain and fused-prolongation
    ("fd", "3d_zsr_edges", None, ZS),
    ("fd", "3d192_zsweep", None, ZS),
    # k_jsweep_half; restriction-drawn pre-sweep noise; post-sweep noise drawn by the tail launch's spare workgroups
    ("fd", "3d_jsweep_tail", None, JSWEEP_TAIL),
    # restriction-drawn pre-sweep noise of the window quad passes; the tail's noise drawn by the restriction launch's
    # spare workgroups (here and on 3d16, not on 3d_jsweep_tail)
    ("fd", "3d_192x48x48_5lvl", None, [(0, {"sweep^": "k_zsweep_rb7<"}), (1, {"quads": "window"}),
                                      (2, {"quads": "window", "noise": "restriction+tail"})]),
    ("fd", "3d_320x24x16", None, [(1, {"sweep": "k_sweep_pairs<3>", "quads": None})]),
    # k_sweep_quads forward and backward (SSOR)
    ("fd", "3d_80x48x40_ssor_W", None, [(1, {"sweep": "k_sweep_quads<3>", "quads": "window"})]),
    # k_rb2d, k_quads_restrict2d's own sweep; 2d_qr_aniso_ssor_W: its coarse level is the coarsest, whose SSOR
    # sampler's pairs the launch's spare workgroups draw
    ("fd", "2d_qr_aniso_ssor_W", None, QR + [(2, {"sweep^": COARSE_SSOR})]),
    ("fd", "2d_200x120_4lvl", None, QR + [(2, {"sweep": "k_tail<2>"})]),
    # k_coarse_ssor_lds, 2D and 3D: every item in registers; more than 4 x 1024 items (the second draw loop);
    # 2d256_global_coarse: a 127^2 coarsest level that does not fit LDS and runs the quad passes instead
    ("fd", "2d16_1lvl", None, [(0, {"sweep^": COARSE_SSOR})]),
    ("fd", "3d8_1lvl", None, [(0, {"sweep^": COARSE_SSOR})]),
    ("fd", "2d48_1lvl_items", None, [(0, {"sweep^": COARSE_SSOR})]),
    ("fd", "3d12_1lvl_items", None, [(0, {"sweep^": COARSE_SSOR})]),
    ("fd", "2d256_global_coarse", None, [(0, {"sweep": "k_rb2d"})]),
    # k_tail's own draws; every sweep's own draws instead of pre-drawn buffers
    ("fd", "3d16", "post_noise", [(0, {"sweep": "k_sweep_rb<3>"}), (1, {"sweep": "k_tail<3>"}), (2, {"sweep": "k_tail<3>"})]),
    ("fd", "3d_jsweep_tail", "post_noise", [(1, {"sweep^": "k_jsweep_half<128"}),
                                            (2, {"sweep": "k_sweep_quads<3>", "noise": None}), (3, {"sweep": "k_tail<3>"})]),
    # generic colour passes (point_normal)
    ("fd", "3d16", PAR.ALL_PATHS, [(0, {"sweep": "k_sweep_rb<3>"}), (1, {"sweep": "k_sweep_mc<3>"}),
                                   (2, {"sweep^": COARSE_SSOR})]),
    ("fd", "2d64_template_W", PAR.ALL_PATHS, [(0, {"sweep": "k_sweep_rb<2>"}), (1, {"sweep": "k_sweep_mc<2>"}),
                                              (2, {"sweep": "k_sweep_mc<2>"}), (3, {"sweep^": COARSE_SSOR})]),
    # dense and blocked Cholesky
    ("fd", "2d64_chol_W", None, [(-1, {"sweep": "k_coarse_chol"})]),
    ("chol", BLOCKED_SMALLEST, None, [(-1, {"sweep": "k_coarse_chol_blocked"})]),
    ("fd", "2d64_chol_W", "chol_dense", [(-1, {"sweep": "k_coarse_chol_blocked"})]),
    # low-rank draws: k_lr_small, the dense-column path, k_tail's, the row lists around quads and the z-sweep
    ("lr", "2d32_point_global", None, LOWRANK),
    ("lr", "3d32_points_tail_W", None, LOWRANK + [("any", {"sweep": "k_tail<3>", "lowrank": "small"})]),
    ("lr", "2d128_point_global_W", None, [(0, {"lowrank^": "dense"}), ("any", {"lowrank": "small"})]),
    ("lr", "3d_96x48x48_points", None, [(1, {"sweep": "k_sweep_quads<3>", "quads": "window", "lowrank^": ""})]),
    ("lr", "3d_aniso_zres_points", None, LOWRANK + [(0, {"sweep^": "k_zsweep_rb7<"})]),
    # low-rank fallback launches
    ("lr", "2d32_point_global", "lr_small,lr_merge,tail", LOWRANK),
    # field mode; the FEM fine level
    ("field", FIELD_SMALLEST, None, [(0, {"sweep": "k_fsweep<2>"}), (1, {"sweep": "k_fsweep<2>"})]),
    ("fem", FEM_SMALLEST, None, [(0, {"sweep^": "k_sweep_quads<2>"})]),
]


def _id(case):
    family, name, paths, _ = case
    return f"{family}-{name}" + (f"-{'all_paths' if paths == PAR.ALL_PATHS else paths}" if paths else "")


@pytest.mark.parametrize("case", CYCLES, ids=_id)
def test_cycles_bitwise_all_words(hip_device, monkeypatch, case):
    """A: whole cycles against the oracle with seed, chain id and sample index all beyond 32 bits; the low sample
    word carries into the high one between the third and the fourth cycle."""
    family, name, paths, labels = case
    s, mc, p, lat = _build_with_paths(monkeypatch, family, name, ALL, paths)
    _check_labels(s, p, _id(case), labels)
    if family == "lr" and paths:  # the generic fix / patch / restore launches, not k_lr_small
        assert all(s.level_kernels(level).get("lowrank") != "small" for level in range(p.nlevel))
    if family == "fem":
        assert s.level_desc(0)["npoints"] == 3 ** lat.dim
    if family == "field":
        assert s.level_desc(0)["varcoef"]
    _check_cycles(s, mc, lat, S_CARRY)
    s.close()


SINGLE_LABELS = {"3d16": [(0, {"sweep": "k_sweep_rb<3>"}), (1, {"sweep": "k_tail<3>"}), (2, {"sweep": "k_tail<3>"})],
                 "2d64_template_W": [(0, {"sweep": "k_rb2d"}), (1, {"sweep": "k_tail<2>"}), (3, {"sweep": "k_tail<2>"})],
                 "3d_zsr_edges": ZS}


@pytest.mark.parametrize("word", list(SINGLE))
@pytest.mark.parametrize("name", ["3d16", "2d64_template_W", "3d_zsr_edges"])
def test_cycles_bitwise_single_word(hip_device, name, word):
    """A with one word beyond 32 bits at a time, on the three cheapest configurations on their default paths: a
    failure names the word, the labels the launches."""
    words = SINGLE[word]
    s, mc, p, lat = _build("fd", name, words)
    _check_labels(s, p, f"{name}-{word}", SINGLE_LABELS[name])
    _check_cycles(s, mc, lat, words[2])
    s.close()


@pytest.mark.parametrize("name", ["3d16", "2d_aniso_ssor", "3d_zsr_edges", "3d_24x20x12", "2d_100x60"])
def test_component_sweeps_high_counter_words(hip_device, name):
    """B: sor_sampler_apply on every level, both directions, with the tag's top bit set and hi32(sample) != 0 (the
    component path chooses its kernels differently from the cycle)."""
    s, mc, p, lat = _build("fd", name, (SEED64, CHAIN_H, S_HIGH))
    rng = np.random.default_rng(7)
    for level in range(p.nlevel):
        n = s.level_desc(level)["ndof"]
        b = rng.standard_normal(n)
        x = rng.standard_normal(n)
        tag = 2 ** 31 + 5 + level
        for direction in (mg.FORWARD, mg.BACKWARD):
            d = s.sor_sampler_apply(level, direction, tag, S_HIGH, b, x)
            o = mc.sor_sampler_apply(level, direction, tag, S_HIGH, b, x)
            assert not np.array_equal(d, x)
            assert np.array_equal(d, o), f"level {level} dir {direction} sampler"
    s.close()


def _chol_batch(name, nchains=1, chain=0, seed=CH.SEED):
    shape, kw = CH.CONFIGS[name]
    s, p, lat = CH._make(shape, kw, chain=chain, nchains=nchains, seed=seed)
    return s, lat


def _batch_oracle(family, name, paths=None):
    """the oracle of chain CHAIN_H of a batch case (built after the device handles: MGMC_DISABLE is set by then)"""
    tokens = paths.split(",") if paths else []
    O.set_no_fold("fold" in tokens)
    try:
        if family == "fd":
            shape, kw = PAR.CONFIGS[name]
            p = mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **kw})
            return O.Oracle.fd_own(shape, p, 25.0, mode=O.MULTICOLOUR, seed=SEED64, chain=CHAIN_H)
        if family == "chol":
            shape, kw = CH.CONFIGS[name]
            p = mg.MultigridParameters(**{"nlevel": 2, "smoother": "SOR", "coarse_solver": "Cholesky", **kw})
            return O.Oracle.fd_own(shape, p, 25.0, mode=O.MULTICOLOUR, seed=SEED64, chain=CHAIN_H)
        shape, kw, (radius, nmeas, glob) = LR.CONFIGS[name]
        p = mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **kw})
        op, lat = LR.measured(shape, 25.0, radius, nmeas, glob)
        mc = O.Oracle.fd_own(shape, p, 25.0, mode=O.MULTICOLOUR, seed=SEED64, chain=CHAIN_H)
        mc.set_lowrank(op.get_B())
        return mc
    finally:
        O.set_no_fold(False)


# family, configuration, MGMC_DISABLE, nchains: one row per chain-key site (section C)
BATCHES = [
    ("fd", "3d_zsr_edges", None, 4),  # z-sweep, coarse SSOR
    ("fd", "3d_192x48x48_5lvl", None, 4),  # the restriction's spare workgroups, k_tail
    ("fd", "2d_qr_aniso_ssor_W", None, 4),
    ("fd", "2d_200x120_4lvl", None, 4),
    ("fd", "3d8_1lvl", None, 4),
    ("fd", "2d48_1lvl_items", None, 4),  # chain_key into k_coarse_ssor_lds's second draw loop
    ("fd", "3d12_1lvl_items", None, 4),
    ("fd", "2d64_chol_W", None, 4),  # dense Cholesky
    ("chol", "2d256_nl2", None, 4),  # blocked Cholesky (test_blocked_coarse_cholesky_batched_chains' case)
    ("lr", "2d32_point_global", None, 4),
    ("lr", "2d32_point_global_chol", None, 4),
    ("lr", "3d32_points_tail_W", None, 4),
    ("lr", "2d128_points_tail", None, 4),
    ("fd", "2d64_template_W", PAR.ALL_PATHS, 4),  # gibbs_chain in the generic launches
    ("lr", "3d32_points_tail_W", "lr_small,lr_merge,tail", 2),
]


@pytest.mark.parametrize("case", BATCHES, ids=lambda c: _id(c[:3] + (None,)))
def test_batched_chains_bitwise_all_words(hip_device, monkeypatch, case):
    """C: chain c of a batch with chain0 = CHAIN_H under SEED64 equals the one-chain handle CHAIN_H + c bit for bit
    across the carry (what a chain-key site that drops ^ seed_hi breaks), and chain 0 equals the oracle's chain."""
    family, name, paths, nchains = case
    if paths:
        monkeypatch.setenv("MGMC_DISABLE", paths)
    make = {"fd": BAT._prior, "lr": BAT._posterior, "chol": _chol_batch}[family]
    zb, f, x0, qoi = BAT._check_batch(make, name, nchains=nchains, nsteps=6, seed=SEED64, chain0=CHAIN_H,
                                      sample0=S_CARRY)
    mc = _batch_oracle(family, name, paths)
    mc.set_rhs(f)
    mc.set_state(x0)
    mc.set_sample_index(S_CARRY)
    assert np.array_equal(zb[0], mc.sample(6, qoi))


@pytest.mark.parametrize("name", ["3d16", "2d_100x60"])
def test_unrolled_graph_across_the_carry(hip_device, monkeypatch, name):
    """D: MGMC_GRAPH_UNROLL=4, 10 cycles from S_CARRY = two unrolled launches (the carry inside the first) and two
    single cycles, against the oracle's sequential cycles."""
    monkeypatch.setenv("MGMC_GRAPH_UNROLL", "4")
    s, mc, p, lat = _build("fd", name, ALL)
    f = np.random.default_rng(3).standard_normal(lat.Nvertex)
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    for h in (s, mc):
        h.set_sample_index(S_CARRY)
        h.set_state(np.zeros(lat.Nvertex))
    s.fix_rhs(f)
    mc.set_rhs(f)
    assert np.array_equal(s.sample(10, qoi), mc.sample(10, qoi))
    assert np.array_equal(s.get_state(), mc.get_state())
    assert s.get_sample_index() == S_CARRY + 10
    s.close()


def test_timed_sampling_across_the_carry(hip_device):
    """D: mgmc_sample_timed_stride(10, 4) from S_CARRY: the series and the state of a plain sample(10) twin, and the
    index ends at S_CARRY + 10."""
    shape, kw = PAR.CONFIGS["3d16"]
    s = PAR.make(shape, chain=CHAIN_H, seed=SEED64, **kw)[0]
    t, p, lat = PAR.make(shape, chain=CHAIN_H, seed=SEED64, **kw)
    q = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    s.set_sample_index(S_CARRY)
    t.set_sample_index(S_CARRY)
    s.sample_timed(10, q, stride=4)
    z = t.sample(10, q)
    assert np.all(np.isfinite(z)) and np.array_equal(s.get_series(10), z)
    assert np.array_equal(s.get_state(), t.get_state())
    assert s.get_sample_index() == t.get_sample_index() == S_CARRY + 10
    s.close()
    t.close()


def test_field_stats_across_the_carry(hip_device):
    """D: field_stats(1), then 6 cycles from S_CARRY on three chains: the moments of the numpy mirror -- the
    recorded-cycle count does not depend on the sample index."""
    a, b = FS._make("3d16_k3"), FS._make("3d16_k3")
    a.set_sample_index(S_CARRY)
    b.set_sample_index(S_CARRY)
    a.field_stats(1)
    a.sample(6)
    mirror = FS.Mirror(b.ndof)
    FS._mirror_cycles(b, mirror, 6, 0, 1)
    assert mirror.n == 6 * a.nchains and np.any(mirror.m2 > 0)
    FS._assert_equal(a, mirror)
    assert a.get_sample_index() == b.get_sample_index() == S_CARRY + 6
    a.close()
    b.close()


def test_nonfinite_guard_names_a_64_bit_sample_index(hip_device):
    """D: the guard stores 1 + the sample index in a 64-bit control word; from S_HIGH on, the index in the error
    text is the one of a cycle of this call (nothing truncates it on the way to the message)."""
    shape, kw = PAR.CONFIGS["3d16"]
    s, p, lat = PAR.make(shape, chain=CHAIN_H, seed=SEED64, **kw)
    q = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    s.set_sample_index(S_HIGH)
    s.sample(3, q)  # finite chain: no error
    x = s.get_state()
    x[1] = np.nan
    s.set_state(x)
    with pytest.raises(mg.MgmcError, match="non-finite chain state") as e:
        s.sample(40, q)
    assert e.value.code == _native.MGMC_E_NONFINITE
    index = int(re.search(r"in sample (\d+)", str(e.value)).group(1))
    assert S_HIGH + 3 <= index < S_HIGH + 43
    s.close()
