"""Every kernel family on NaN-filled LDS, against the CPU oracle (-m gpu).

MGMC_POISON=1 (read by mgmc_create*) launches k_lds_poison -- NaN into the LDS of every compute unit -- before
every op of the cycle graph and before every LDS-using launch of the per-level entry points.  A kernel that
reads an LDS word before a barrier orders the write of it (the missing barrier of the plain k_zsweep_rb7,
mgmc_zsweep.hpp "if (!PROLONG) __syncthreads()" after the table fill) then computes with
NaN in the first round of workgroups, and the result differs from the oracle's.  Each case here

  * asserts through level_kernels() that the kernel it is written for is the one the level selects,
  * runs once (no repetition: under the poison a first-round workgroup of a racy kernel has nothing but NaN
    to read, so one run decides), and
  * compares uint64 views with the CPU oracle -- MULTICOLOUR, and FAITHFUL where
    test_gpu_parity.test_component_kernels_bitwise uses it -- never with a second device run.

test_lds_poison_reaches_every_probe_workgroup measures the instrument itself (mgmc_debug_lds_probe).

The negative control of record is profiles/r06/fix/race_stress.txt: the build without that barrier returned a
non-finite or changed stand-alone 256^3 sweep in 78 of 80 poisoned repetitions, the fixed one in 0 of 80.  It is
not repeated here (no pre-fix kernel is built, nothing loops)."""
import numpy as np
import pytest

import multigridmc_amd as mg
from tests import oracle_lib as O
from tests import test_gpu_lowrank as LR
from tests.test_gpu_parity import CONFIGS

pytestmark = pytest.mark.gpu

SEED = 5418513
KAPPA_SQ = 25.0
SSOR = dict(smoother="SSOR", npresmooth=2, omega=1.1, coarse_scaling=0.9)  # as tests/test_gpu_rhs_zero.py


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make(monkeypatch, shape, disable=None, **kw):
    """A poisoned handle (the flag is read at creation) and its parameters / lattice."""
    monkeypatch.setenv("MGMC_POISON", "1")
    if disable:
        monkeypatch.setenv("MGMC_DISABLE", disable)
    p = mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **kw})
    lat = mg.Lattice(*shape)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, KAPPA_SQ), SEED, p, device=0)
    return s, p, lat


def oracle(p, lat, mode=O.MULTICOLOUR):
    if mode == O.FAITHFUL:
        return O.Oracle.fd(lat.shape, p, KAPPA_SQ, mode=O.FAITHFUL, seed=SEED)
    return O.Oracle.fd_own(lat.shape, p, KAPPA_SQ, mode=O.MULTICOLOUR, seed=SEED)


# ---- the instrument ----

def test_lds_poison_reaches_every_probe_workgroup(hip_device, monkeypatch):
    """After k_lds_poison, 2 x (compute units) workgroups of its footprint (80 KB of LDS, 1024 threads: one
    resident round of the device) read their LDS without writing it: every one reads NaN in every word."""
    s, p, lat = make(monkeypatch, (16, 16, 16))
    r = s.debug_lds_probe()
    print("lds probe, MGMC_POISON=1:", r)
    assert r["nwg"] >= 2
    assert r["nwg_all_nan"] == r["nwg"]
    assert r["min_nan_fraction"] == 1.0
    s.close()


def test_lds_probe_returns_without_poison(hip_device, monkeypatch):
    """Without MGMC_POISON no fill is launched; the probe still returns, with whatever the LDS held."""
    monkeypatch.delenv("MGMC_POISON", raising=False)
    p = mg.MultigridParameters(nlevel=3)
    lat = mg.Lattice(16, 16, 16)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, KAPPA_SQ), SEED, p, device=0)
    r = s.debug_lds_probe()
    print("lds probe, no poison:", r)
    assert r["nwg"] >= 2 and 0 <= r["nwg_all_nan"] <= r["nwg"] and 0.0 <= r["min_nan_fraction"] <= 1.0
    s.close()


# ---- stand-alone noisy sweeps (mgmc_sor_sampler_apply) ----
# name: shape, parameters, MGMC_DISABLE, level, the level's "sweep" label (prefix)
SWEEPS = {
    # partial y tiles, a short second z-chunk of an up / down pair.  This case and the two below run the plain
    # k_zsweep_rb7 whose first noise draw needs the barrier after the table fill
    "z16_64x44x40": ((64, 44, 40), dict(nlevel=2), None, 0, "k_zsweep_rb7<32,16,...,0>"),
    "z16_192x48x40": ((192, 48, 40), dict(nlevel=2), None, 0, "k_zsweep_rb7<32,16,...,0>"),
    # 520 tiles of 20 rows: the instance of the 512^3 benchmark
    "z20_128x84x416": ((128, 84, 416), dict(nlevel=2), None, 0, "k_zsweep_rb7<32,20,...,0>"),
    "jsweep128": ((512, 44, 60), dict(nlevel=3), None, 1, "k_jsweep_half<128"),
    "quads3": ((512, 32, 32), dict(nlevel=5), None, 2, "k_sweep_quads<3>"),
    "quads2": ((256, 128), dict(nlevel=3), None, 1, "k_sweep_quads<2>"),
    # (every 2D pair-pass level takes the quad passes: the pair passes are what MGMC_DISABLE=quads leaves)
    "pairs2": ((256, 128), dict(nlevel=3), "quads", 1, "k_sweep_pairs<2>"),
    "rb2d": ((256, 256), dict(nlevel=2), None, 0, "k_rb2d"),
    # 24-pair rows (64 % 24 != 0): the three-load window instances, 120-thread workgroups
    "quads3_window": ((96, 96, 96), dict(nlevel=5), None, 1, "k_sweep_quads<3>"),
    # 80-pair rows: the colour-pair passes on their default path, 3 rows = 240 of 256 threads
    "pairs3_default": ((320, 24, 16), dict(nlevel=3), None, 1, "k_sweep_pairs<3>"),
}


@pytest.mark.parametrize("name", list(SWEEPS))
def test_poisoned_noisy_sweep_bitwise(hip_device, monkeypatch, name):
    """One noisy sweep per direction on the named level, random b and x, against the MULTICOLOUR oracle."""
    shape, kw, disable, level, label = SWEEPS[name]
    s, p, lat = make(monkeypatch, shape, disable, **kw)
    assert s.level_kernels(level)["sweep"].startswith(label), s.level_kernels(level)
    assert s.level_kernels(level).get("quads") == ("window" if name == "quads3_window" else None)
    mc = oracle(p, lat)
    rng = np.random.default_rng(7)
    n = s.level_desc(level)["ndof"]
    b = rng.standard_normal(n)
    x = rng.standard_normal(n)
    for direction in (mg.FORWARD, mg.BACKWARD):
        d = s.sor_sampler_apply(level, direction, 5, 77, b, x)
        o = mc.sor_sampler_apply(level, direction, 5, 77, b, x)
        assert np.all(np.isfinite(d)), f"{name} dir {direction}: non-finite sweep"
        assert same_bits(d, o), f"{name} dir {direction}"
    s.close()


# ---- stand-alone deterministic entries ----
# name: shape, parameters, {level: {label key: value}} asserted before the level's calls
COMPONENTS = {
    "zres7_partial": ((256, 40, 48), dict(nlevel=2), {0: {"residual_restrict": "k_zresrestrict<7,64,4>"}}),
    "zres27": ((512, 16, 24), dict(nlevel=3), {1: {"residual_restrict": "k_zresrestrict<27,64,4>"}}),
    "zres_lasttile": ((132, 36, 20), dict(nlevel=2), {0: {"residual_restrict": "k_zresrestrict<7,64,4>",
                                                          "sweep": "k_sweep_rb<3>"}}),
    # the small kernels.  Levels 1-2 are k_tail's in the cycle: the per-level calls run their separate kernels
    # there (colour-pair passes, k_residual_restrict<3,27>, k_restrict, the prolongation, k_operator_apply)
    "small16": ((16, 16, 16), dict(nlevel=3), {0: {"residual_restrict": "k_zresrestrict<7,16,4>",
                                                    "sweep": "k_sweep_rb<3>"},
                                               1: {"sweep": "k_tail<3>"}, 2: {"sweep": "k_tail<3>"}}),
}


@pytest.mark.parametrize("name", list(COMPONENTS))
def test_poisoned_component_entries_bitwise(hip_device, monkeypatch, name):
    """operator_apply, restrict, prolongate_add, residual_restrict and two deterministic sweeps per direction on
    every level.  The contract of test_component_kernels_bitwise: the FAITHFUL oracle's CSR arithmetic bit for
    bit, except the residual of a fold level, which is the MULTICOLOUR oracle's; the sweeps are MULTICOLOUR's."""
    shape, kw, labels = COMPONENTS[name]
    s, p, lat = make(monkeypatch, shape, **kw)
    for level, want in labels.items():
        got = s.level_kernels(level)
        assert all(got.get(k) == v for k, v in want.items()), (level, got)
    faithful = oracle(p, lat, O.FAITHFUL)
    mc = oracle(p, lat)
    rng = np.random.default_rng(42)
    for level in range(p.nlevel):
        n = s.level_desc(level)["ndof"]
        x = rng.standard_normal(n)
        f = rng.standard_normal(n)
        assert same_bits(s.operator_apply(level, x), faithful.operator_apply(level, x)), f"level {level} apply"
        for direction in (mg.FORWARD, mg.BACKWARD):
            assert same_bits(s.smoother_apply(level, direction, 2, f, x),
                             mc.smoother_apply(level, direction, 2, f, x)), f"level {level} dir {direction} smoother"
        if level + 1 < p.nlevel:
            xc = rng.standard_normal(s.level_desc(level + 1)["ndof"])
            assert same_bits(s.restrict(level, f), faithful.restrict(level, f)), f"level {level} restrict"
            assert same_bits(s.prolongate_add(level, 1.3, xc, x),
                             faithful.prolongate_add(level, 1.3, xc, x)), f"level {level} prolongate_add"
            ref = mc if O.fold_level(s.level_desc(level)) else faithful
            assert same_bits(s.residual_restrict(level, f, x), ref.residual_restrict(level, f, x)), \
                f"level {level} residual_restrict"
    s.close()


# ---- low-rank ----

def test_poisoned_lowrank_small_path_bitwise(hip_device, monkeypatch):
    """The smallest posterior set-up of tests/test_gpu_lowrank.py on the lr_small path (32^2, three point
    measurements and the global average): a stand-alone noisy sweep per direction (low-rank noise patch, sweep,
    B_bar fix) and the posterior residual + restriction on every level, then two cycles, against the oracle with
    the same B."""
    monkeypatch.setenv("MGMC_POISON", "1")
    s, mc, p, lat, op = LR.make("2d32_point_global")
    assert all(s.level_kernels(level)["lowrank"] == "small" for level in range(p.nlevel))
    rng = np.random.default_rng(3)
    for level in range(p.nlevel):
        n = s.level_desc(level)["ndof"]
        x = rng.standard_normal(n)
        b = rng.standard_normal(n)
        for direction in (mg.FORWARD, mg.BACKWARD):
            assert same_bits(s.sor_sampler_apply(level, direction, 5, 77, b, x),
                             mc.sor_sampler_apply(level, direction, 5, 77, b, x)), f"level {level} dir {direction}"
        if level + 1 < p.nlevel:
            assert same_bits(s.residual_restrict(level, b, x), mc.residual_restrict(level, b, x)), f"level {level}"
    # k_lr_small itself (the fix / restore / patch between the ops of level 0) runs in the cycle only
    f = rng.standard_normal(lat.Nvertex)
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    s.fix_rhs(f)
    mc.set_rhs(f)
    assert same_bits(s.sample(2, qoi), mc.sample(2, qoi))
    assert same_bits(s.get_state(), mc.get_state())
    s.close()


# ---- poisoned cycles: the kernels only the graph reaches ----
# name: shape, parameters, MGMC_DISABLE, {level: {label key: value}} asserted once f is zero
ZS = "k_zsweep_rb7<32,16,...,PROLONG>"
CYCLES = {
    # coarse_scaling 1 (a power of two): PROLONG = 2; one post-sweep: the copy back
    "3d128_zsweep_odd": (*CONFIGS["3d128_zsweep_odd"], None, {0: {"post_sweep": ZS, "rhs": "zero"}}),
    # coarse_scaling 0.9: PROLONG = 1; SSOR: backward sweeps
    "128x36x24_ssor": ((128, 36, 24), dict(nlevel=2, **SSOR), None, {0: {"post_sweep": ZS, "rhs": "zero"}}),
    "3d_zres7": (*CONFIGS["3d_zres7"], None, {0: {"residual_restrict": "k_zresrestrict<7,64,4>", "rhs": "zero"}}),
    # k_tail, its spare noise workgroups and the noise the quad passes of level 2 read from them
    "3d_jsweep_tail": (*CONFIGS["3d_jsweep_tail"], None,
                       {0: {"rhs": "zero"}, 2: {"sweep": "k_sweep_quads<3>", "noise": "restriction+tail"},
                        3: {"sweep": "k_tail<3>"}, 4: {"sweep": "k_tail<3>"}}),
    "3d16": (*CONFIGS["3d16"], None, {1: {"sweep": "k_tail<3>"}, 2: {"sweep": "k_tail<3>"}}),  # the tail, not k_coarse_ssor_lds
    # ... which a two-level hierarchy with a coarsest level of 15 x 7 x 7 runs (no tail below three levels)
    "3d_aniso": (*CONFIGS["3d_aniso"], None, {1: {"sweep": "k_coarse_ssor_lds (or separate colour passes)"}}),
    "2d512_qrestrict": (*CONFIGS["2d512_qrestrict"], None, {1: {"residual_restrict": "k_quads_restrict2d"},
                                                            2: {"residual_restrict": "k_quads_restrict2d"}}),
    "2d_qr_cj5_notail": (*CONFIGS["2d_qr_cj5"], "tail", {1: {"residual_restrict": "k_quads_restrict2d"}}),
    "2d64_chol_W": (*CONFIGS["2d64_chol_W"], None, {3: {"sweep": "k_coarse_chol"}}),
    # selects the dense k_coarse_chol (7^3 coarsest unknowns) ...
    "3d128_zsweep_chol": (*CONFIGS["3d128_zsweep_chol"], None, {0: {"rhs": "zero"}, 4: {"sweep": "k_coarse_chol"}}),
    # ... so the blocked solves come from test_gpu_cholesky.py's 2d256_nl2 (127^2 > 8,192 coarsest unknowns)
    "2d256_chol_blocked": ((256, 256), dict(nlevel=2, coarse_solver="Cholesky"), None,
                           {1: {"sweep": "k_coarse_chol_blocked"}}),
    # rows that are no powers of two: the window quad passes reading restriction- and tail-drawn noise under a
    # three-tile fine z-sweep; k_rb2d with partial tiles over k_quads_restrict2d with idle threads and a tail
    "3d_192x48x48_5lvl": (*CONFIGS["3d_192x48x48_5lvl"], None,
                          {0: {"rhs": "zero"}, 1: {"sweep": "k_sweep_quads<3>", "quads": "window"},
                           2: {"sweep": "k_sweep_quads<3>", "quads": "window", "noise": "restriction+tail"},
                           3: {"sweep": "k_tail<3>"}, 4: {"sweep": "k_tail<3>"}}),
    "2d_200x120_4lvl": (*CONFIGS["2d_200x120_4lvl"], None,
                        {0: {"sweep": "k_rb2d"}, 1: {"residual_restrict": "k_quads_restrict2d"},
                         2: {"sweep": "k_tail<2>"}, 3: {"sweep": "k_tail<2>"}}),
}


@pytest.mark.parametrize("name", list(CYCLES))
def test_poisoned_cycle_bitwise(hip_device, monkeypatch, name):
    """One apply(f, x) with a random f, then two cycles of the device-resident loop from that state with f = 0 (on
    a z-sweep level 0: the FZ instances of the sweeps and of the residual + restriction): state and QoI series
    against the MULTICOLOUR oracle."""
    shape, kw, disable, labels = CYCLES[name]
    s, p, lat = make(monkeypatch, shape, disable, **kw)
    mc = oracle(p, lat)
    f = np.random.default_rng(11).standard_normal(lat.Nvertex)
    x_dev, x_orc = np.zeros(lat.Nvertex), np.zeros(lat.Nvertex)
    s.apply(f, x_dev)
    mc.apply(f, x_orc)
    assert same_bits(x_dev, x_orc), f"{name}: apply"
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    zero = np.zeros(lat.Nvertex)
    s.fix_rhs(zero)
    s.set_state(x_dev)
    mc.set_rhs(zero)
    mc.set_state(x_orc)
    for level, want in labels.items():
        got = s.level_kernels(level)
        assert all(got.get(k) == v for k, v in want.items()), (level, got)
    if s.level_kernels(0)["sweep"].startswith("k_zsweep_rb7"):
        assert s.level_kernels(0).get("rhs") == "zero"
    assert same_bits(s.sample(2, qoi), mc.sample(2, qoi)), f"{name}: QoI series"
    assert same_bits(s.get_state(), mc.get_state()), f"{name}: state"
    s.close()
