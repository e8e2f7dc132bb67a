"""Tuning neutrality (-m gpu): the parity cases under re-tuned launch shapes.

multigridmc_amd/csrc/mgmc_tuning.hpp holds every tile shape, chunk depth, thread count and launch threshold, and
claims that none of them changes a result.  This module is what checks the claim: the libraries
build/libmgmc_tune_<name>.so (tests/tuning_variants.py, scripts/build_tuning_variants.py) are the product sources
with those constants moved down ("lo") and up ("hi"), so that tile and chunk edges fall on other rows, planes and
columns, thresholds select the other kernel of a pair, and instances the default reaches only at 256^3 / 512^3 (the
512-thread 7-point restriction, the unhalved z-chunk depths, quad passes on long rows) run at test sizes.

The parent computes every case's expected arrays once with the MULTICOLOUR CPU oracle and writes them to .npy files;
one fresh child process per library (the product library as control, then each variant; one after another) runs
tests/tuning_worker.py over all cases and reports, per case, pass / fail, the level_kernels labels and for a mismatch
the first and last differing (i, j, k) and the count -- which localises a broken tile or chunk edge.  The
parametrised tests only look results up.  If a child times out, is killed by a signal, exits with 134 / 139 or
reports a HIP error, no further child is started and every case that did not run fails as "not run after <library>
died".

Per case: two apply(f, x) cycles with a random f; four prior cycles (f = 0, zero state: the zero-right-hand-side
instances) with QoI series and final state; for cases marked sweeps the per-level smoother, noisy sweep and
residual + restriction calls.  Some cases run again with MGMC_POISON=1 (NaN-filled LDS before every launch).

The vd_* cases are matrix handles with a variable-diagonal fine level (a case's "operator" key; the lattices of
tests/test_gpu_vardiag.py): the VD instance of k_zsweep_rb7 borrows ZS_TYP and ZS_TZ (12 / 16 / 20-row tiles under
lo / control / hi), and lo's ZR7_WIDE_MIN_TILES = 1 selects k_zresrestrict<7,64,8,512,...,VD>, which the default
build reaches only at 512^3 and no other test launches.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import multigridmc_amd as mg
from tests import oracle_lib as O
from tests.test_gpu_field_stats import Mirror
from tests.test_gpu_lowrank import CONFIGS as LR_CONFIGS, measured
from tests.test_gpu_parity import CONFIGS
from tests.test_gpu_vardiag import CASES as VD_CASES, build_operator
from tests.tuning_variants import VARIANTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 5418513
KAPPA_SQ = 25.0
LIBRARIES = ["control"] + list(VARIANTS)

# Wall time of the control child (product library, every case below, interpreter start and library load included)
# measured on an MI355X: 3.70 s (the lo / hi children: 3.66 / 3.65 s; the slowest case, depth_hi, 0.42 s; the
# eight vd_* cases together 0.96 s, of which the first, vd_A, 0.24 s and the three-level vd_C 0.27 s).  A
# child's limit is 5 x that (spilled or tiny-tile variants and first-use code-object loads are slower); a child that
# exceeds it counts as hung.
CONTROL_SECONDS = 3.70
CHILD_TIMEOUT = 5 * CONTROL_SECONDS

# ---- the z-chunk depth cases ----
# zsweep_depth (mgmc_capi.hip) halves a z-sweep's chunk depth while 4 * tiles_xy * nchunks < 3 * 2 * num_cu, so below
# 256^3 every variant's ZS_TZ / ZS_TZP ends at 8.  The smallest even-extent two-level lattice that keeps a variant's
# depths on tiles that meet every kind of edge: two 64-wide x tiles (nx = 128); ny - 1 = max(ZS_TY, ZS_TYP) + 1
# interior rows, i.e. a full tile and a one-row tile of the taller shape, a full and a partial tile of the other
# (2 x 2 = 4 tiles in x-y for both launches); and nchunks = ceil((nz - 1) / tz) >= 6 * num_cu / (4 * 4) = 96 on the
# 256 compute units of an MI355X for the deeper of the two depths, i.e. nz - 1 = tz * 95 + 1: the last chunk is
# partial (one plane).  lo: 128 x 18 x 3042 (7.0 M unknowns), hi: 128 x 30 x 6082 (23 M).  The test asserts the tz=
# label and that the device reports no more compute units than this.
NUM_CU = 256


def depth_shape(variant):
    edits = VARIANTS[variant]
    rows = max(edits["ZS_TY"], edits["ZS_TYP"]) + 1
    tiles_xy = 2 * 2
    assert all(-(-rows // edits[k]) == 2 for k in ("ZS_TY", "ZS_TYP"))
    nchunks = -(-6 * NUM_CU // (4 * tiles_xy))
    shape = (128, rows + 1, max(edits["ZS_TZ"], edits["ZS_TZP"]) * (nchunks - 1) + 2)
    assert all(v % 2 == 0 for v in shape)
    return shape


def _case(cid, shape, params, *, disable="", poison=False, nchains=1, sweeps=False, measurements=None,
          field_stats=0, oracle=None, operator=None, lowrank=False):
    """operator: None (the FD prior, kappa^2 = 25) or a matrix handle's, "fd_periodic" | "dominant"
    (tests/test_gpu_vardiag.build_operator; lowrank: with its three point measurements and the global average)."""
    return {"id": cid + ("-poison" if poison else ""), "shape": list(shape), "params": params, "disable": disable,
            "poison": poison, "nchains": nchains, "chain0": 0 if nchains == 1 else 11, "sweeps": sweeps,
            "measurements": measurements, "field_stats": field_stats, "oracle": oracle or cid,
            "operator": operator, "lowrank": lowrank}


def _vardiag(name, *, suffix="", **kw):
    """A lattice of tests/test_gpu_vardiag.py (A .. D) as a matrix handle: the VD instances of k_zsweep_rb7 (which
    borrow ZS_TYP and ZS_TZ) and of k_zresrestrict<7, ...> (ZR7_WIDE_MIN_TILES) under the variants."""
    shape, params = VD_CASES[name]
    cid = f"vd_{name}{suffix}" + (f"-k{kw['nchains']}" if kw.get("nchains") else "")
    return _case(cid, shape, params, operator="dominant" if name == "D" else "fd_periodic", oracle=cid, **kw)


def _prior(name, **kw):
    shape, params = CONFIGS[name]
    cid = name + ("-no_" + kw["disable"] if kw.get("disable") else "") + (f"-k{kw['nchains']}" if kw.get("nchains") else "")
    # (MGMC_DISABLE=fuse_prolong / jsweep and the poison change no arithmetic: the same expected arrays)
    return _case(cid, shape, params, oracle=name + (f"-k{kw['nchains']}" if kw.get("nchains") else ""), **kw)


def _posterior(name, **kw):
    shape, params, meas = LR_CONFIGS[name]
    cid = "lr_" + name + (f"-k{kw['nchains']}" if kw.get("nchains") else "")
    return _case(cid, shape, params, measurements=list(meas), **kw)


POISONED = [("3d_zsr_edges", dict(sweeps=True)), ("3d128_zsweep_odd", dict(sweeps=True)), ("3d192_zsweep", {}),
            ("3d128_zsweep", {}), ("3d_aniso_zsweep_ssor", {}), ("3d_zres7", {}), ("3d_jsweep_tail", {}),
            ("3d64_4lvl", {})]

CASES = (
    [_prior("3d_zsr_edges", sweeps=True), _prior("3d_zsr_edges", nchains=2),
     _prior("3d128_zsweep_odd", sweeps=True), _prior("3d192_zsweep"),
     _prior("3d128_zsweep"), _prior("3d128_zsweep", disable="fuse_prolong"),
     _prior("3d_zres7"), _prior("3d_zres_lasttile"), _prior("3d_aniso_zsweep_ssor"),
     _prior("3d_zres27"), _prior("3d_zres27", disable="jsweep"),
     _prior("3d_jsweep_ssor_W"), _prior("3d_jsweep_tail"), _prior("3d_320x24x16"),
     _prior("3d64_4lvl"), _prior("3d96_5lvl"), _prior("3d136_4lvl"),
     _prior("2d512_qrestrict"), _prior("2d_200x120_4lvl"), _prior("2d64_template_W")] +
    [_posterior("3d_aniso_zres_points"), _posterior("2d128_point_global_W"), _posterior("3d128_global_inplace_W"),
     _posterior("3d_96x48x48_points"), _posterior("3d_96x48x48_points", nchains=3),
     _posterior("3d32_ball_global"), _posterior("3d32_ball_global", nchains=3)] +
    [_case("field_stats_24x20x12-k2", (24, 20, 12), dict(nlevel=2), nchains=2, field_stats=5)] +
    [_case(f"depth_{v}", depth_shape(v), dict(nlevel=2)) for v in VARIANTS] +
    # the separate z-marching prolongation with PROLONG_Z planes per thread needs 2^21 fine pair items (below that
    # it takes PROLONG_Z_SMALL, which 3d128_zsweep-no_fuse_prolong reaches): the smaller depth case has 3.3 M, and
    # a plane count (3041) that no PROLONG_Z of 4 / 8 / 16 divides
    [_case("depth_lo-no_fuse_prolong", depth_shape("lo"), dict(nlevel=2), disable="fuse_prolong", oracle="depth_lo")] +
    # JS_ROUNDS: the j-marching plan (jsweep_plan) cuts a plane's steps into as many chunks as JS_ROUNDS rounds of the
    # 3 x 256 resident workgroups hold, at most one per step.  The j-marching levels above have at most 15 planes x
    # 16 steps per half: one chunk per step with one round already.  Here level 1 is 256 x 58 x 58: 28 planes x 30
    # steps = 840 > 768, so one round gives 768 / 28 = 27 -> 15 chunks of 2 steps (the multi-step chunk path) and
    # two rounds 30 chunks of 1 step.  No label carries the plan (the j-marching level's labels are compared whole
    # elsewhere): tests/test_tuning_host.py asserts it from jsweep_plan_dims, the function launch_jsweep calls, for 256
    # compute units, and test_jsweep_rounds_case_is_sized_for_the_device checks the device's count against it
    [_case("3d_jsweep_rounds", (512, 116, 116), dict(nlevel=3))] +
    # matrix handles with a variable-diagonal fine level: no other case runs a VD kernel through a variant, and the
    # default build reaches the 512-thread k_zresrestrict<7,64,8,...,VD> only at 512^3
    [_vardiag("A", sweeps=True), _vardiag("B", sweeps=True), _vardiag("C"), _vardiag("D"), _vardiag("B", nchains=3),
     _vardiag("B", suffix="_lowrank", lowrank=True)] +
    [_prior(name, poison=True, **kw) for name, kw in POISONED] +
    [_vardiag("A", sweeps=True, poison=True), _vardiag("C", poison=True)])
CASE_IDS = [c["id"] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


# ---- expected labels ----
# case id -> library -> [(level, key, value)]; a key ending in "^" asserts a prefix, a value None the key's absence.
# The control rows are the default labels (the worker itself is right); the variant rows name the instance the case
# is there for.  tests/test_tuning_host.py asserts the same selections on the CPU from the host-side level plan.
def _tz(variant, unhalved):
    e = VARIANTS[variant]
    return f"{e['ZS_TZ']}/{e['ZS_TZP']}" if unhalved else "8/8"


LABELS = {
    "3d_zsr_edges": {"control": [(0, "sweep", "k_zsweep_rb7<32,16,...,0>"), (0, "post_sweep^", "k_zsweep_rb7<32,16,"),
                                 (0, "tz", "8/8"), (0, "rhs", "zero")],
                     "lo": [(0, "sweep", "k_zsweep_rb7<32,16,...,0>"), (0, "post_sweep^", "k_zsweep_rb7<32,12,"),
                            (0, "tz", "8/8"), (0, "residual_restrict", "k_zresrestrict<7,64,8>")],
                     "hi": [(0, "sweep^", "k_zsweep_rb7<32,28,"), (0, "post_sweep^", "k_zsweep_rb7<32,20,"),
                            (0, "tz", "8/8")]},
    "3d128_zsweep_odd": {"lo": [(0, "post_sweep^", "k_zsweep_rb7<32,12,")], "hi": [(0, "sweep^", "k_zsweep_rb7<32,28,")]},
    "3d192_zsweep": {"lo": [(0, "sweep^", "k_zsweep_rb7<32,16,")], "hi": [(0, "sweep^", "k_zsweep_rb7<32,28,")]},
    "3d128_zsweep": {"control": [(1, "sweep", "k_sweep_quads<3>"), (1, "quads", None),
                                 (1, "residual_restrict", "k_zresrestrict<27,64,4>")],
                     "lo": [(1, "sweep", "k_sweep_quads<3>"), (1, "quads", "window"),
                            (1, "residual_restrict", "k_zresrestrict<27,64,8>"),
                            (0, "residual_restrict", "k_zresrestrict<7,64,8>")],
                     "hi": [(1, "quads", None), (1, "residual_restrict", "k_zresrestrict<27,16,4>")]},
    "3d128_zsweep-no_fuse_prolong": {"control": [(0, "post_sweep", None)], "lo": [(0, "post_sweep", None)],
                                     "hi": [(0, "post_sweep", None)]},
    "3d_zres7": {"control": [(0, "residual_restrict", "k_zresrestrict<7,64,4>")],
                 "lo": [(0, "residual_restrict", "k_zresrestrict<7,64,8>")],
                 "hi": [(0, "residual_restrict", "k_zresrestrict<7,64,4>")]},
    "3d_zres_lasttile": {"control": [(0, "residual_restrict", "k_zresrestrict<7,64,4>")],
                         "lo": [(0, "residual_restrict", "k_zresrestrict<7,64,8>")]},
    "3d_aniso_zsweep_ssor": {"control": [(1, "sweep", "k_sweep_quads<3>"), (1, "quads", None)],
                             "lo": [(1, "sweep", "k_sweep_pairs<3>")],
                             "hi": [(1, "sweep", "k_sweep_quads<3>"),
                                    (1, "residual_restrict", "k_zresrestrict<27,32,4>")]},
    "3d_zres27": {lib: [(1, "sweep^", "k_jsweep_half<128")] for lib in LIBRARIES},
    "3d_zres27-no_jsweep": {"control": [(1, "sweep", "k_sweep_pairs<3>")], "lo": [(1, "sweep", "k_sweep_pairs<3>")],
                            "hi": [(1, "sweep", "k_sweep_quads<3>"), (1, "quads", "window")]},
    "3d_jsweep_ssor_W": {lib: [(1, "sweep^", "k_jsweep_half<128")] for lib in LIBRARIES},
    "3d_jsweep_tail": {"control": [(1, "sweep^", "k_jsweep_half<128"), (2, "sweep", "k_sweep_quads<3>"),
                                   (2, "noise", "restriction+tail")],
                       # (under lo level 2's 64-pair rows take the pair passes: no quad-pass level, the tail draws
                       # nothing here; TAIL_PN_WG 0 is reached through 3d64_4lvl and 3d96_5lvl)
                       "lo": [(1, "sweep^", "k_jsweep_half<128"), (2, "sweep", "k_sweep_pairs<3>"), (2, "noise", None)],
                       "hi": [(1, "sweep^", "k_jsweep_half<128"), (1, "residual_restrict", "k_zresrestrict<27,32,4>"),
                              (2, "sweep", "k_sweep_quads<3>"), (2, "noise", "restriction+tail")]},
    "3d_jsweep_rounds": {lib: [(1, "sweep^", "k_jsweep_half<128")] for lib in LIBRARIES},
    "3d_320x24x16": {"control": [(1, "sweep", "k_sweep_pairs<3>")], "lo": [(1, "sweep", "k_sweep_pairs<3>")],
                     "hi": [(1, "sweep", "k_sweep_quads<3>"), (1, "quads", "window")]},
    "3d64_4lvl": {"control": [(0, "residual_restrict", "k_zresrestrict<7,64,4>"),
                              (1, "residual_restrict", "k_zresrestrict<27,16,4>"), (1, "quads", None),
                              (1, "noise", "tail")],
                  "lo": [(0, "residual_restrict", "k_zresrestrict<7,64,8>"),
                         (1, "residual_restrict", "k_zresrestrict<27,64,8>"), (1, "quads", "window"),
                         (1, "noise", "tail")],
                  "hi": [(0, "residual_restrict", "k_zresrestrict<7,16,4>"),
                         (1, "residual_restrict", "k_zresrestrict<27,16,4>"), (1, "noise", "tail")]},
    # (the quad-pass levels above a tail read their first post-sweep's noise from the tail launch's spare workgroups,
    # TAIL_PN_WG 0 / 255 of them under lo / hi: noise=tail; under lo the 27-point restriction onto level 2 is not the
    # small one and also draws that level's first pre-sweep's: restriction+tail)
    "3d96_5lvl": {"control": [(0, "residual_restrict", "k_zresrestrict<7,64,4>"), (1, "quads", "window"),
                              (1, "noise", "tail"), (2, "noise", "tail")],
                  "lo": [(0, "residual_restrict", "k_zresrestrict<7,64,8>"), (1, "quads", "window"),
                         (2, "quads", "window"), (1, "noise", "tail"), (2, "noise", "restriction+tail")],
                  "hi": [(0, "residual_restrict", "k_zresrestrict<7,16,4>"), (1, "quads", "window"),
                         (1, "noise", "tail"), (2, "noise", "tail")]},
    "3d136_4lvl": {"control": [(0, "residual_restrict", "k_zresrestrict<7,64,4>"),
                               (1, "residual_restrict", "k_zresrestrict<27,64,4>")],
                   "lo": [(0, "residual_restrict", "k_zresrestrict<7,64,8>"), (1, "sweep", "k_sweep_pairs<3>"),
                          (2, "quads", "window")],
                   "hi": [(0, "residual_restrict", "k_zresrestrict<7,64,4>"),
                          (1, "residual_restrict", "k_zresrestrict<27,16,4>")]},
    "2d512_qrestrict": {lib: [(0, "sweep", "k_rb2d"), (1, "residual_restrict", "k_quads_restrict2d")]
                        for lib in LIBRARIES},
    "lr_3d128_global_inplace_W": {lib: [(0, "lowrank", "dense,rhs_inplace"), (1, "lowrank", "dense")]
                                  for lib in LIBRARIES},
    "lr_3d_96x48x48_points": {lib: [(1, "sweep", "k_sweep_quads<3>"), (1, "quads", "window")] for lib in LIBRARIES},
}
# the VD instances: the sweep's tile is the variant's ZS_TYP, the 7-point restriction the 512-thread 64 x 8 instance
# under lo (ZR7_WIDE_MIN_TILES 1), which the default build selects only at 512^3 and no other test launches
_VD_ROWS = {"control": 16, "lo": VARIANTS["lo"]["ZS_TYP"], "hi": VARIANTS["hi"]["ZS_TYP"]}
_VD_RES = {"control": "k_zresrestrict<7,64,4>", "lo": "k_zresrestrict<7,64,8>", "hi": "k_zresrestrict<7,64,4>"}
assert _VD_ROWS == {"control": 16, "lo": 12, "hi": 20}
for _c in CASES:
    if _c["operator"] and not _c["poison"]:
        LABELS[_c["id"]] = {
            lib: [(0, "sweep", f"k_zsweep_rb7<32,{_VD_ROWS[lib]},...,0,VD>"), (0, "residual_restrict", _VD_RES[lib]),
                  (0, "diag", "field"), (0, "post_sweep", None), (0, "rhs", None), (0, "tz", "8")] +
                 ([(1, "sweep", "k_fsweep<3>"), (1, "residual_restrict", "k_fresidual + k_restrict"), (1, "diag", None)]
                  if _c["params"]["nlevel"] > 2 else [])
            for lib in LIBRARIES}
        LABELS[_c["id"] + "-poison"] = LABELS[_c["id"]]
for _v in VARIANTS:  # a variant's own depth case keeps its ZS_TZ / ZS_TZP; every smaller z-sweep case ends at 8 / 8
    LABELS[f"depth_{_v}"] = {_v: [(0, "tz", _tz(_v, True))]}
for _name, _ in POISONED:  # the poisoned runs select what the plain ones do
    if _name in LABELS:
        LABELS[_name + "-poison"] = LABELS[_name]


# ---- the parent's side: expected arrays from the CPU oracle ----
def _parameters(case):
    return mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **case["params"]})


def _oracle(case, chain):
    p = _parameters(case)
    if case["operator"]:  # the replay of the matrix the worker hands to mgmc_create_csr
        op, _ = build_operator(tuple(case["shape"]), case["operator"] == "dominant", case["lowrank"])
        rowptr, col, val = getattr(op, "base_operator", op).get_csr()
        mc = O.Oracle.csr(tuple(case["shape"]), p, rowptr, col, val, mode=O.MULTICOLOUR, seed=SEED)
        mc.reseed(SEED, chain)
        if case["lowrank"]:
            mc.set_lowrank(op.get_B())
        return mc, p
    mc = O.Oracle.fd_own(tuple(case["shape"]), p, KAPPA_SQ, mode=O.MULTICOLOUR, seed=SEED, chain=chain)
    if case["measurements"] is not None:
        op, _ = measured(tuple(case["shape"]), KAPPA_SQ, *case["measurements"])
        mc.set_lowrank(op.get_B())
    return mc, p


def write_expected(case, directory):
    """The arrays tests/tuning_worker.py compares with, for one oracle key (a case and the cases that share its
    arithmetic)."""
    os.makedirs(directory)
    lat = mg.Lattice(*case["shape"])
    n, k = lat.Nvertex, case["nchains"]

    def save(key, a):
        np.save(os.path.join(directory, key + ".npy"), np.asarray(a, dtype=np.float64))

    if case["field_stats"]:
        chains = [_oracle(case, case["chain0"] + c)[0] for c in range(k)]
        mirror = Mirror(n)
        for mc in chains:
            mc.set_rhs(np.zeros(n))
            mc.set_state(np.zeros(n))
        for _ in range(case["field_stats"]):
            for mc in chains:  # the kernel folds the chains of a cycle in order
                mc.sample(1)
                mirror.fold(mc.get_state())
        save("fs_count", [float(mirror.n)])
        save("fs_mean", mirror.mean)
        save("fs_m2", mirror.m2)
        return
    qoi = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    f = np.random.default_rng(7).standard_normal(n)
    apply1, apply2, series, state = [], [], [], []
    for c in range(k):
        mc, p = _oracle(case, case["chain0"] + c)
        x = np.zeros(n)
        mc.apply(f, x)
        apply1.append(x.copy())
        mc.apply(f, x)
        apply2.append(x.copy())
        mc.set_rhs(np.zeros(n))
        mc.set_state(np.zeros(n))
        series.append(mc.sample(4, qoi))
        state.append(mc.get_state())
        if case["sweeps"]:
            rng = np.random.default_rng(7)
            for level in range(p.nlevel):
                b = rng.standard_normal(mc.ndof(level))
                x = rng.standard_normal(mc.ndof(level))
                for direction in (mg.FORWARD, mg.BACKWARD):
                    save(f"smoother_l{level}_d{direction}", mc.smoother_apply(level, direction, 2, b, x))
                    save(f"sampler_l{level}_d{direction}", mc.sor_sampler_apply(level, direction, 5 + level, 77, b, x))
                if level + 1 < p.nlevel:
                    save(f"residual_restrict_l{level}", mc.residual_restrict(level, b, x))
    save("apply1", apply1)
    save("apply2", apply2)
    save("prior_series", series)
    save("prior_state", state)


def library_path(name):
    if name == "control":
        from multigridmc_amd import _native
        return _native.LIB_PATH
    # the recipe of __graft_entry__.build(): compiles nothing while the library's inputs are unchanged, rebuilds a
    # missing or stale one; a failure here fails the tests
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "build_tuning_variants.py"), name], check=True,
                   stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "build", f"libmgmc_tune_{name}.so")


HIP_ERROR_TEXTS = ("illegal memory access", "HSA_STATUS_ERROR", "hipError", "Memory access fault", "HIP error")


def run_child(name, cases_file):
    """One child over every case; returns ({case id: result}, worker header, why it died or None)."""
    env = dict(os.environ, MGMC_LIBRARY=library_path(name))
    env.pop("MGMC_DISABLE", None)
    env.pop("MGMC_POISON", None)
    proc = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "tuning_worker.py"), cases_file], env=env,
                            cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    died = None
    t0 = time.perf_counter()
    try:
        out, err = proc.communicate(timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        proc.kill()
        out, err = proc.communicate()
        died = f"no result within {CHILD_TIMEOUT:.0f} s (counts as a hang)"
    wall = time.perf_counter() - t0
    results, header = {}, {}
    for line in out.splitlines():
        try:
            rec = json.loads(line)
        except ValueError:
            continue
        if "id" in rec:
            results[rec["id"]] = rec
        else:
            header = rec
    header["wall_seconds"] = round(wall, 2)
    if died is None and proc.returncode != 0:
        died = f"exit status {proc.returncode}" + (" (signal)" if proc.returncode < 0 or proc.returncode in (134, 139) else "")
    if died is None and any(t in out or t in err for t in HIP_ERROR_TEXTS):
        died = "a HIP error in its output"
    if died is not None:
        died += ": " + err.strip()[-600:]
    return results, header, died


@pytest.fixture(scope="session")
def tuning_results(hip_device, tmp_path_factory):
    """{library: {case id: result}}: the expected arrays once, then one child per library, one after another."""
    top = tmp_path_factory.mktemp("tuning")
    O.set_threads(min(16, O.cpu_share()))
    try:
        done = {}
        for case in CASES:
            directory = os.path.join(str(top), case["oracle"])
            if case["oracle"] not in done:
                write_expected(case, directory)
                done[case["oracle"]] = dict(case)
            # cases that share expected arrays must ask for the same ones
            assert all(done[case["oracle"]][key] == case[key] for key in ("shape", "params", "nchains", "chain0",
                                                                          "measurements", "field_stats", "operator",
                                                                          "lowrank"))
            case["dir"] = directory
    finally:
        O.set_threads(1)
    cases_file = os.path.join(str(top), "cases.json")
    with open(cases_file, "w") as fh:
        json.dump(CASES, fh)
    results, dead = {}, None
    for name in LIBRARIES:
        if dead is not None:
            results[name] = {"results": {}, "header": {}, "died": f"not run after {dead[0]} died ({dead[1]})"}
            continue
        res, header, died = run_child(name, cases_file)
        print(f"tuning child {name}: {header.get('wall_seconds')} s wall, {sum(r['seconds'] for r in res.values()):.1f} s "
              f"in its {len(res)} cases, {header}")
        results[name] = {"results": res, "header": header, "died": died}
        if died is not None:
            dead = (name, died)
    return results


@pytest.mark.parametrize("case_id", CASE_IDS)
@pytest.mark.parametrize("library", LIBRARIES)
def test_tuning_variant_bitwise(tuning_results, library, case_id):
    """The case through the library equals the oracle bit for bit, and ran the kernel instances it is there for."""
    child = tuning_results[library]
    r = child["results"].get(case_id)
    if r is None:
        why = child["died"] or "the worker printed no result for it"
        pytest.fail(f"{case_id} under {library}: not run after {library} died: {why}" if "not run after" not in why
                    else f"{case_id} under {library}: {why}")
    print(json.dumps(r))
    assert r["error"] is None, f"{case_id} under {library}: {r['error']}"
    assert not r["mismatches"], f"{case_id} under {library}: {r['mismatches']} (labels {r['labels']})"
    assert r["ok"] and r["checks"] > 0
    for level, key, value in LABELS.get(case_id, {}).get(library, []):
        got = r["labels"][level]
        if key.endswith("^"):
            assert got.get(key[:-1], "").startswith(value), (case_id, library, level, got, child["header"])
        else:
            assert got.get(key) == value, (case_id, library, level, got, child["header"])
    if library == "lo":  # QUADS_LANES 0: the three-load window on every 3D quad-pass level
        assert all(k.get("quads") == "window" for k in r["labels"] if k["sweep"] == "k_sweep_quads<3>"), r["labels"]
    # (every z-sweep case below the depth cases' size ends at 8 / 8; 3d_jsweep_rounds, 6.9 M unknowns, is sized for
    # its level 1 and keeps deeper chunks)
    if r["labels"][0]["sweep"].startswith("k_zsweep_rb7") and not case_id.startswith(("depth_", "3d_jsweep_rounds")):
        # (the VD instance is the plain sweep only: its label carries one depth)
        want = "8" if r["labels"][0].get("diag") == "field" else "8/8"
        assert r["labels"][0]["tz"] == want, (case_id, r["labels"][0])


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_depth_case_is_sized_for_the_device(tuning_results, variant):
    """The depth case's lattice is sized for 256 compute units: what the device reports must not be more (with
    fewer, the chunks stay unhalved all the more)."""
    header = tuning_results[variant]["header"]
    assert header, tuning_results[variant]["died"]
    assert 0 < header["num_cu"] <= NUM_CU, header


def test_jsweep_rounds_case_is_sized_for_the_device(tuning_results):
    """3d_jsweep_rounds: with 3 workgroups per compute unit (53,264 B of LDS each), one round must not hold a chunk
    per step of level 1's 28 planes x 30 steps (3 num_cu / 28 < 30), and two rounds must (6 num_cu / 28 >= 30)."""
    header = tuning_results["control"]["header"]
    assert header, tuning_results["control"]["died"]
    assert 3 * header["num_cu"] // 28 < 30 <= 6 * header["num_cu"] // 28, header
