"""Rao-Blackwellised field statistics on the device (-m gpu): mgmc_field_stats_enable_cond /
MultigridMCSampler.field_stats(conditional=True), multigridmc_amd/csrc/mgmc_fieldcond.hpp.

  * bitwise against a numpy mirror (the twin-handle scheme of tests/test_gpu_field_stats.py): the twin runs the same
    cycles one at a time; per recorded state y = operator_apply(0, x), c = x + (f - y) / d in float64, folded with the
    Welford / batch-means statements of the kernel.  d itself bitwise against numpy: the stencil's centre or the
    matrix diagonal, plus B_ik B_ik / Sigma_k in ascending k.  10 cycles without batching, then 10 with batch 3.
    The cases are the smallest that reach each way to go wrong: for the fused z-march one x tile with a row
    overhang (both the f = 0 and the f != 0 instance), two x tiles x three row tiles, chunk seams with a short last
    chunk, thinning; for the two passes every operator family, a d-field, three chains, a sparse and a dense low-rank
    column;
  * the fused z-march against the forced two passes, bitwise; one fused case on NaN-poisoned LDS;
  * the chain is untouched; lifecycle; mgmc_set_lowrank resets; unrolled and timed graphs record every cycle;
  * statistics: the three assertions of tests/test_field_cond_host.py on the device's own fields (3D 16^3), and the
    template's 2D 32^2 posterior against the exact posterior; the driver's --rao-blackwell.
"""
import os
import re

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd.driver import ExactTargets, _measured_values, main
from multigridmc_amd.parameters import MeasurementParameters
from tests.test_field_batch_host import BatchMirror
from tests.test_field_cond_host import (RB_BATCH, RB_CHAIN, RB_DISCARD, RB_KEPT, RB_LEVELS, RB_SHAPE,
                                        conditional_precision, small_posterior)
from tests.test_gpu_field_stats import CHAIN0, GOLD, SEED, _template_posterior

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERIODIC = mg.PeriodicCorrelationLengthModel(0.2, 0.4)


def _chunk_depth():
    """FC_TZ, the z-march's planes per chunk (a bitwise-neutral tile constant of mgmc_fieldcond.hpp)"""
    text = open(os.path.join(ROOT, "multigridmc_amd", "csrc", "mgmc_fieldcond.hpp")).read()
    return int(re.search(r"constexpr int FC_TZ = (\d+);", text).group(1))


TZ = _chunk_depth()


def _fd(shape, nlevel):
    return mg.ShiftedLaplaceFDOperator(mg.Lattice(*shape), 25.0), mg.MultigridParameters(nlevel=nlevel)


def _rhs(op, seed=11):
    return np.random.default_rng(seed).standard_normal(op.get_ndof())


def _measured_3d(shape):
    """two point measurements on a 3D FD prior"""
    mp = MeasurementParameters(radius=0.0, variance_scaling=1e-3, measure_global=False, variance_global=0.02)
    mp.measurement_locations = [[0.3, 0.4, 0.45], [0.7, 0.55, 0.6]]
    mp.variance = [1.5, 2.5]
    return mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(mg.Lattice(*shape), 25.0), mp)


# name -> (operator, parameters, nchains, right-hand side or None, stride, path)
def _case(name):
    if name == "z64x22x10":  # one x tile, a row overhang, the FZ instance
        return _fd((64, 22, 10), 2) + (1, None, 1, "fused")
    if name == "z64x22x10_f":  # the instance that reads f
        op, p = _fd((64, 22, 10), 2)
        return op, p, 1, _rhs(op), 1, "fused"
    if name == "z128x34x18":  # two x tiles, three row tiles: x and y tile edges
        return _fd((128, 34, 18), 2) + (1, None, 1, "fused")
    if name == "z64x20_seams":  # two whole chunks and a short one
        return _fd((64, 20, 2 * TZ + 6), 2) + (1, None, 1, "fused")
    if name == "z64x22x10_stride3":
        return _fd((64, 22, 10), 2) + (1, None, 3, "fused")
    if name == "3d16":
        return _fd((16, 16, 16), 3) + (1, None, 1, "two_pass")
    if name == "3d24x20x12":
        return _fd((24, 20, 12), 2) + (1, None, 1, "two_pass")
    if name == "2d48x40":
        return _fd((48, 40), 3) + (1, None, 1, "two_pass")
    if name == "2d32_squared":  # the reach-2 layout
        return (mg.SquaredShiftedLaplaceFDOperator(mg.Lattice(32, 32), 25.0), mg.MultigridParameters(nlevel=2), 1, None, 1,
                "two_pass")
    if name == "fem16":
        return (mg.ShiftedLaplaceFEMOperator(mg.Lattice(16, 16, 16), 25.0), mg.MultigridParameters(nlevel=3), 1, None, 1,
                "two_pass")
    if name == "periodic64x16x16":  # variable diagonal through the matrix path: a d-field on a z-sweep level
        return (mg.ShiftedLaplaceFDOperator(mg.Lattice(64, 16, 16), PERIODIC), mg.MultigridParameters(nlevel=2), 1, None, 1,
                "two_pass")
    if name == "3d16_k3":  # chain order
        return _fd((16, 16, 16), 3) + (3, None, 1, "two_pass")
    if name == "2d32_posterior":  # the template's 8 measurements, f != 0: d-field, low-rank y
        op, mp, p = _template_posterior()
        return op, p, 1, _rhs(op), 1, "two_pass"
    if name == "2d12x10_global":  # a dense low-rank column
        op = small_posterior()
        return op, mg.MultigridParameters(nlevel=2), 1, _rhs(op, 5), 1, "two_pass"
    raise KeyError(name)


FUSED = ["z64x22x10", "z64x22x10_f", "z128x34x18", "z64x20_seams", "z64x22x10_stride3"]
TWO_PASS = ["3d16", "3d24x20x12", "2d48x40", "2d32_squared", "fem16", "periodic64x16x16", "3d16_k3", "2d32_posterior",
            "2d12x10_global"]


def _make(name, chain=CHAIN0):
    op, p, k, f, stride, path = _case(name)
    s = mg.MultigridMCSampler(op, SEED, p, device=0, chain_id=chain, nchains=k)
    if f is not None:
        s.fix_rhs(f)
    return s


def _numpy_d(s, op):
    """d from the operator alone: the centre of level 0's stencil or the matrix diagonal, plus the low-rank part"""
    desc = s.level_desc(0)
    base = getattr(op, "base_operator", op)
    if desc["varcoef"]:
        diag = base.matrix().diagonal()
    else:
        diag = np.full(s.ndof, desc["stencil"][13 if len(desc["shape"]) == 3 else 4])
    return conditional_precision(diag, op.get_B() if hasattr(op, "get_B") else None)


def _conditional_mean(b, x, f, d):
    y = b.operator_apply(0, x)
    return x + ((f if f is not None else np.zeros_like(x)) - y) / d


def _mirror_cycles(b, mirror, ncycles, stride, f, d):
    """ncycles single cycles of b, numbered 1 ... from the enable; the recorded ones folded, chains in order"""
    for j in range(ncycles):
        b.sample(1)
        if (j + 1) % stride == 0:
            mirror.record([_conditional_mean(b, b.get_state(c), f, d) for c in range(b.nchains)])


def _assert_moments(a, mirror):
    n, mean, m2 = a.field_moments()
    assert n == mirror.n
    assert np.array_equal(mean, mirror.mean)
    assert np.array_equal(m2, mirror.m2)


def _assert_batch(a, mirror):
    nb, bmean, bm2 = a.field_batch_moments()
    assert a.field_batch_info() == {"batch": mirror.B, "nbatches": mirror.nb}
    assert nb == mirror.nb
    assert np.array_equal(bmean, mirror.bmean)
    assert np.array_equal(bm2, mirror.bm2)


@pytest.mark.parametrize("name", FUSED + TWO_PASS)
def test_bitwise_equal_numpy_mirror(hip_device, name):
    op, p, k, f, stride, path = _case(name)
    a, b = _make(name), _make(name)
    assert a.field_cond_info() == {"enabled": False, "path": None}
    a.field_stats(stride, conditional=True)
    assert a.field_cond_info() == {"enabled": True, "path": path}
    assert a.field_stats_info() == {"enabled": True, "stride": stride, "nrecorded": 0}
    d = a.field_conditional_precision()
    want = _numpy_d(a, op)
    assert np.array_equal(d.view(np.uint64), want.view(np.uint64))
    a.sample(10)
    mirror = BatchMirror(b.ndof, k, 1 << 30)
    _mirror_cycles(b, mirror, 10, stride, f, d)
    assert mirror.n == (10 // stride) * k and np.any(mirror.m2 > 0)
    _assert_moments(a, mirror)
    # the same handles, ten more cycles with batch means of 3 recorded cycles
    a.field_stats(stride, batch=3, conditional=True)
    assert a.field_cond_info() == {"enabled": True, "path": path}
    assert a.field_stats_info()["nrecorded"] == 0
    a.sample(10)
    mirror = BatchMirror(b.ndof, k, 3)
    _mirror_cycles(b, mirror, 10, stride, f, d)
    assert mirror.nb == (10 // stride) // 3
    if stride == 1:
        assert mirror.nb == 3 and mirror.bsum.any() and np.any(mirror.bm2 > 0)
    _assert_moments(a, mirror)
    _assert_batch(a, mirror)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["z64x22x10", "z128x34x18"])
def test_fused_equals_forced_two_pass(hip_device, name):
    a, t = _make(name), _make(name)
    a.field_stats(1, batch=3, conditional=True)
    t.field_stats(1, batch=3, conditional=True, two_pass=True)
    assert a.field_cond_info()["path"] == "fused" and t.field_cond_info()["path"] == "two_pass"
    a.sample(10)
    t.sample(10)
    for fa, ft in zip(a.field_moments() + a.field_batch_moments(), t.field_moments() + t.field_batch_moments()):
        assert np.array_equal(fa, ft)
    assert np.any(a.field_moments()[2] > 0) and np.any(a.field_batch_moments()[2] > 0)
    a.close()
    t.close()


def test_fused_on_poisoned_lds(hip_device, monkeypatch):
    monkeypatch.setenv("MGMC_POISON", "1")
    a = _make("z128x34x18")
    monkeypatch.delenv("MGMC_POISON")
    b = _make("z128x34x18")
    a.field_stats(1, batch=3, conditional=True)
    assert a.field_cond_info()["path"] == "fused"
    d = a.field_conditional_precision()
    a.sample(10)
    mirror = BatchMirror(b.ndof, 1, 3)
    _mirror_cycles(b, mirror, 10, 1, None, d)
    _assert_moments(a, mirror)
    _assert_batch(a, mirror)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["z64x22x10", "3d16"])
def test_chain_is_untouched_and_unchanged_after_off(hip_device, name):
    a, b = _make(name), _make(name)
    q = a.ndof // 2
    kernels = [a.level_kernels(l) for l in range(a.nlevel)]
    a.field_stats(conditional=True)
    assert [a.level_kernels(l) for l in range(a.nlevel)] == kernels
    za, zb = a.sample(10, q), b.sample(10, q)
    assert np.array_equal(za, zb)
    assert np.array_equal(a.get_state(), b.get_state())
    a.field_stats_off()
    assert a.field_stats_info() == {"enabled": False, "stride": 0, "nrecorded": 0}
    assert a.field_cond_info() == {"enabled": False, "path": None}
    assert [a.level_kernels(l) for l in range(a.nlevel)] == kernels
    za, zb = a.sample(5, q), b.sample(5, q)
    assert np.array_equal(za, zb)
    assert np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_lifecycle(hip_device):
    live = mg.load_library().mgmc_live_handles()
    s, b = _make("z64x22x10"), _make("z64x22x10")
    # while the mode is off
    with pytest.raises(mg.MgmcError) as e:
        s.field_conditional_precision()
    assert e.value.code == -1
    with pytest.raises(ValueError):
        s.field_rb_mean_variance()
    s.field_stats(1)
    with pytest.raises(mg.MgmcError):  # plain statistics: still off
        s.field_conditional_precision()
    with pytest.raises(ValueError):
        s.field_rb_mean_variance()
    s.field_stats_off()
    for args in [(0, 0, 0), (1, -1, 0), (1, 0, 2), (1, 0, 4)]:  # stride < 1, batch < 0, unknown flag bits
        assert s.lib.mgmc_field_stats_enable_cond(s.handle, *args) == -1
    assert s.field_stats_info()["enabled"] is False
    with pytest.raises(ValueError):
        s.field_stats(1, two_pass=True)
    # conditional -> plain -> conditional: every switch resets
    s.field_stats(1, conditional=True)
    with pytest.raises(ValueError):  # n = 0
        s.field_rb_mean_variance()
    with pytest.raises(mg.MgmcError):  # wrong n
        s._chk(s.lib.mgmc_field_stats_get_cond_precision(s.handle, None, s.ndof + 1))
    d = s.field_conditional_precision()
    s.sample(4)
    b.sample(4)
    assert s.field_stats_info()["nrecorded"] == 4
    s.field_stats(1)
    assert s.field_cond_info() == {"enabled": False, "path": None}
    assert s.field_stats_info() == {"enabled": True, "stride": 1, "nrecorded": 0}
    s.sample(3)
    plain = BatchMirror(b.ndof, 1, 1 << 30)
    for _ in range(3):
        b.sample(1)
        plain.record([b.get_state()])
    _assert_moments(s, plain)  # the plain fields fold x
    s.field_stats(1, batch=2, conditional=True)
    assert s.field_cond_info() == {"enabled": True, "path": "fused"}
    n, mean, m2 = s.field_moments()
    assert n == 0 and not mean.any() and not m2.any()
    s.sample(5)
    mirror = BatchMirror(b.ndof, 1, 2)
    _mirror_cycles(b, mirror, 5, 1, None, d)
    _assert_moments(s, mirror)
    _assert_batch(s, mirror)
    mean_rb, var_rb = s.field_rb_mean_variance()
    assert np.array_equal(mean_rb, mirror.mean) and np.array_equal(var_rb, 1.0 / d + mirror.m2 / 5)
    # batched conditional -> batched plain: a reset too
    s.field_stats(1, batch=2)
    assert s.field_cond_info()["enabled"] is False and s.field_stats_info()["nrecorded"] == 0
    # reset keeps the mode; set_qoi_vector keeps recording
    s.field_stats(1, conditional=True, two_pass=True)
    assert s.field_cond_info() == {"enabled": True, "path": "two_pass"}
    s.sample(2)
    b.sample(2)
    s.reset_field_stats()
    assert s.field_cond_info() == {"enabled": True, "path": "two_pass"} and s.field_stats_info()["nrecorded"] == 0
    rows, vals = mg.measurement_vector(mg.Lattice(64, 22, 10), [0.5, 0.5, 0.5], 0.1)
    mirror = BatchMirror(b.ndof, 1, 1 << 30)
    s.sample(2)
    _mirror_cycles(b, mirror, 2, 1, None, d)
    for h in (s, b):
        h.set_qoi_vector(rows, vals)
    s.sample(3, mg.QOI_VECTOR)
    _mirror_cycles(b, mirror, 3, 1, None, d)
    _assert_moments(s, mirror)
    s.close()  # conditional at close: mgmc_destroy frees the fields and the buffer
    b.close()
    assert mg.load_library().mgmc_live_handles() == live


def test_set_rhs_and_set_state_do_not_reset(hip_device):
    """a new right-hand side switches the fused instance (f = 0 -> f != 0) and keeps the statistics"""
    a, b = _make("z64x22x10"), _make("z64x22x10")
    a.field_stats(conditional=True)
    d = a.field_conditional_precision()
    mirror = BatchMirror(b.ndof, 1, 1 << 30)
    a.sample(3)
    _mirror_cycles(b, mirror, 3, 1, None, d)
    f = _rhs(a.linear_operator, 4)
    x0 = _rhs(a.linear_operator, 6)
    for h in (a, b):
        h.fix_rhs(f)
        h.set_state(x0)
    a.sample(3)
    _mirror_cycles(b, mirror, 3, 1, f, d)
    assert a.field_cond_info() == {"enabled": True, "path": "fused"}
    _assert_moments(a, mirror)
    a.close()
    b.close()


def test_set_lowrank_resets_and_replans(hip_device):
    op = _measured_3d((64, 22, 10))
    p = mg.MultigridParameters(nlevel=2)
    a = mg.MultigridMCSampler(op.base_operator, SEED, p, chain_id=CHAIN0)
    b = mg.MultigridMCSampler(op.base_operator, SEED, p, chain_id=CHAIN0)
    a.field_stats(1, batch=2, conditional=True)
    assert a.field_cond_info()["path"] == "fused"
    a.sample(3)
    b.sample(3)
    assert a.field_stats_info()["nrecorded"] == 3
    for h in (a, b):
        h.set_lowrank(op.get_B())
    assert a.field_cond_info() == {"enabled": True, "path": "two_pass"}
    assert a.field_stats_info() == {"enabled": True, "stride": 1, "nrecorded": 0}
    assert a.field_batch_info() == {"batch": 2, "nbatches": 0}
    d = a.field_conditional_precision()
    want = _numpy_d(a, op)
    assert np.array_equal(d.view(np.uint64), want.view(np.uint64))
    assert np.count_nonzero(d != d[0]) == 2  # (two point measurements)
    a.sample(5)
    mirror = BatchMirror(b.ndof, 1, 2)
    _mirror_cycles(b, mirror, 5, 1, None, d)
    _assert_moments(a, mirror)
    _assert_batch(a, mirror)
    for h in (a, b):  # and back to the prior: fused again, reset again
        h.set_lowrank(None)
    assert a.field_cond_info() == {"enabled": True, "path": "fused"}
    assert a.field_stats_info()["nrecorded"] == 0
    d = a.field_conditional_precision()
    assert np.all(d == d[0])
    a.sample(4)
    mirror = BatchMirror(b.ndof, 1, 2)
    _mirror_cycles(b, mirror, 4, 1, None, d)
    _assert_moments(a, mirror)
    _assert_batch(a, mirror)
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["z64x22x10", "2d48x40"])
def test_unrolled_and_timed_graphs_record_every_cycle(hip_device, monkeypatch, name):
    monkeypatch.setenv("MGMC_GRAPH_UNROLL", "4")
    a = _make(name)
    monkeypatch.delenv("MGMC_GRAPH_UNROLL")
    b = _make(name)
    a.field_stats(conditional=True)
    d = a.field_conditional_precision()
    a.sample(10)  # two launches of the 4-cycle graph + two single cycles
    a.sample_timed(4)
    mirror = BatchMirror(b.ndof, 1, 1 << 30)
    _mirror_cycles(b, mirror, 14, 1, None, d)
    _assert_moments(a, mirror)
    a.close()
    b.close()


def _z_scores(s, exact_var, exact_mean):
    """the estimator's z-scores from the device's own fields: (z variance, z mean, var(c), tau)"""
    n, mean, m2 = s.field_moments()
    tau = np.maximum(s.field_iact(), 1.0)
    mean_rb, var_rb = s.field_rb_mean_variance()
    var_c = m2 / n
    z_var = np.abs(var_rb - exact_var) / (var_c * np.sqrt(2.0 * tau / n))
    z_mean = np.abs(mean_rb - exact_mean) / np.sqrt(var_c * tau / n)
    return z_var, z_mean, var_c, tau


def test_statistics_on_the_device_16cubed(hip_device):
    """The case of tests/test_field_cond_host.py::test_rao_blackwell_on_the_oracle with the device's fields:
    field_stats(1, batch=50, conditional=True), 200 cycles discarded, 4000 kept; var(x) from a plain twin.
    Measured on the device: the oracle's figures (max z variance 3.23, max z mean 3.44, largest
    var(c) / var(x) 0.305; the device reproduces the oracle's chain)."""
    op = mg.ShiftedLaplaceFDOperator(mg.Lattice(*RB_SHAPE), 25.0)
    p = mg.MultigridParameters(nlevel=RB_LEVELS)
    a = mg.MultigridMCSampler(op, SEED, p, chain_id=RB_CHAIN)
    t = mg.MultigridMCSampler(op, SEED, p, chain_id=RB_CHAIN)
    for h in (a, t):
        h.sample(RB_DISCARD)
    a.field_stats(1, batch=RB_BATCH, conditional=True)
    t.field_stats(1)
    a.sample(RB_KEPT)
    t.sample(RB_KEPT)
    exact = np.diag(np.linalg.inv(op.matrix().toarray()))
    z_var, z_mean, var_c, tau = _z_scores(a, exact, 0.0)
    var_x = t.field_mean_variance()[1]
    var_rb = a.field_rb_mean_variance()[1]
    rms_rb = np.sqrt(np.mean(((var_rb - exact) / exact) ** 2))
    rms_x = np.sqrt(np.mean(((var_x - exact) / exact) ** 2))
    print(f"device 16^3: max z variance {z_var.max():.2f}, max z mean {z_mean.max():.2f}, largest var(c) / var(x) "
          f"{(var_c / var_x).max():.3f}, median tau {np.median(tau):.2f}, RMS relative error of the variance "
          f"RB {rms_rb:.4f} / plain {rms_x:.4f} = {rms_rb / rms_x:.3f}")
    assert a.field_batch_info() == {"batch": RB_BATCH, "nbatches": RB_KEPT // RB_BATCH}
    assert z_var.max() < 5.0
    assert z_mean.max() < 5.0
    assert np.all(var_c < var_x)
    a.close()
    t.close()


def test_statistics_against_the_exact_posterior(hip_device):
    """2D 32^2, the template's posterior and multigrid parameters, 200 warm-up cycles, 20,000 samples, B = 100: the
    Rao-Blackwell mean against Q^-1 B Sigma^-1 y at every vertex within 5 of its own batch-means standard error, the
    Rao-Blackwell variance against (Q^-1)_vv at the 8 probe vertices of
    tests/test_gpu_field_stats.py::test_fields_against_the_exact_posterior within 5 var(c) sqrt(2 tau / n)."""
    op, mp, p = _template_posterior()
    lat = op.get_lattice()
    s = mg.MultigridMCSampler(op, SEED, p)
    exact = ExactTargets(s)
    mean_exact = exact.posterior_mean(_measured_values(mp))
    s.fix_rhs(s.operator_apply(0, mean_exact))
    s.set_state(np.zeros(s.ndof))
    n = 20000
    q = mg.measurement_vector_index(lat, [0.5, 0.5])
    s.sample(200)
    s.field_stats(1, batch=100, conditional=True)
    assert s.field_cond_info()["path"] == "two_pass"
    s.sample(n)
    mean, stderr = s.field_mean_stderr()
    zmean = np.abs(mean - mean_exact) / stderr
    rng = np.random.default_rng(8)
    probes = [q] + [int(v) for v in rng.choice(s.ndof, 7, replace=False)]
    var_exact = np.zeros(s.ndof)
    for v in probes:
        e = np.zeros(s.ndof)
        e[v] = 1.0
        var_exact[v] = exact.solve(e)[v]
    z_var = _z_scores(s, var_exact, mean_exact)[0][probes]
    var_rb = s.field_rb_mean_variance()[1]
    print(f"exact posterior: max z mean {zmean.max():.3f} at vertex {int(zmean.argmax())}, max z variance "
          f"{z_var.max():.3f} over {len(probes)} probes; 1 / d over variance at the probes "
          f"{np.min(1.0 / s.field_conditional_precision()[probes] / var_rb[probes]):.3f} .. "
          f"{np.max(1.0 / s.field_conditional_precision()[probes] / var_rb[probes]):.3f}")
    assert s.field_stats_info()["nrecorded"] == n
    assert np.all(stderr > 0)
    assert np.all(var_rb > 1.0 / s.field_conditional_precision())  # (every vertex, the measured ones included)
    assert zmean.max() < 5.0
    assert z_var.max() < 5.0
    s.close()


def test_driver_rao_blackwell(hip_device, tmp_path, monkeypatch):
    text = open(os.path.join(GOLD, "parameters_template.cfg")).read()
    assert "save_posterior_statistics = true;" in text and "nx = 32;" in text
    text = re.sub(r"nsamples = 10000;", "nsamples = 2000;", text)
    (tmp_path / "parameters.cfg").write_text(text)
    (tmp_path / "measurements_template.cfg").write_text(open(os.path.join(GOLD, "measurements_template.cfg")).read())
    monkeypatch.chdir(tmp_path)
    assert main(["--rao-blackwell", str(tmp_path / "parameters.cfg")]) == 0
    lines = (tmp_path / "posterior.vtk").read_text().split("\n")
    heads = [i for i, ln in enumerate(lines) if ln.startswith("SCALARS ")]
    assert [lines[i].split()[1] for i in heads] == ["mean", "mean_exact", "variance", "variance_conditional"]
    sections = {}
    for i, nxt in zip(heads, heads[1:] + [len(lines) - 1]):
        assert lines[i + 1] == "LOOKUP_TABLE default"
        sections[lines[i].split()[1]] = np.array([float(v) for v in lines[i + 2:nxt]]).reshape(33, 33)
    vc, var = sections["variance_conditional"], sections["variance"]
    inner = (slice(1, 32), slice(1, 32))
    assert np.all(vc[inner] > 0)
    for edge in (vc[0], vc[32], vc[:, 0], vc[:, 32]):
        assert not edge.any()
    # variance = 1 / d + var(c) > 1 / d.  The file holds six digits: at the 8 measured vertices (measurement
    # variances of 1e-6) var(c) d is 2e-6 .. 4e-6 by the dense algebra and the two numbers may print alike; there the
    # file can only show >=.  (The estimates themselves are compared in full precision by
    # test_statistics_against_the_exact_posterior.)
    op, mp, p = _template_posterior()
    measured = np.zeros(31 * 31, dtype=bool)
    measured[op.get_B().rows] = True
    assert measured.sum() == 8
    free = ~measured.reshape(31, 31)
    assert np.all(var[inner][free] > vc[inner][free])
    assert np.all(var[inner] >= vc[inner])
    assert np.all(np.isfinite(sections["mean"]))
