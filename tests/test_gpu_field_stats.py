"""Pointwise field statistics on the device (-m gpu): mgmc_field_stats_* / MultigridMCSampler.field_stats,
the mean and M2 fields of the reference's posterior_statistics (driver_mgmc.cc:118-171).

  * bitwise against a numpy mirror: a second handle with the same seed and chain ids runs the same cycles
    one at a time, its states are folded in float64 with the Welford update the kernel uses (chains in order);
  * bitwise against the QoI moments at the QoI vertex (the moments the exact-statistics tests validate);
  * the chain itself is untouched by the statistics, and unchanged after they are switched off;
  * lifecycle: errors while disabled, enable-on-enabled resets, graph rebuilds keep recording, handles freed;
  * the mean / variance fields of the template's 2D posterior against the exact posterior within 5 sigma;
  * the driver writes posterior.vtk and sample_location.vtk.
"""
import os
import re

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd.driver import ExactTargets, _measured_values, main
from multigridmc_amd.parameters import MeasurementParameters, MultigridParameters, read_config

pytestmark = pytest.mark.gpu

SEED = 5418513
CHAIN0 = 3
GOLD = os.path.join(os.path.dirname(__file__), "golden")


class Mirror:
    """The kernel's update in numpy float64, one state at a time."""

    def __init__(self, ndof):
        self.n = 0
        self.mean = np.zeros(ndof)
        self.m2 = np.zeros(ndof)

    def fold(self, x):
        cnt = float(self.n + 1)
        delta = x - self.mean
        mean = self.mean + delta / cnt
        self.m2 = self.m2 + delta * (x - mean)
        self.mean = mean
        self.n += 1


def _template_posterior(n=32):
    cfg = read_config(os.path.join(GOLD, "parameters_template.cfg"))
    mp = MeasurementParameters.from_config(cfg, GOLD)
    lat = mg.Lattice(n, n)
    op = mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(lat, mg.ConstantCorrelationLengthModel(0.2)), mp)
    return op, mp, MultigridParameters.from_config(cfg)


def _fd(shape, nlevel):
    return mg.ShiftedLaplaceFDOperator(mg.Lattice(*shape), 25.0), mg.MultigridParameters(nlevel=nlevel)


# name -> (operator, parameters, nchains, fixed right-hand side or None)
def _case(name):
    if name == "3d16":
        return _fd((16, 16, 16), 3) + (1, None)
    if name == "3d24x20x12":  # rows no power of two, odd interior row length 23
        return _fd((24, 20, 12), 2) + (1, None)
    if name == "2d48x40":
        return _fd((48, 40), 3) + (1, None)
    if name == "2d32_squared":  # reach-2 layout with its margin offset
        return (mg.SquaredShiftedLaplaceFDOperator(mg.Lattice(32, 32), 25.0), mg.MultigridParameters(nlevel=2), 1, None)
    if name == "3d16_k3":
        return _fd((16, 16, 16), 3) + (3, None)
    if name == "2d32_posterior":  # the template's 8 measurements, f != 0
        op, mp, p = _template_posterior()
        f = np.random.default_rng(11).standard_normal(op.get_ndof())
        return op, p, 1, f
    if name == "3d64":  # hundreds of workgroups, the last one partly beyond the field (one pass per thread at any size)
        return _fd((64, 64, 64), 4) + (1, None)
    raise KeyError(name)


CASES = ["3d16", "3d24x20x12", "2d48x40", "2d32_squared", "3d16_k3", "2d32_posterior", "3d64"]


def _make(name):
    op, p, k, f = _case(name)
    s = mg.MultigridMCSampler(op, SEED, p, device=0, chain_id=CHAIN0, nchains=k)
    if f is not None:
        s.fix_rhs(f)
    return s


def _mirror_cycles(b, mirror, ncycles, cycle0, stride):
    """ncycles single cycles of b, cycle numbers cycle0 + 1 ...; the recorded ones folded, chains in order"""
    for j in range(ncycles):
        b.sample(1)
        if (cycle0 + j + 1) % stride == 0:
            for c in range(b.nchains):
                mirror.fold(b.get_state(c))
    return cycle0 + ncycles


def _assert_equal(a, mirror):
    n, mean, m2 = a.field_moments()
    assert n == mirror.n
    assert a.field_stats_info()["nrecorded"] == mirror.n
    assert np.array_equal(mean, mirror.mean)
    assert np.array_equal(m2, mirror.m2)


@pytest.mark.parametrize("name", CASES)
def test_moments_bitwise_equal_numpy_mirror(hip_device, name):
    a, b = _make(name), _make(name)
    a.field_stats()
    assert a.field_stats_info() == {"enabled": True, "stride": 1, "nrecorded": 0}
    a.sample(10)
    mirror = Mirror(b.ndof)
    _mirror_cycles(b, mirror, 10, 0, 1)
    assert mirror.n == 10 * a.nchains
    assert np.any(mirror.m2 > 0)
    _assert_equal(a, mirror)
    a.close()
    b.close()


def test_stride_three_records_cycles_3_6_9(hip_device):
    a, b = _make("3d16_k3"), _make("3d16_k3")
    a.field_stats(3)
    a.sample(10)
    mirror = Mirror(b.ndof)
    _mirror_cycles(b, mirror, 10, 0, 3)
    assert a.field_stats_info() == {"enabled": True, "stride": 3, "nrecorded": 3 * 3}
    _assert_equal(a, mirror)
    a.close()
    b.close()


def test_cycles_split_over_sample_calls_and_one_apply(hip_device):
    """Every cycle counts, whichever entry point ran it: sample(4), one apply (mgmc_apply: a new right-hand
    side and state, which reset nothing), sample(5)."""
    a, b = _make("3d16"), _make("3d16")
    rng = np.random.default_rng(2)
    f, x0 = rng.standard_normal(a.ndof), rng.standard_normal(a.ndof)
    mirror = Mirror(b.ndof)
    a.field_stats()
    a.sample(4)
    _mirror_cycles(b, mirror, 4, 0, 1)
    xa, xb = x0.copy(), x0.copy()
    a.apply(f, xa)
    b.apply(f, xb)
    assert np.array_equal(xa, xb)
    mirror.fold(xb)
    a.sample(5)
    _mirror_cycles(b, mirror, 5, 5, 1)
    assert mirror.n == 10
    _assert_equal(a, mirror)
    a.close()
    b.close()


def test_unrolled_graph_records_every_cycle(hip_device, monkeypatch):
    """MGMC_GRAPH_UNROLL=4: 10 cycles = two launches of the 4-cycle graph + two single cycles."""
    monkeypatch.setenv("MGMC_GRAPH_UNROLL", "4")
    a = _make("2d48x40")
    monkeypatch.delenv("MGMC_GRAPH_UNROLL")
    b = _make("2d48x40")
    a.field_stats()
    a.sample(10)
    mirror = Mirror(b.ndof)
    _mirror_cycles(b, mirror, 10, 0, 1)
    _assert_equal(a, mirror)
    a.close()
    b.close()


def test_timed_cycles_are_recorded(hip_device):
    a, b = _make("3d16"), _make("3d16")
    a.field_stats()
    a.sample_timed(10)
    mirror = Mirror(b.ndof)
    _mirror_cycles(b, mirror, 10, 0, 1)
    _assert_equal(a, mirror)
    a.close()
    b.close()


def test_moments_at_the_qoi_vertex_equal_qoi_moments(hip_device):
    op, p, _, _ = _case("3d16")
    s = mg.MultigridMCSampler(op, SEED, p)
    q = mg.measurement_vector_index(op.get_lattice(), [0.5, 0.5, 0.5])
    s.sample(20, q)
    s.field_stats(1)
    s.reset_moments()
    s.reset_field_stats()
    s.sample(200, q)
    n, mean, m2 = s.field_moments()
    qm = s.qoi_moments()
    assert n == 200 and qm[0] == 200.0
    assert mean[q] == qm[1] and m2[q] == qm[2]
    assert qm[2] > 0
    s.close()


def test_chain_is_untouched_and_unchanged_after_off(hip_device):
    a, b = _make("3d16"), _make("3d16")
    q = mg.measurement_vector_index(mg.Lattice(16, 16, 16), [0.5, 0.5, 0.5])
    kernels = [a.level_kernels(l) for l in range(a.nlevel)]
    a.field_stats()
    za, zb = a.sample(10, q), b.sample(10, q)
    assert np.array_equal(za, zb)
    assert np.array_equal(a.get_state(), b.get_state())
    a.field_stats_off()
    assert a.field_stats_info() == {"enabled": False, "stride": 0, "nrecorded": 0}
    assert [a.level_kernels(l) for l in range(a.nlevel)] == kernels
    za, zb = a.sample(5, q), b.sample(5, q)
    assert np.array_equal(za, zb)
    assert np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_lifecycle(hip_device):
    live = mg.load_library().mgmc_live_handles()
    s = _make("2d48x40")
    with pytest.raises(mg.MgmcError) as e:
        s.field_moments()
    assert e.value.code == -1
    with pytest.raises(mg.MgmcError) as e:
        s.reset_field_stats()
    assert e.value.code == -1
    with pytest.raises(mg.MgmcError) as e:
        s.field_stats(0)
    assert e.value.code == -1
    s.field_stats_off()  # no-op while disabled
    s.field_stats(2)
    s.sample(6)
    assert s.field_stats_info() == {"enabled": True, "stride": 2, "nrecorded": 3}
    s.field_stats(1)  # on an enabled handle: a reset with the new stride
    n, mean, m2 = s.field_moments()
    assert s.field_stats_info() == {"enabled": True, "stride": 1, "nrecorded": 0}
    assert n == 0 and not mean.any() and not m2.any()
    # reset + n cycles == a fresh enable + n cycles (same chain: a twin handle run the same cycles)
    t = _make("2d48x40")
    t.sample(6)
    s.sample(3)
    t.sample(3)
    s.reset_field_stats()
    t.field_stats()
    s.sample(7)
    t.sample(7)
    ns, means, m2s = s.field_moments()
    nt, meant, m2t = t.field_moments()
    assert ns == nt == 7
    assert np.array_equal(means, meant) and np.array_equal(m2s, m2t)
    with pytest.raises(mg.MgmcError):  # wrong n
        s._chk(s.lib.mgmc_field_stats_get(s.handle, None, None, s.ndof + 1))
    s.close()  # enabled at close: mgmc_destroy frees the fields
    t.close()
    assert mg.load_library().mgmc_live_handles() == live


def test_graph_rebuilds_keep_recording(hip_device):
    """mgmc_set_lowrank and mgmc_set_qoi_vector rebuild the op list / the graphs: the statistics go on."""
    op, mp, p = _template_posterior()
    prior = op.base_operator

    def make():
        return mg.MultigridMCSampler(prior, SEED, p, chain_id=CHAIN0)

    a, b = make(), make()
    rows, vals = mg.measurement_vector(prior.get_lattice(), [0.5, 0.5], 0.1)
    mirror = Mirror(b.ndof)
    a.field_stats()
    a.sample(3)
    cyc = _mirror_cycles(b, mirror, 3, 0, 1)
    for s in (a, b):
        s.set_lowrank(op.get_B())
    a.sample(3)
    cyc = _mirror_cycles(b, mirror, 3, cyc, 1)
    for s in (a, b):
        s.set_qoi_vector(rows, vals)
    a.sample(4, mg.QOI_VECTOR)
    _mirror_cycles(b, mirror, 4, cyc, 1)
    assert a.field_stats_info()["enabled"]
    _assert_equal(a, mirror)
    a.close()
    b.close()


def _iact(z):
    z = z - z.mean()
    var = z.var()
    tau = 1.0
    for t in range(1, len(z) // 10):
        rho = np.dot(z[:-t], z[t:]) / ((len(z) - t) * var)
        if rho < 0.05:
            break
        tau += 2 * rho
    return tau


def test_fields_against_the_exact_posterior(hip_device):
    """2D 32^2, the template's posterior and multigrid parameters, 200 warm-up cycles, 20,000 samples: the
    mean field against Q^-1 B Sigma^-1 y at every vertex, the variance against (Q^-1)_vv at 8 probe
    vertices, within 5 standard errors; the standard error from the field's own variance and the integrated
    autocorrelation time (floored at 1) of the centre-vertex series of the same run."""
    op, mp, p = _template_posterior()
    lat = op.get_lattice()
    s = mg.MultigridMCSampler(op, SEED, p)
    exact = ExactTargets(s)
    mean_exact = exact.posterior_mean(_measured_values(mp))
    s.fix_rhs(s.operator_apply(0, mean_exact))
    s.set_state(np.zeros(s.ndof))
    n = 20000
    q = mg.measurement_vector_index(lat, [0.5, 0.5])
    s.sample(200, q)
    s.field_stats()
    z = s.sample(n, q)
    mean, var = s.field_mean_variance()
    assert s.field_stats_info()["nrecorded"] == n
    tau = max(1.0, _iact(z))
    zmean = np.abs(mean - mean_exact) / np.sqrt(var * tau / n)
    rng = np.random.default_rng(8)
    probes = [q] + [int(v) for v in rng.choice(s.ndof, 7, replace=False)]
    zvar = []
    for v in probes:
        e = np.zeros(s.ndof)
        e[v] = 1.0
        var_exact = exact.solve(e)[v]
        zvar.append(abs(var[v] - var_exact) / (var[v] * np.sqrt(2.0 * tau / n)))
    print(f"field statistics vs exact posterior: n={n} tau(centre)={tau:.3f} max z(mean)={zmean.max():.3f} "
          f"at vertex {int(zmean.argmax())}, max z(variance)={max(zvar):.3f} over {len(probes)} probes")
    assert np.all(var > 0)
    assert zmean.max() < 5.0
    assert max(zvar) < 5.0
    s.close()


def test_driver_writes_posterior_vtk(hip_device, tmp_path, monkeypatch):
    text = open(os.path.join(GOLD, "parameters_template.cfg")).read()
    assert "save_posterior_statistics = true;" in text and "nx = 32;" in text
    text = re.sub(r"nsamples = 10000;", "nsamples = 2000;", text)
    (tmp_path / "parameters.cfg").write_text(text)
    (tmp_path / "measurements_template.cfg").write_text(open(os.path.join(GOLD, "measurements_template.cfg")).read())
    monkeypatch.chdir(tmp_path)
    assert main([str(tmp_path / "parameters.cfg")]) == 0
    assert (tmp_path / "sample_location.vtk").exists()
    lines = (tmp_path / "posterior.vtk").read_text().split("\n")
    assert lines[4] == "DIMENSIONS 33 33 1 " and lines[8] == "POINT_DATA 1089"
    heads = [i for i, ln in enumerate(lines) if ln.startswith("SCALARS ")]
    assert [lines[i] for i in heads] == [f"SCALARS {lb} double 1" for lb in ("mean", "mean_exact", "variance")]
    sections = {}
    for i, nxt in zip(heads, heads[1:] + [len(lines) - 1]):
        assert lines[i + 1] == "LOOKUP_TABLE default"
        sections[lines[i].split()[1]] = lines[i + 2:nxt]
    assert all(len(v) == 33 * 33 for v in sections.values())
    assert lines[-1] == ""
    op, mp, p = _template_posterior()
    s = mg.MultigridMCSampler(op, SEED, p)
    mean_exact = ExactTargets(s).posterior_mean(_measured_values(mp))
    s.close()
    full = np.zeros((33, 33))
    full[1:32, 1:32] = mean_exact.reshape(31, 31)
    assert sections["mean_exact"] == ["%g" % v for v in full.reshape(-1)]
    variance = np.array([float(v) for v in sections["variance"]]).reshape(33, 33)
    assert np.all(variance[1:32, 1:32] > 0) and not variance[0].any() and not variance[:, 0].any()
