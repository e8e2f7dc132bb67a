"""Whole-field energy on the device (-m gpu): mgmc_energy / mgmc_energy_record_* (mgmc_energy.hpp), per chain
xqx = x^T A x + sum_k (B_k^T x)^2 / Sigma_k and fx = f^T x of the level-0 state.

Recorded values against the longdouble reference of tests/energy_ref.py, from the operator's own matrix, low-rank
part and right-hand side: handle A records with stride 1 over 6 cycles, handle B (same seed and chains) steps one
cycle at a time and hands each state to the helper.  Per record |xqx - xqx_ref| <= 2 n u S and |fx - fx_ref| <=
2 N u T, u = 2^-53, n = nnz(A) + 2 nnz(B) + N + 4 m: the bound of any summation order of that many rounded terms,
doubled (about 5e-11 relative to S at these sizes; one dropped coupling at one vertex is about 1e-6).  Largest
|error| / bound observed per case over the 6 records on an MI355X (xqx, fx; 0: equal to the rounded reference):
    z64x22x10 1.9e-06, 0          z128x34x18 0, 0              z192x48x40 7.7e-08, 0      z64x12x130 3.1e-07, 0
    z64x22x10_f 0, 5.2e-05        vd64x22x10 1.8e-06, 0        vd128x34x18 3.2e-07, 0     z64x48x48_lowrank 1.1e-07, 3.2e-06
    g24x20x12 1.0e-05, 0          g2d48x40 1.5e-05, 0          g2d32_squared 0, 0         gfem16 4.5e-06, 0
    gperiodic32x16x16 4.4e-06, 0  g2d32_posterior 3.1e-05, 4.2e-04                        g32_ball_global 0, 0
(the tree-shaped reduction leaves an ulp or two, the bound allows n of them).
Identities bit for bit (repeatability, energy() against the last record, MGMC_GRAPH_UNROLL, stride, Welford
moments, capacity, MGMC_POISON), the forced general kernel against the z-march, the chain untouched by the
recording, the lifecycle, batched chains against one-chain handles, and the chi-square identity on the device.
"""
import os
import re

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd import _native
from multigridmc_amd.driver import main
from multigridmc_amd.parameters import MeasurementParameters, MultigridParameters, read_config
from tests import energy_ref as ER
from tests.test_energy_host import CHI_CHAIN, CHI_DISCARD, chi_operator

pytestmark = pytest.mark.gpu

SEED = 5418513
CHAIN0 = 3
GOLD = os.path.join(os.path.dirname(__file__), "golden")
PERIODIC = mg.PeriodicCorrelationLengthModel(0.2, 0.4)

def _fd(shape, nlevel):
    return mg.ShiftedLaplaceFDOperator(mg.Lattice(*shape), 25.0), mg.MultigridParameters(nlevel=nlevel)


def _measured(base, radius, nmeas, glob, seed=1212417):
    rng = np.random.default_rng(seed)
    dim = base.get_lattice().dim
    mp = MeasurementParameters(radius=radius, variance_scaling=1e-3, measure_global=glob, variance_global=0.02)
    mp.measurement_locations = [list(rng.uniform(0.15, 0.85, dim)) for _ in range(nmeas)]
    mp.variance = list(1.0 + 2.0 * rng.random(nmeas))
    return mg.MeasuredOperator(base, mp)


def _rhs(op, seed=11):
    return np.random.default_rng(seed).standard_normal(op.get_ndof())


# name -> (operator, parameters, right-hand side or None)
def _case(name):
    if name == "z64x22x10":  # one x tile, a partial y tile
        return _fd((64, 22, 10), 2) + (None,)
    if name == "z128x34x18":
        return _fd((128, 34, 18), 2) + (None,)
    if name == "z192x48x40":
        return _fd((192, 48, 40), 3) + (None,)
    if name == "z64x12x130":  # more planes than any z chunk
        return _fd((64, 12, 130), 2) + (None,)
    if name == "z64x22x10_f":
        op, p = _fd((64, 22, 10), 2)
        return op, p, _rhs(op)
    if name == "vd64x22x10":  # variable diagonal: the periodic-kappa FD operator through the matrix path
        return mg.ShiftedLaplaceFDOperator(mg.Lattice(64, 22, 10), PERIODIC), mg.MultigridParameters(nlevel=2), None
    if name == "vd128x34x18":
        return mg.ShiftedLaplaceFDOperator(mg.Lattice(128, 34, 18), PERIODIC), mg.MultigridParameters(nlevel=2), None
    if name == "z64x48x48_lowrank":  # 4 point measurements, f != 0
        op = _measured(_fd((64, 48, 48), 3)[0], 0.0, 4, False)
        return op, mg.MultigridParameters(nlevel=3), _rhs(op)
    if name == "g24x20x12":
        return _fd((24, 20, 12), 2) + (None,)
    if name == "g2d48x40":
        return _fd((48, 40), 3) + (None,)
    if name == "g2d32_squared":  # reach 2
        return mg.SquaredShiftedLaplaceFDOperator(mg.Lattice(32, 32), 25.0), mg.MultigridParameters(nlevel=2), None
    if name == "gfem16":
        return mg.ShiftedLaplaceFEMOperator(mg.Lattice(16, 16, 16), 25.0), mg.MultigridParameters(nlevel=3), None
    if name == "gperiodic32x16x16":  # a 3D field level
        return mg.ShiftedLaplaceFDOperator(mg.Lattice(32, 16, 16), PERIODIC), mg.MultigridParameters(nlevel=2), None
    if name == "g2d32_posterior":  # the template's 8 measurements, f != 0
        cfg = read_config(os.path.join(GOLD, "parameters_template.cfg"))
        mp = MeasurementParameters.from_config(cfg, GOLD)
        lat = mg.Lattice(32, 32)
        op = mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(lat, mg.ConstantCorrelationLengthModel(0.2)), mp)
        return op, MultigridParameters.from_config(cfg), _rhs(op)
    if name == "g32_ball_global":  # ball averages + the global average (a dense column)
        return _measured(_fd((32, 32, 32), 3)[0], 0.1, 2, True), mg.MultigridParameters(nlevel=3), None
    raise KeyError(name)


ZMARCH = ["z64x22x10", "z128x34x18", "z192x48x40", "z64x12x130", "z64x22x10_f", "vd64x22x10", "vd128x34x18",
          "z64x48x48_lowrank"]
GENERAL = ["g24x20x12", "g2d48x40", "g2d32_squared", "gfem16", "gperiodic32x16x16", "g2d32_posterior",
           "g32_ball_global"]


def _make(name, chain=CHAIN0, nchains=1):
    op, p, f = _case(name)
    s = mg.MultigridMCSampler(op, SEED, p, device=0, chain_id=chain, nchains=nchains)
    if f is not None:
        s.fix_rhs(f)
    return s, op, f


@pytest.mark.parametrize("name", ZMARCH + GENERAL)
def test_records_within_the_bound_of_the_reference(hip_device, name):
    (a, op, f), (b, _, _) = _make(name), _make(name)
    if name.startswith(("z", "vd")):
        assert a.level_kernels(0)["sweep"].startswith("k_zsweep"), a.level_kernels(0)
    else:
        assert not a.level_kernels(0)["sweep"].startswith("k_zsweep"), a.level_kernels(0)
    a.energy_record(1, 16)
    assert a.energy_record_info() == {"enabled": True, "stride": 1, "ncycles": 0, "nrecorded": 0}
    a.sample(6)
    assert a.energy_record_info() == {"enabled": True, "stride": 1, "ncycles": 6, "nrecorded": 6}
    q, g = a.energy_series()
    assert q.shape == g.shape == (6,)
    worst = [0.0, 0.0]
    for t in range(6):
        b.sample(1)
        ref = ER.reference(op, f, b.get_state())
        ok, rq, rf = ER.within_bound(q[t], g[t], ref)
        worst = [max(worst[0], rq), max(worst[1], rf)]
        assert ok, (name, t, q[t], g[t], ref, rq, rf)
        assert ref[2] > 0 and q[t] > 0
        if f is None:
            assert g[t] == 0.0 and np.signbit(g[t]) == False  # noqa: E712  (+0.0 while f is zero)
    print(f"energy ratio {name}: xqx {worst[0]:.1e} fx {worst[1]:.1e} (relative bound {2 * ref[4] * ER.U:.2e})")
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["z64x22x10", "g2d48x40"])
def test_batched_chains_equal_one_chain_handles(hip_device, name):
    a, _, _ = _make(name, nchains=3)
    a.energy_record(1, 8)
    a.sample(4)
    now = a.energy()
    for c in range(3):
        s, _, _ = _make(name, chain=CHAIN0 + c)
        s.energy_record(1, 8)
        s.sample(4)
        for u, v in zip(a.energy_series(c), s.energy_series(0)):
            assert np.array_equal(u, v), (name, c)
        assert np.array_equal(a.energy_moments(c), s.energy_moments(0))
        assert a.energy(chain=c) == s.energy(chain=0) == (now[0][c], now[1][c])
        s.close()
    a.close()


@pytest.mark.parametrize("name", ["z64x22x10_f", "g2d32_posterior", "z64x48x48_lowrank"])
def test_energy_repeats_and_equals_the_last_record(hip_device, name):
    a, _, _ = _make(name)
    a.energy_record(1, 8)
    a.sample(5)
    e1, e2 = a.energy(), a.energy()
    assert np.array_equal(e1[0], e2[0]) and np.array_equal(e1[1], e2[1])
    q, g = a.energy_series()
    assert (q[-1], g[-1]) == (e1[0][0], e1[1][0]) == a.energy(chain=0)
    assert a.energy_record_info()["nrecorded"] == 5  # energy() records nothing
    a.close()


@pytest.mark.parametrize("name", ["z64x22x10", "g24x20x12"])
def test_graph_unroll_one_gives_the_same_series(hip_device, name, monkeypatch):
    a, _, _ = _make(name)
    monkeypatch.setenv("MGMC_GRAPH_UNROLL", "1")
    b, _, _ = _make(name)
    monkeypatch.delenv("MGMC_GRAPH_UNROLL")
    for s in (a, b):
        s.energy_record(1, 16)
        s.sample(11)
    for u, v in zip(a.energy_series(), b.energy_series()):
        assert np.array_equal(u, v)
    a.close()
    b.close()


def test_stride_three_records_cycles_3_6_9(hip_device):
    (a, _, _), (b, _, _) = _make("z64x22x10_f"), _make("z64x22x10_f")
    a.energy_record(3, 16)
    b.energy_record(1, 16)
    a.sample(10)
    b.sample(10)
    assert a.energy_record_info() == {"enabled": True, "stride": 3, "ncycles": 10, "nrecorded": 3}
    for u, v in zip(a.energy_series(), b.energy_series()):
        assert np.array_equal(u, v[[2, 5, 8]])
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["z64x22x10_f", "g2d32_posterior"])
def test_moments_equal_a_numpy_welford_mirror(hip_device, name):
    a, _, _ = _make(name, nchains=2)
    a.energy_record(1, 16)
    a.sample(9)
    for c in range(2):
        q, g = a.energy_series(c)
        assert np.array_equal(a.energy_moments(c), ER.welford(q - 2.0 * g))
    a.close()


def test_capacity_keeps_the_first_records_and_the_moments_count_on(hip_device):
    (a, _, _), (b, _, _) = _make("g2d48x40"), _make("g2d48x40")
    a.energy_record(1, 4)
    b.energy_record(1, 16)
    a.sample(6)
    b.sample(6)
    assert a.energy_record_info()["nrecorded"] == 6
    qa, ga = a.energy_series()
    qb, gb = b.energy_series()
    assert len(qa) == 4 and np.array_equal(qa, qb[:4]) and np.array_equal(ga, gb[:4])
    assert a.energy_moments()[0] == 6.0 and np.array_equal(a.energy_moments(), b.energy_moments())
    a.close()
    b.close()


@pytest.mark.parametrize("name", ["z64x22x10_f", "g2d32_posterior"])
def test_poisoned_scratch_and_lds_give_the_same_bits(hip_device, name, monkeypatch):
    a, _, _ = _make(name)
    monkeypatch.setenv("MGMC_POISON", "1")
    b, _, _ = _make(name)
    monkeypatch.delenv("MGMC_POISON")
    for s in (a, b):
        s.energy_record(1, 8)
        s.sample(4)
    for u, v in zip(a.energy_series(), b.energy_series()):
        assert np.array_equal(u, v)
    ea, eb = a.energy(general=True), b.energy(general=True)
    assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
    a.close()
    b.close()


@pytest.mark.parametrize("name", ZMARCH)
def test_forced_general_kernel_against_the_z_march(hip_device, name):
    a, op, f = _make(name)
    a.sample(3)
    ref = ER.reference(op, f, a.get_state())
    z, g = a.energy(chain=0), a.energy(chain=0, general=True)
    okz, rz, _ = ER.within_bound(z[0], z[1], ref)
    okg, rg, _ = ER.within_bound(g[0], g[1], ref)
    assert okz and okg, (name, z, g, ref, rz, rg)
    a.close()


@pytest.mark.parametrize("name", ["z64x22x10_f", "g2d32_posterior"])
def test_the_chain_is_untouched(hip_device, name):
    (a, _, _), (b, _, _) = _make(name), _make(name)
    kernels = [b.level_kernels(l) for l in range(b.nlevel)]
    qoi = a.ndof // 2
    a.energy_record(2, 8)
    za, zb = a.sample(7, qoi), b.sample(7, qoi)
    assert np.array_equal(za, zb) and np.array_equal(a.get_state(), b.get_state())
    assert a.get_sample_index() == b.get_sample_index() == 7
    a.energy_record_off()
    assert a.energy_record_info() == {"enabled": False, "stride": 0, "ncycles": 0, "nrecorded": 0}
    assert [a.level_kernels(l) for l in range(a.nlevel)] == kernels
    assert np.array_equal(a.sample(3, qoi), b.sample(3, qoi)) and np.array_equal(a.get_state(), b.get_state())
    a.close()
    b.close()


def _invalid(call):
    with pytest.raises(_native.MgmcError) as e:
        call()
    assert e.value.code == _native.MGMC_E_INVALID


def test_lifecycle(hip_device):
    lib = mg.load_library()
    live0 = lib.mgmc_live_handles()
    a, op, _ = _make("z64x22x10")
    assert lib.mgmc_live_handles() == live0 + 1
    _invalid(lambda: a.energy_record(0, 4))
    _invalid(lambda: a.energy_record(1, 0))
    _invalid(a.reset_energy_record)
    _invalid(lambda: a.energy_moments())
    _invalid(lambda: a._chk(lib.mgmc_energy_get_series(a.handle, 0, None, None, 0)))
    _invalid(lambda: a._chk(lib.mgmc_energy(a.handle, 0, None, None)))
    a.energy_record_off()  # a no-op while disabled
    a.energy_record(1, 8)
    _invalid(lambda: a.energy_moments(1))
    a.sample(3)
    _invalid(lambda: a._chk(lib.mgmc_energy_get_series(a.handle, 0, None, None, 4)))
    # enable on an enabled handle resets (another stride, then another capacity)
    a.energy_record(2, 8)
    assert a.energy_record_info() == {"enabled": True, "stride": 2, "ncycles": 0, "nrecorded": 0}
    assert a.energy_moments()[0] == 0.0
    a.sample(2)
    a.energy_record(1, 12)
    assert a.energy_record_info() == {"enabled": True, "stride": 1, "ncycles": 0, "nrecorded": 0}
    a.sample(2)
    a.reset_energy_record()
    assert a.energy_record_info() == {"enabled": True, "stride": 1, "ncycles": 0, "nrecorded": 0}
    # graph rebuilds keep it recording; set_state / set_sample_index reset nothing; fx follows set_rhs
    f = _rhs(op, 5)
    states, refs = [], []

    def step(ref_op, rhs):
        a.sample(1)
        states.append(a.get_state())
        refs.append(ER.reference(ref_op, rhs, states[-1]))

    step(op, None)
    a.set_qoi_vector(np.array([0, 5, 9]), np.array([1.0, 2.0, 3.0]))
    step(op, None)
    a.fix_rhs(f)  # zero -> non-zero
    step(op, f)
    a.set_state(np.zeros(a.ndof))
    a.set_sample_index(40)
    step(op, f)
    measured = _measured(op, 0.0, 3, False)
    a.set_lowrank(measured.get_B())
    step(measured, f)
    a.fix_rhs(np.zeros(a.ndof))  # and back
    step(measured, None)
    assert a.energy_record_info() == {"enabled": True, "stride": 1, "ncycles": 6, "nrecorded": 6}
    q, g = a.energy_series()
    for t, ref in enumerate(refs):
        assert ER.within_bound(q[t], g[t], ref)[0], (t, q[t], g[t], ref)
    assert g[0] == g[1] == g[5] == 0.0 and g[2] != 0.0 and g[3] != 0.0 and g[4] != 0.0
    # (the low-rank term is in the record after set_lowrank: the prior's reference no longer fits)
    assert not ER.within_bound(q[4], g[4], ER.reference(op, f, states[4]))[0]
    a.close()
    assert lib.mgmc_live_handles() == live0


def test_chi_square_on_the_device(hip_device):
    """64 x 36 x 20 (N = 41,895), 3 levels, seed 5418513, chain 3, 100 cycles discarded, 1,100 recorded:
    |mean - N| <= 5 sqrt(2 N tau / 1100) with tau = 1.157, iact_windowed of the MULTICOLOUR oracle's series
    (tests/test_energy_host.py::test_chi_square_identity_on_the_oracle prints it; the oracle chain's own mean
    over these 1,100 cycles is 41,886.4, well inside).  A noise scale wrong by 1 % in one kernel moves the mean by about 2 % of
    N, some 90 of these standard errors."""
    tau, kept = 1.157, 1100
    op, p = chi_operator()
    s = mg.MultigridMCSampler(op, SEED, p, device=0, chain_id=CHI_CHAIN)
    s.sample(CHI_DISCARD)
    s.energy_record(1, kept)
    s.sample(kept)
    q, g = s.energy_series()
    n, mean, m2 = s.energy_moments()
    N = s.ndof
    assert n == kept and len(q) == kept and N == 41895 and not np.any(g)
    assert abs(mean - q.mean()) <= 1e-9 * N
    sigma = np.sqrt(2.0 * N * tau / kept)
    print(f"device chi-square: mean {mean:.1f}, N {N}, z {(mean - N) / sigma:+.2f}, tau(device series) "
          f"{ER.iact_windowed(q):.3f}, var / 2N {m2 / kept / (2 * N):.3f}")
    assert abs(mean - N) <= 5.0 * sigma
    s.close()


def test_driver_energy_stride(hip_device, tmp_path, monkeypatch, capsys):
    """--energy-stride 4 on the template's 2D posterior (f != 0): energy_multigridmc.txt holds (cycle, xqx, fx) of
    every 4th of the 2,000 samples, and the printed mean of E = xqx - 2 fx + f^T Q^-1 f lies within 5 of its
    standard errors of N = 961 (the z-score the driver prints, with its own tau)."""
    text = open(os.path.join(GOLD, "parameters_template.cfg")).read()
    text = re.sub(r"nsamples = 10000;", "nsamples = 2000;", text)
    text = re.sub(r"nsamples = 1000;", "nsamples = 20;", text)
    text = re.sub(r"save_posterior_statistics = true;", "save_posterior_statistics = false;", text)
    (tmp_path / "parameters.cfg").write_text(text)
    (tmp_path / "measurements_template.cfg").write_text(open(os.path.join(GOLD, "measurements_template.cfg")).read())
    monkeypatch.chdir(tmp_path)
    assert main(["--energy-stride", "4", str(tmp_path / "parameters.cfg")]) == 0
    rows = np.loadtxt(tmp_path / "energy_multigridmc.txt")
    assert rows.shape == (500, 3) and np.array_equal(rows[:, 0], 4.0 * np.arange(1, 501))
    assert np.all(rows[:, 1] > 0) and np.any(rows[:, 2] != 0)
    out = capsys.readouterr().out
    m = re.search(r"chi-square N\s+=\s+(\d+)\s+z-score = ([-+][0-9.]+)", out)
    assert m, out
    assert int(m.group(1)) == 961 and abs(float(m.group(2))) <= 5.0
    e = re.search(r"MGMC energy\s+=\s+([0-9.e+-]+) over 500 records", out)
    assert e and abs(float(e.group(1)) - 961) < 0.1 * 961
