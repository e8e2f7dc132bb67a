"""Batch means of the field statistics on the device (-m gpu): mgmc_field_stats_enable_batched /
MultigridMCSampler.field_stats(stride, batch=B), field_mean_stderr, field_iact.

  * bmean and bM2 bitwise against the numpy mirror of tests/test_field_batch_host.py, fed by a twin handle that
    runs the same cycles one at a time (the cases of tests/test_gpu_field_stats.py);
  * mean and M2 bitwise those of a handle without batching;
  * B = 1, a stride with a batch, batches spanning every entry point that runs a cycle and the unrolled graph;
  * a partial batch is dropped by a reset and kept by the graph rebuilds;
  * bitwise against the mirror run on the QoI series alone at the QoI vertex;
  * the chain is untouched; off means off; lifecycle and errors; poisoned LDS; the re-tuned builds;
  * the estimator against the windowed series estimator on a slowly mixing chain, and the mean field of the
    template's 2D posterior against the exact posterior with every vertex's own standard error;
  * the driver's --stderr-batch.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd.driver import ExactTargets, _measured_values, main
from tests.test_field_batch_host import (SLOW_BATCH, SLOW_KAPPA_SQ, SLOW_N, SLOW_SHAPE, SLOW_WARMUP, BatchMirror,
                                         iact_batch_means, iact_windowed, slow_parameters)
from tests.test_gpu_field_stats import CHAIN0, GOLD, SEED, _case, _template_posterior

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["3d16", "3d16_k3", "3d24x20x12", "2d32_squared", "3d64"]
# standard deviation of (batch-means tau - windowed tau) over 20 chain ids of the slow chain on the CPU oracle
# (test_batch_means_tau_agrees_with_the_windowed_estimator_on_the_oracle)
SLOW_TAU_DIFF_SD = 1.79


def make(name):
    op, p, k, f = _case(name)
    s = mg.MultigridMCSampler(op, SEED, p, device=0, chain_id=CHAIN0, nchains=k)
    if f is not None:
        s.fix_rhs(f)
    return s


def mirror_cycles(b, mirror, ncycles, cycle0, stride):
    """ncycles single cycles of b, cycle numbers cycle0 + 1 ...; the recorded ones go to the mirror, chains in order"""
    for j in range(ncycles):
        b.sample(1)
        if (cycle0 + j + 1) % stride == 0:
            mirror.record([b.get_state(c) for c in range(b.nchains)])
    return cycle0 + ncycles


def assert_equal(a, mirror):
    nb, bmean, bm2 = a.field_batch_moments()
    n, mean, m2 = a.field_moments()
    assert a.field_batch_info() == {"batch": mirror.B, "nbatches": mirror.nb}
    assert nb == mirror.nb and n == mirror.n
    assert np.array_equal(bmean, mirror.bmean)
    assert np.array_equal(bm2, mirror.bm2)
    assert np.array_equal(mean, mirror.mean)
    assert np.array_equal(m2, mirror.m2)


@pytest.mark.parametrize("name", CASES)
def test_batch_moments_bitwise_equal_numpy_mirror(hip_device, name):
    """batch 4, 10 cycles: two batches, and the two cycles of the third are in neither field."""
    a, b = make(name), make(name)
    a.field_stats(1, batch=4)
    assert a.field_batch_info() == {"batch": 4, "nbatches": 0}
    a.sample(10)
    mirror = BatchMirror(b.ndof, b.nchains, 4)
    mirror_cycles(b, mirror, 8, 0, 1)
    after8 = (mirror.bmean.copy(), mirror.bm2.copy())
    mirror_cycles(b, mirror, 2, 8, 1)
    assert mirror.nb == 2 and mirror.bsum.any()
    assert np.any(mirror.bm2 > 0)
    assert_equal(a, mirror)
    nb, bmean, bm2 = a.field_batch_moments()
    assert nb == 2 and np.any(bm2 > 0)
    assert np.array_equal(bmean, after8[0]) and np.array_equal(bm2, after8[1])
    a.close()
    b.close()


@pytest.mark.parametrize("name", CASES)
def test_mean_and_m2_are_those_without_batching(hip_device, name):
    a, t = make(name), make(name)
    a.field_stats(1, batch=4)
    t.field_stats(1)
    a.sample(10)
    t.sample(10)
    na, meana, m2a = a.field_moments()
    nt, meant, m2t = t.field_moments()
    assert na == nt == 10 * a.nchains
    assert np.array_equal(meana, meant) and np.array_equal(m2a, m2t)
    assert np.any(m2a > 0)
    assert a.field_stats_info() == t.field_stats_info() == {"enabled": True, "stride": 1, "nrecorded": na}
    a.close()
    t.close()


@pytest.mark.parametrize("name", ["3d16", "3d16_k3"])
def test_batch_of_one_cycle(hip_device, name):
    a, b = make(name), make(name)
    a.field_stats(1, batch=1)
    a.sample(5)
    mirror = BatchMirror(b.ndof, b.nchains, 1)
    mirror_cycles(b, mirror, 5, 0, 1)
    assert mirror.nb == 5 and not mirror.bsum.any()
    assert_equal(a, mirror)
    if a.nchains == 1:  # B = K = 1: the batch fields repeat the Welford fields
        nb, bmean, bm2 = a.field_batch_moments()
        n, mean, m2 = a.field_moments()
        assert np.array_equal(bmean, mean) and np.array_equal(bm2, m2)
    a.close()
    b.close()


def test_stride_three_batch_two(hip_device):
    """13 cycles: recorded cycles 3, 6, 9, 12 give two batches of 2 cycles x 3 chains."""
    a, b = make("3d16_k3"), make("3d16_k3")
    a.field_stats(3, batch=2)
    a.sample(13)
    mirror = BatchMirror(b.ndof, 3, 2)
    mirror_cycles(b, mirror, 13, 0, 3)
    assert mirror.r == 4 and mirror.nb == 2
    assert a.field_stats_info() == {"enabled": True, "stride": 3, "nrecorded": 12}
    assert_equal(a, mirror)
    a.close()
    b.close()


def test_batches_span_every_way_a_cycle_runs(hip_device):
    """batch 4 over sample(3), sample(1) (the batch ends in a single-cycle launch), one apply (cycle 5) and
    sample_timed(5) (the second batch ends in a timed graph)."""
    a, b = make("3d16"), make("3d16")
    rng = np.random.default_rng(2)
    f, x0 = rng.standard_normal(a.ndof), rng.standard_normal(a.ndof)
    mirror = BatchMirror(b.ndof, 1, 4)
    a.field_stats(1, batch=4)
    a.sample(3)
    assert a.field_batch_info()["nbatches"] == 0
    a.sample(1)
    assert a.field_batch_info()["nbatches"] == 1
    mirror_cycles(b, mirror, 4, 0, 1)
    xa, xb = x0.copy(), x0.copy()
    a.apply(f, xa)
    b.apply(f, xb)
    assert np.array_equal(xa, xb)
    mirror.record([xb])
    a.sample_timed(5)
    mirror_cycles(b, mirror, 5, 5, 1)
    assert mirror.r == 10 and mirror.nb == 2
    assert_equal(a, mirror)
    a.close()
    b.close()


def test_batch_ends_inside_an_unrolled_graph(hip_device, monkeypatch):
    """MGMC_GRAPH_UNROLL=4, batch 3: 10 cycles = two launches of the 4-cycle graph + two single cycles; the
    batches end at cycles 3 and 6, inside the graph launches, and at 9."""
    monkeypatch.setenv("MGMC_GRAPH_UNROLL", "4")
    a = make("2d32_squared")
    monkeypatch.delenv("MGMC_GRAPH_UNROLL")
    b = make("2d32_squared")
    a.field_stats(1, batch=3)
    a.sample(10)
    mirror = BatchMirror(b.ndof, 1, 3)
    mirror_cycles(b, mirror, 10, 0, 1)
    assert mirror.nb == 3
    assert_equal(a, mirror)
    a.close()
    b.close()


def test_reset_drops_the_partial_batch(hip_device):
    a, b = make("3d16_k3"), make("3d16_k3")
    a.field_stats(1, batch=4)
    a.sample(6)  # one batch and half of the next
    assert a.field_batch_info() == {"batch": 4, "nbatches": 1}
    a.reset_field_stats()
    assert a.field_batch_info() == {"batch": 4, "nbatches": 0}
    nb, bmean, bm2 = a.field_batch_moments()
    assert nb == 0 and not bmean.any() and not bm2.any()
    a.sample(9)
    b.sample(6)
    mirror = BatchMirror(b.ndof, 3, 4)  # restarted: had the partial sum survived, the next batch mean would differ
    mirror_cycles(b, mirror, 9, 0, 1)
    assert mirror.nb == 2
    assert_equal(a, mirror)
    a.close()
    b.close()


def test_graph_rebuilds_keep_the_partial_batch(hip_device):
    """mgmc_set_lowrank after cycle 3 and mgmc_set_qoi_vector after cycle 6, batch 4: both fall into a batch."""
    op, mp, p = _template_posterior()
    prior = op.base_operator

    def twin():
        return mg.MultigridMCSampler(prior, SEED, p, chain_id=CHAIN0)

    a, b = twin(), twin()
    rows, vals = mg.measurement_vector(prior.get_lattice(), [0.5, 0.5], 0.1)
    mirror = BatchMirror(b.ndof, 1, 4)
    a.field_stats(1, batch=4)
    a.sample(3)
    cyc = mirror_cycles(b, mirror, 3, 0, 1)
    for s in (a, b):
        s.set_lowrank(op.get_B())
    a.sample(3)
    cyc = mirror_cycles(b, mirror, 3, cyc, 1)
    assert a.field_batch_info() == {"batch": 4, "nbatches": 1}
    for s in (a, b):
        s.set_qoi_vector(rows, vals)
    a.sample(4, mg.QOI_VECTOR)
    mirror_cycles(b, mirror, 4, cyc, 1)
    assert mirror.nb == 2 and mirror.bsum.any()
    assert_equal(a, mirror)
    a.close()
    b.close()


def test_rebuild_on_the_posterior_with_a_right_hand_side(hip_device):
    """2d32_posterior (the template's 8 measurements, f != 0): mgmc_set_lowrank again mid-batch."""
    op, _, _, _ = _case("2d32_posterior")
    a, b = make("2d32_posterior"), make("2d32_posterior")
    mirror = BatchMirror(b.ndof, 1, 4)
    a.field_stats(1, batch=4)
    a.sample(2)
    cyc = mirror_cycles(b, mirror, 2, 0, 1)
    for s in (a, b):
        s.set_lowrank(op.get_B())
    a.sample(7)
    mirror_cycles(b, mirror, 7, cyc, 1)
    assert mirror.nb == 2
    assert_equal(a, mirror)
    a.close()
    b.close()


def test_batch_moments_at_the_qoi_vertex_equal_the_mirror_on_the_series(hip_device):
    op, p, _, _ = _case("3d16")
    s = mg.MultigridMCSampler(op, SEED, p)
    q = mg.measurement_vector_index(op.get_lattice(), [0.5, 0.5, 0.5])
    s.sample(20, q)
    s.field_stats(1, batch=8)
    z = s.sample(50, q)
    mirror = BatchMirror(1, 1, 8)
    for v in z:
        mirror.record([np.array([v])])
    nb, bmean, bm2 = s.field_batch_moments()
    n, mean, m2 = s.field_moments()
    assert nb == mirror.nb == 6 and n == 50
    assert bmean[q] == mirror.bmean[0] and bm2[q] == mirror.bm2[0]
    assert mean[q] == mirror.mean[0] and m2[q] == mirror.m2[0]
    assert bm2[q] > 0
    s.close()


def test_chain_is_untouched_and_off_means_off(hip_device):
    a, b = make("3d16"), make("3d16")
    q = mg.measurement_vector_index(mg.Lattice(16, 16, 16), [0.5, 0.5, 0.5])
    kernels = [a.level_kernels(l) for l in range(a.nlevel)]
    a.field_stats(1, batch=4)
    za, zb = a.sample(10, q), b.sample(10, q)
    assert np.array_equal(za, zb)
    assert np.array_equal(a.get_state(), b.get_state())
    a.field_stats_off()
    assert a.field_stats_info() == {"enabled": False, "stride": 0, "nrecorded": 0}
    assert a.field_batch_info() == {"batch": 0, "nbatches": 0}
    assert [a.level_kernels(l) for l in range(a.nlevel)] == kernels
    za, zb = a.sample(5, q), b.sample(5, q)
    assert np.array_equal(za, zb)
    assert np.array_equal(a.get_state(), b.get_state())
    a.field_stats(1)  # without batching: no batch fields
    a.sample(4)
    assert a.field_batch_info()["batch"] == 0
    with pytest.raises(mg.MgmcError) as e:
        a.field_batch_moments()
    assert e.value.code == -1 and "batch" in str(e.value)
    with pytest.raises(mg.MgmcError):
        a.field_mean_stderr()
    a.close()
    b.close()


def test_lifecycle_and_errors(hip_device):
    live = mg.load_library().mgmc_live_handles()
    s = make("3d16")
    with pytest.raises(mg.MgmcError) as e:  # while off
        s.field_batch_moments()
    assert e.value.code == -1 and "batch means are not enabled" in str(e.value)
    for stride, batch, text in ((1, 0, "batch must be >= 1"), (1, -3, "batch must be >= 1"), (0, 2, "stride must be >= 1")):
        with pytest.raises(mg.MgmcError) as e:
            s.field_stats(stride, batch=batch)
        assert e.value.code == -1 and text in str(e.value)
    assert s.field_stats_info()["enabled"] is False and s.field_batch_info() == {"batch": 0, "nbatches": 0}
    s.field_stats(1)
    s.sample(6)
    s.field_stats(2, batch=3)  # on a plain-enabled handle: a reset with both parameters
    assert s.field_stats_info() == {"enabled": True, "stride": 2, "nrecorded": 0}
    assert s.field_batch_info() == {"batch": 3, "nbatches": 0}
    n, mean, m2 = s.field_moments()
    nb, bmean, bm2 = s.field_batch_moments()
    assert n == 0 and nb == 0 and not any(v.any() for v in (mean, m2, bmean, bm2))
    with pytest.raises(mg.MgmcError) as e:  # wrong n
        s._chk(s.lib.mgmc_field_stats_get_batch(s.handle, None, None, s.ndof + 1))
    assert e.value.code == -1 and "size mismatch" in str(e.value)
    s._chk(s.lib.mgmc_field_stats_get_batch(s.handle, None, None, s.ndof))  # either pointer may be NULL
    s.sample(9)  # recorded cycles 2, 4, 6, 8: one batch and a partial sum
    assert s.field_batch_info() == {"batch": 3, "nbatches": 1}
    with pytest.raises(ValueError):  # fewer than two batches
        s.field_mean_stderr()
    with pytest.raises(ValueError):
        s.field_iact()
    s.field_stats(1, batch=2)  # on a batched handle: a reset with both; then as a fresh enable on a twin
    assert s.field_stats_info() == {"enabled": True, "stride": 1, "nrecorded": 0}
    assert s.field_batch_info() == {"batch": 2, "nbatches": 0}
    t = make("3d16")
    t.sample(15)
    t.field_stats(1, batch=2)
    s.sample(5)
    t.sample(5)
    for got, want in zip(s.field_batch_moments() + s.field_moments(), t.field_batch_moments() + t.field_moments()):
        assert np.array_equal(got, want)
    mean, stderr = s.field_mean_stderr()
    assert np.all(stderr > 0) and np.all(s.field_iact() > 0)
    s.field_stats(1)  # back to the statistics without batching
    assert s.field_batch_info() == {"batch": 0, "nbatches": 0}
    s.sample(3)
    assert s.field_stats_info() == {"enabled": True, "stride": 1, "nrecorded": 3}
    s.field_stats(1, batch=2)
    s.close()  # batched at close: mgmc_destroy frees the five fields
    t.close()
    assert mg.load_library().mgmc_live_handles() == live


def test_poisoned_lds(hip_device, monkeypatch):
    monkeypatch.setenv("MGMC_POISON", "1")
    a = make("3d64")
    monkeypatch.delenv("MGMC_POISON")
    b = make("3d64")
    a.field_stats(1, batch=4)
    a.sample(10)
    mirror = BatchMirror(b.ndof, 1, 4)
    mirror_cycles(b, mirror, 10, 0, 1)
    assert mirror.nb == 2
    assert_equal(a, mirror)
    a.close()
    b.close()


def test_retuned_builds(hip_device):
    """The bitwise case on 3d64 through build/libmgmc_tune_lo.so (FS_NT 128, FS_PAIRS 2) and _hi.so (FS_NT 512),
    each in a child process; the second is not started if the first died."""
    libs = [os.path.join(ROOT, "build", f"libmgmc_tune_{name}.so") for name in ("lo", "hi")]
    if not all(os.path.exists(p) for p in libs):
        pytest.skip("the re-tuned libraries build/libmgmc_tune_lo.so and _hi.so are not built (__graft_entry__.build())")
    env = dict(os.environ)
    for key in ("MGMC_DISABLE", "MGMC_POISON", "MGMC_LIBRARY", "MGMC_GRAPH_UNROLL"):
        env.pop(key, None)
    for path in libs:
        proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "field_batch_worker.py"), path, "3d64", "4",
                               "10"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert proc.returncode == 0, f"{path}: exit status {proc.returncode}: {proc.stdout[-300:]} {proc.stderr[-600:]}"
        out = json.loads(proc.stdout.strip().splitlines()[-1])
        assert out["library"] == path
        assert out["ok"] and out["nb"] == 2, out


def test_statistics_tau_against_the_series_and_the_exact_posterior(hip_device):
    """(a) The slow chain of tests/test_field_batch_host.py (2D 12 x 12, kappa^2 = 1, one level; 200 warm-up cycles,
    20,000 samples, B = 250): the device's batch-means tau at the QoI vertex against the windowed estimator on the
    same device series, within 5 x 1.79 = 8.95 (1.79: the standard deviation of that difference over 20 chain ids on
    the CPU oracle; on the oracle the mean of the difference is +0.59 and the windowed tau 9.23 on average).
    Measured on the device: batch-means tau 9.077 (the mirror on the series gives the same), windowed tau 9.430,
    difference -0.35; tau over the 121 vertices of this lattice 1.43 .. 12.66.
    (b) 2D 32^2, the template's posterior (test_fields_against_the_exact_posterior), 200 warm-up + 20,000 samples,
    B = 100: z-scores of the mean field against the exact posterior mean with each vertex's own batch-means standard
    error; the largest |z| over the 961 vertices is at most 5.  Measured: largest |z| 3.02 (vertex 652), RMS z 0.98;
    tau over the 961 vertices 0.84 .. 2.81, median 1.28, largest at vertex 793."""
    # (a)
    lat = mg.Lattice(*SLOW_SHAPE)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, SLOW_KAPPA_SQ), SEED, slow_parameters())
    q = mg.measurement_vector_index(lat, [0.5, 0.5])
    s.sample(SLOW_WARMUP, q)
    s.field_stats(1, batch=SLOW_BATCH)
    z = s.sample(SLOW_N, q)
    tau_field = s.field_iact()
    assert s.field_batch_info() == {"batch": SLOW_BATCH, "nbatches": SLOW_N // SLOW_BATCH}
    s.close()
    tau_b, tau_w, tau_mirror = float(tau_field[q]), iact_windowed(z), iact_batch_means(z, SLOW_BATCH)
    print(f"slow chain: batch-means tau {tau_b:.3f} (mirror on the series {tau_mirror:.3f}), windowed tau {tau_w:.3f}, "
          f"difference {tau_b - tau_w:+.3f} (bound {5 * SLOW_TAU_DIFF_SD:.2f}); tau over the field "
          f"{tau_field.min():.2f} .. {tau_field.max():.2f}")
    # (b)
    op, mp, p = _template_posterior()
    s = mg.MultigridMCSampler(op, SEED, p)
    mean_exact = ExactTargets(s).posterior_mean(_measured_values(mp))
    s.fix_rhs(s.operator_apply(0, mean_exact))
    s.set_state(np.zeros(s.ndof))
    n, batch = 20000, 100
    s.sample(200)
    s.field_stats(1, batch=batch)
    s.sample(n)
    mean, stderr = s.field_mean_stderr()
    tau = s.field_iact()
    assert s.field_batch_info() == {"batch": batch, "nbatches": n // batch}
    s.close()
    zmean = np.abs(mean - mean_exact) / stderr
    print(f"exact posterior: max |z| {zmean.max():.3f} at vertex {int(zmean.argmax())}, rms z "
          f"{np.sqrt(np.mean(zmean ** 2)):.3f}; tau over the 961 vertices {tau.min():.3f} .. {tau.max():.3f} "
          f"(median {np.median(tau):.3f}, largest at vertex {int(tau.argmax())})")
    assert tau_b == pytest.approx(tau_mirror, rel=1e-12)
    assert tau_w >= 5.0
    assert abs(tau_b - tau_w) <= 5 * SLOW_TAU_DIFF_SD
    assert mean.shape == (961,) and np.all(stderr > 0) and np.all(np.isfinite(tau))
    assert zmean.max() <= 5.0


def _run_driver(tmp_path, monkeypatch, args):
    text = open(os.path.join(GOLD, "parameters_template.cfg")).read()
    assert "save_posterior_statistics = true;" in text and "nx = 32;" in text
    text = re.sub(r"nsamples = 10000;", "nsamples = 1000;", text)
    tmp_path.mkdir(exist_ok=True)
    (tmp_path / "parameters.cfg").write_text(text)
    (tmp_path / "measurements_template.cfg").write_text(open(os.path.join(GOLD, "measurements_template.cfg")).read())
    monkeypatch.chdir(tmp_path)
    assert main(args + [str(tmp_path / "parameters.cfg")]) == 0
    lines = (tmp_path / "posterior.vtk").read_text().split("\n")
    heads = [i for i, ln in enumerate(lines) if ln.startswith("SCALARS ")]
    sections = {}
    for i, nxt in zip(heads, heads[1:] + [len(lines) - 1]):
        assert lines[i + 1] == "LOOKUP_TABLE default"
        sections[lines[i].split()[1]] = np.array([float(v) for v in lines[i + 2:nxt]])
    assert all(len(v) == 33 * 33 for v in sections.values())
    return [lines[i].split()[1] for i in heads], sections


def test_driver_stderr_batch(hip_device, tmp_path, monkeypatch):
    labels, sections = _run_driver(tmp_path / "with", monkeypatch, ["--stderr-batch", "10"])
    assert labels == ["iact", "mean", "mean_exact", "mean_stderr", "variance"]
    for label in ("mean_stderr", "iact"):
        v = sections[label].reshape(33, 33)
        assert np.all(np.isfinite(v)) and np.all(v[1:32, 1:32] > 0)
        assert not v[0].any() and not v[:, 0].any() and not v[32].any() and not v[:, 32].any()
    # stderr^2 = variance tau / n, up to the vtk file's six digits and the n / (n - 1) of the sample variance
    n = 1000
    inner = (slice(1, 32), slice(1, 32))
    lhs = sections["mean_stderr"].reshape(33, 33)[inner] ** 2
    rhs = sections["variance"].reshape(33, 33)[inner] * sections["iact"].reshape(33, 33)[inner] / n
    assert np.allclose(lhs, rhs, rtol=2e-3)
    labels, plain = _run_driver(tmp_path / "without", monkeypatch, [])
    assert labels == ["mean", "mean_exact", "variance"]
    for label in labels:  # the same chain: the option changes nothing else
        assert np.array_equal(plain[label], sections[label])
