"""bench.py --dump-outputs / --full: the files a run writes are what the timed path left with its
caller (state, QoI series, QoI moments), a plain run leaves the CPU baseline out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeSampler:
    """Host stand-in for dump_outputs: chain c's state is c + arange(ndof), its series c + arange(steps)."""

    def __init__(self, nchains, ndof):
        self.nchains, self.ndof = nchains, ndof

    def get_state(self, chain=0):
        return chain + np.arange(self.ndof, dtype=np.float64)

    def get_series(self, n, chain=0):
        return chain + np.arange(n, dtype=np.float64)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """A state within its share is written whole; a longer one at the same seeded, ascending vertices
    for every chain and every run; the series keeps the last steps that fit; all float64."""
    import bench
    mom = np.array([[5.0, 0.1, 1.0], [5.0, 0.2, 2.0]])
    bench.dump_outputs(str(tmp_path / "a"), _FakeSampler(2, 1000), 5, mom)
    st = np.load(tmp_path / "a" / "state.npy")
    assert st.dtype == np.float64 and st.shape == (2, 1000)
    assert np.array_equal(st[1], 1 + np.arange(1000.0))
    assert np.array_equal(np.load(tmp_path / "a" / "qoi_series.npy"), [[0, 1, 2, 3, 4], [1, 2, 3, 4, 5]])
    assert np.array_equal(np.load(tmp_path / "a" / "qoi_moments.npy"), mom)

    monkeypatch.setattr(bench, "DUMP_STATE_VALUES", 200)
    monkeypatch.setattr(bench, "DUMP_SERIES_VALUES", 6)
    for d in "bc":
        bench.dump_outputs(str(tmp_path / d), _FakeSampler(2, 1000), 5, mom)
    st = np.load(tmp_path / "b" / "state.npy")
    assert st.dtype == np.float64 and st.shape == (2, 100)
    assert np.all(np.diff(st[0]) >= 0) and 0 <= st[0].min() and st[0].max() < 1000
    assert np.array_equal(st[1], st[0] + 1)  # the same vertices for every chain
    assert np.array_equal(st, np.load(tmp_path / "c" / "state.npy"))
    assert np.array_equal(np.load(tmp_path / "b" / "qoi_series.npy"), [[2, 3, 4], [3, 4, 5]])


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--n", "32", "--nlevel", "3", *extra], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_chain_it_timed(hip_device, tmp_path):
    """bench.py --dump-outputs at 32^3, 3 levels, 2 warm-up + 3 timed steps: state.npy, qoi_series.npy
    and qoi_moments.npy equal, bit for bit, a sampler driven through the same 5 cycles here; a second
    run writes the same files; the plain line times 3 steps and carries no CPU baseline."""
    import multigridmc_amd as mg
    import bench
    a, b = tmp_path / "a", tmp_path / "b"
    line = _bench("--dump-outputs", str(a))
    _bench("--dump-outputs", str(b))
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-3)
    assert line["cpu_baseline"] is None and line["qoi"]["samples"] == 3

    lat = mg.Lattice3d(32, 32, 32)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, kappa_sq=1.0 / 0.2 ** 2), bench.SEED,
                              mg.MultigridParameters(nlevel=3, smoother="SOR", coarse_solver="SSOR", npresmooth=1,
                                                     npostsmooth=1, ncoarsesmooth=1, omega=1.0, cycle=1,
                                                     coarse_scaling=1.0), device=0)
    q = mg.measurement_vector_index(lat, [0.5] * 3)
    s.sample(2, q)
    s.reset_moments()
    z = s.sample(3, q)
    x, mom = s.get_state(), s.qoi_moments()
    s.close()
    for d in (a, b):
        st, ser, mo = (np.load(d / f) for f in ("state.npy", "qoi_series.npy", "qoi_moments.npy"))
        assert st.dtype == ser.dtype == mo.dtype == np.float64
        assert st.shape == (1, lat.Nvertex) and np.array_equal(st[0], x)
        assert ser.shape == (1, 3) and np.array_equal(ser[0], z)
        assert mo.shape == (1, 3) and np.array_equal(mo[0], mom)


@pytest.mark.gpu
def test_bench_full_adds_the_cpu_baseline(hip_device):
    """--full at 32^3: the line carries the CPU oracle's baseline (1 core and the all-cores aggregate)."""
    line = _bench("--full", "--cpu-samples", "2", "--cpu-warmup", "1")
    assert line["steps"] == 3 and line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] == 1
