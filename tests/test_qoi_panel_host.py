"""The host side of the QoI panel (CPU only): the C-ABI symbols, panel_statistics (the reference's Statistics,
src/auxilliary/statistics.cc, restated for a host series), the matrix Chan merge, measurement_panel and the
C++ methods of include/mgmc_sampler.hh."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd import _native
from multigridmc_amd.distributed import merge_panel_moments, panel_moments_of
from multigridmc_amd.parameters import MeasurementParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["mgmc_qoi_panel_set", "mgmc_qoi_panel_eval", "mgmc_qoi_panel_record_enable",
           "mgmc_qoi_panel_record_disable", "mgmc_qoi_panel_record_reset", "mgmc_qoi_panel_info",
           "mgmc_qoi_panel_get_series", "mgmc_qoi_panel_moments", "mgmc_qoi_panel_autocov"]


def test_library_exports_the_nine_symbols_and_the_abi_stays_5():
    lib = mg.load_library()
    bound = {name for name, _, _ in _native.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "mgmc.h")).read()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in bound and f"int {s}(" in header, s
    assert lib.mgmc_abi_version() == _native.ABI_VERSION == 5
    # a null handle is refused before any device call
    assert lib.mgmc_qoi_panel_record_enable(None, 1, 32, 16) == _native.MGMC_E_INVALID
    assert lib.mgmc_qoi_panel_set(None, 0, None, None, None) == _native.MGMC_E_INVALID


def ar1(n, K, seed=20250219):
    """x_i = Phi x_{i-1} + e_i with a fixed numpy seed: K correlated AR(1) components with a non-zero mean"""
    rng = np.random.default_rng(seed)
    phi = np.linspace(0.2, 0.9, K)
    mix = np.eye(K) + 0.3 * rng.standard_normal((K, K))
    x = np.zeros(K)
    out = np.empty((n, K))
    for i in range(n):
        x = phi * x + rng.standard_normal(K)
        out[i] = mix @ x + np.arange(1, K + 1)
    return out


def direct_statistics(series, window):
    """statistics.cc:5-38 line by line, with a deque: (n, avg, avg2, [S_0, S_1, ...])"""
    from collections import deque
    Qk, Sk = deque(), []
    n, avg, avg2 = 0, None, None
    for Q in series:
        n += 1
        if n == 1:
            avg, avg2 = Q.copy(), np.outer(Q, Q)
        else:
            avg = avg + (Q - avg) / (1.0 * n)
            avg2 = avg2 + (np.outer(Q, Q) - avg2) / (1.0 * n)
        Qk.appendleft(Q.copy())
        if len(Qk) > window:
            Qk.pop()
        for k in range(len(Qk)):
            Nk = n - k
            if Nk == 1:
                Sk.append(np.outer(Qk[0], Qk[k]))
            else:
                Sk[k] = Sk[k] + (np.outer(Qk[0], Qk[k]) - Sk[k]) / (1.0 * Nk)
    return n, avg, avg2, Sk


def direct_tau_int(avg, Sk, v):
    """statistics.cc:54-80"""
    Ck = [S - np.outer(avg, avg) for S in Sk]
    variance = v @ Ck[0] @ v
    tau = 1.0
    kmax = len(Ck)
    for k in range(1, kmax):
        tau += 2 * (1.0 - k / (1.0 * kmax)) * (v @ Ck[k] @ v) / variance
    return tau


@pytest.mark.parametrize("n,window", [(400, 16), (10, 32), (1, 8)])
def test_panel_statistics_against_the_direct_restatement(n, window):
    """An AR(1) series; W larger than the series (10 samples, window 32); a one-sample series."""
    K = 3
    z = ar1(n, K)
    st = mg.panel_statistics(z, window)
    dn, avg, avg2, Sk = direct_statistics(z, window)
    assert st.samples() == dn == n
    assert np.array_equal(st.average(), avg)
    L = min(window, n)
    C = st.auto_covariance()
    assert C.shape == (L, K, K)
    for k in range(L):
        assert np.array_equal(C[k], Sk[k] - np.outer(avg, avg)), k
    if n == 1:
        assert np.all(np.isnan(st.covariance()))  # n / (n - 1) with n = 1, as the reference's
        assert st.tau_int([1.0, 0.0, 0.0]) == 1.0
        return
    assert np.array_equal(st.covariance(), 1.0 * n / (n - 1.0) * (avg2 - np.outer(avg, avg)))
    assert np.allclose(st.covariance(), np.cov(z.T), rtol=1e-11, atol=0)
    for v in (np.array([1.0, 0.0, 0.0]), np.array([0.5, -2.0, 1.5])):
        assert st.tau_int(v) == pytest.approx(direct_tau_int(avg, Sk, v), rel=1e-13)
    units = st.tau_int_columns()
    for k in range(K):
        assert units[k] == pytest.approx(direct_tau_int(avg, Sk, np.eye(K)[k]), rel=1e-13)
    if n == 400:  # the slowest component (phi 0.9 dominates the last mixed column) has the largest tau
        assert units.max() > 3.0 and units.min() > 0.8


def test_one_dimensional_series_is_one_observable():
    z = ar1(50, 1)[:, 0]
    st = mg.panel_statistics(z, 4)
    assert st.average().shape == (1,) and st.covariance().shape == (1, 1)
    assert st.covariance()[0, 0] == pytest.approx(z.var(ddof=1), rel=1e-12)


def test_matrix_chan_merge_against_pooling():
    """merge_panel_moments of per-chunk (n, mean, C) against the two-pass moments of the pooled series.  Measured
    here: max |C_merged - C_pooled| = 1.22 eps ||C||_F (K = 4, chunks of 10, 1, 57 and 300 samples of an AR(1) series
    with means 1 .. 4).  Either side carries an error of a few eps ||C|| (n K rounded terms each, errors adding like
    sqrt(n)); the bound 16 eps ||C||_F leaves a factor of about 13 over the measured figure and is four orders of
    magnitude below the effect of a dropped or doubled cross term delta delta^T n nb / tot."""
    z = ar1(368, 4)
    cuts = [0, 10, 11, 68, 68, 368]
    parts = [panel_moments_of(z[a:b]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    parts.insert(2, (0.0, np.zeros(4), np.zeros((4, 4))))  # an empty chain is skipped
    n, mean, C = merge_panel_moments(parts)
    pn, pmean, pC = panel_moments_of(z)
    assert n == pn == 368
    err = np.max(np.abs(C - pC)) / np.linalg.norm(pC)
    print(f"matrix Chan merge: max |dC| / ||C||_F = {err / np.finfo(float).eps:.2f} eps")
    assert err <= 16 * np.finfo(float).eps
    assert np.max(np.abs(mean - pmean)) <= 8 * np.finfo(float).eps * np.max(np.abs(pmean))
    assert np.array_equal(C, C.T)
    # K = 1 is distributed.merge_moments
    from multigridmc_amd.distributed import merge_moments, moments_of
    s1 = merge_moments([moments_of(z[a:b, 0]) for a, b in zip(cuts[:-1], cuts[1:])])
    p1 = merge_panel_moments([panel_moments_of(z[a:b, :1]) for a, b in zip(cuts[:-1], cuts[1:]) if b > a])
    assert s1[0] == p1[0] and s1[1] == pytest.approx(p1[1][0], rel=1e-14) and s1[2] == pytest.approx(p1[2][0, 0], rel=1e-13)
    with pytest.raises(ValueError):
        merge_panel_moments([])


def test_measurement_panel_column_layout():
    lat = mg.Lattice(16, 12)
    mp = MeasurementParameters(radius=0.1, variance_scaling=1.0, measure_global=True, variance_global=0.01)
    mp.measurement_locations = [[0.3, 0.4], [0.7, 0.6]]
    mp.variance = [1e-3, 2e-3]
    op = mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(lat, 25.0), mp)
    extra = (np.array([3, 5]), np.array([1.0, -1.0]))
    cols = mg.measurement_panel(op, extra=[extra])
    lr = op.get_B()
    assert len(cols) == lr.m + 1 == 4
    for k in range(2):
        r, v = mg.measurement_vector(lat, mp.measurement_locations[k], 0.1)
        assert np.array_equal(cols[k][0], r) and np.array_equal(cols[k][1], v)
    assert np.array_equal(cols[2][0], np.arange(lat.Nvertex)) and np.all(cols[2][1] == 1.0 / (16 * 12))  # global
    assert np.array_equal(cols[3][0], extra[0]) and np.array_equal(cols[3][1], extra[1])
    assert cols[3][0].dtype == np.int64 and cols[3][1].dtype == np.float64
    B = lr.dense()
    for k in range(3):
        assert np.array_equal(B[cols[k][0], k], cols[k][1])
    assert len(mg.measurement_panel(op)) == 3


def build_panel_client(tmpdir, asan=False):
    exe = os.path.join(str(tmpdir), "qoi_panel_client_asan" if asan else "qoi_panel_client")
    libdir = os.path.join(ROOT, "multigridmc_amd")
    san = ["-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"] \
        if asan else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "qoi_panel_client.cpp"), "-L", libdir, "-lmgmc_hip",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("asan", [False, True])
def test_cpp_sampler_panel_methods_compile_and_link(tmp_path, asan):
    """include/mgmc_sampler.hh's panel methods compile with g++ -Wall -Werror against the C-ABI library (also with
    AddressSanitizer + UBSan on the client); the nine entry points refuse a null handle (host only); without a GPU
    the construction of the sampler prints the library error and exits with -1.  With a GPU present the test ends
    after the host-only part, as tests/test_host.py's client test does."""
    exe = build_panel_client(tmp_path, asan)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, "link"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "abi 5 refused 9", (r.stdout, r.stderr)
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_int(0)
    if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 and n.value > 0:
        return  # nothing instrumented opens a GPU; tests/test_gpu_qoi_panel.py runs the plain client's `record` there
    r = subprocess.run([exe, "record", "2"], capture_output=True, text=True, env=env)
    assert r.returncode == 255 and "ERROR: mgmc_create" in r.stderr
