"""The QoI panel on the device (-m gpu): mgmc_qoi_panel_* (mgmc_panel.hpp), K functionals b_k^T x per cycle with
their mean, co-moments and windowed autocovariance -- the reference's Statistics (src/auxilliary/statistics.cc).

The yardsticks are the existing scalar path (set_qoi_vector + sample(..., QOI_VECTOR) and qoi_moments) and float64
numpy replays of the three recurrences (the library is built with -ffp-contract=off, so a replay is bit-exact).
Everything but the last test compares bits.

Fixtures: 2D 32 x 24 (3 levels, 713 interior vertices: every column is one partial block) and 3D 24 x 16 x 20
(2 levels, 6555 interior vertices: a dense column has two blocks, the second partial, and rows of 23 < 64 vertices,
so the incremental walk of the dense group carries more than once per step).  Columns: one vertex, a ball, lists of
exactly 4096 and of 4097 entries (3D only), a dense column with distinct values, a dense constant column.
Every run is 12 cycles."""
import ctypes

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd import _native
from multigridmc_amd.distributed import merge_panel_moments
from multigridmc_amd.parameters import MeasurementParameters, MultigridParameters, read_config

pytestmark = pytest.mark.gpu

SEED = 5418513
CHAIN0 = 3
NCYC = 12
FIXTURES = {"2d": ((32, 24), 3), "3d": ((24, 16, 20), 2)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _operator(fixture, variant):
    shape, nlevel = FIXTURES[fixture]
    lat = mg.Lattice(*shape)
    base = mg.ShiftedLaplaceFDOperator(lat, 25.0)
    p = mg.MultigridParameters(nlevel=nlevel)
    if variant == "prior":
        return base, p, None
    # a low-rank part with m = 3, one column dense, and f != 0
    rng = np.random.default_rng(1212417)
    mp = MeasurementParameters(radius=0.0, variance_scaling=1e-3, measure_global=True, variance_global=0.02)
    mp.measurement_locations = [list(rng.uniform(0.15, 0.85, lat.dim)) for _ in range(2)]
    mp.variance = list(1.0 + 2.0 * rng.random(2))
    op = mg.MeasuredOperator(base, mp)
    assert op.get_m_lowrank() == 3
    return op, p, np.random.default_rng(11).standard_normal(lat.Nvertex)


def make(fixture, variant="prior", chain=CHAIN0, nchains=1):
    op, p, f = _operator(fixture, variant)
    s = mg.MultigridMCSampler(op, SEED, p, device=0, chain_id=chain, nchains=nchains)
    if f is not None:
        s.fix_rhs(f)
    return s


def columns(fixture):
    shape, _ = FIXTURES[fixture]
    lat = mg.Lattice(*shape)
    N = lat.Nvertex
    rng = np.random.default_rng(77)
    centre = mg.measurement_vector_index(lat, [0.5] * lat.dim)
    cols = [(np.array([centre], dtype=np.int64), np.array([1.0]))]
    ball = mg.measurement_vector(lat, [0.4, 0.55, 0.6][: lat.dim], 0.1 if lat.dim == 2 else 0.05)  # 43 / 36 entries
    assert 15 <= len(ball[0]) <= 60, len(ball[0])
    cols.append(ball)
    if N > 4097:
        for n in (4096, 4097):
            cols.append((np.sort(rng.choice(N, n, replace=False)).astype(np.int64), rng.standard_normal(n)))
    cols.append((np.arange(N, dtype=np.int64), rng.standard_normal(N)))
    cols.append((np.arange(N, dtype=np.int64), np.full(N, 1.0 / float(np.prod(shape)))))
    return cols


def panel_run(fixture, variant="prior", window=5, chain=CHAIN0, nchains=1, ncyc=NCYC):
    s = make(fixture, variant, chain, nchains)
    s.set_qoi_panel(columns(fixture))
    s.qoi_panel_record(1, window, 64)
    s.sample(ncyc)
    return s


_SCALAR = {}


def scalar_runs(fixture, variant, cache=True):
    """Per column: (series, qoi_moments) of a fresh sampler that records the column as its QoI vector."""
    key = (fixture, variant)
    if cache and key in _SCALAR:
        return _SCALAR[key]
    out = []
    for rows, vals in columns(fixture):
        s = make(fixture, variant)
        s.set_qoi_vector(rows, vals)
        z = s.sample(NCYC, _native.QOI_VECTOR)
        out.append((z.copy(), s.qoi_moments().copy()))
        s.close()
    if cache:
        _SCALAR[key] = out
    return out


def replay(series, W):
    """The three recurrences of k_panel_record on a downloaded (n, K) series: mean, C (mirrored), S (K, W)."""
    n, K = series.shape
    mean, C, S = np.zeros(K), np.zeros((K, K)), np.zeros((K, W))
    iu = np.triu(np.ones((K, K), dtype=bool))
    for r in range(n):
        z = series[r]
        cnt = float(r) + 1.0
        delta = z - mean
        mean = mean + delta / cnt
        C = np.where(iu, C + np.outer(delta, z - mean), C)
        for j in range(min(W, r + 1)):
            p = z * series[r - j]
            nj = r + 1 - j
            S[:, j] = p if nj == 1 else S[:, j] + (p - S[:, j]) / float(nj)
    C = np.triu(C) + np.triu(C, 1).T
    return mean, C, S


def _case1(fixture, variant, cache=True):
    ref = scalar_runs(fixture, variant, cache)
    s = panel_run(fixture, variant)
    z = s.qoi_panel_series()
    assert z.shape == (NCYC, len(ref)) and np.all(np.isfinite(z))
    for k, (zk, _) in enumerate(ref):
        assert same_bits(z[:, k], zk), f"{fixture} {variant}: column {k} differs from the scalar QoI-vector path"
    assert same_bits(s.qoi_panel_eval(), z[-1]), "eval of the current state differs from the last record"
    s.close()


@pytest.mark.parametrize("fixture,variant", [("2d", "prior"), ("3d", "prior"), ("2d", "posterior"), ("3d", "posterior")])
def test_columns_equal_the_scalar_qoi_vector_path(hip_device, fixture, variant):
    """1. Column k of the panel is what MGMC_QOI_VECTOR records for that vector, bit for bit; eval = the last record."""
    _case1(fixture, variant)


@pytest.mark.parametrize("fixture,window", [("3d", 1), ("3d", 5), ("3d", 32), ("2d", 5)])
def test_moments_equal_the_numpy_replay(hip_device, fixture, window):
    """2. mean, C and S against the replay; the diagonal of C against the scalar path's M2; nlags = min(W, 12)."""
    s = panel_run(fixture, "prior", window)
    z = s.qoi_panel_series()
    n, mean, C = s.qoi_panel_comoments()
    S, nlags = s.qoi_panel_autocovariance()
    rm, rC, rS = replay(z, window)
    assert n == NCYC and nlags == min(window, NCYC) and S.shape == (z.shape[1], window)
    assert same_bits(mean, rm) and same_bits(C, rC)
    assert same_bits(S[:, :nlags], rS[:, :nlags])
    for k, (_, mom) in enumerate(scalar_runs(fixture, "prior")):
        assert mom[0] == NCYC and same_bits(mean[k], mom[1]) and same_bits(C[k, k], mom[2]), k
    n2, m2, cov = s.qoi_panel_moments(0)
    assert same_bits(cov, C / (NCYC - 1.0))
    tau = s.qoi_panel_tau_int()
    ref_tau = mg.tau_int_from_autocov(rS[:, :nlags] - (rm * rm)[:, None])
    assert same_bits(tau, ref_tau)
    s.close()


def test_stride_counters_reset_and_capacity(hip_device):
    """3. stride 3 records cycles 3, 6, 9, 12; info; reset zeroes everything and the thinning restarts; a capacity
    of 2 keeps two records while the moments count four.  (That reset rebuilds no graph cannot be seen from Python:
    the level_kernels comparison only shows that the plan is untouched; mgmc_qoi_panel_record_reset's code path,
    panel_zero, has no call that could rebuild.)"""
    full = panel_run("2d")
    zf = full.qoi_panel_series()
    full.close()
    s = make("2d")
    s.set_qoi_panel(columns("2d"))
    assert s.qoi_panel_info() == {"K": 4, "enabled": False, "stride": 0, "window": 0, "ncycles": 0, "nrecorded": 0}
    s.qoi_panel_record(3, 5, 2)
    assert s.qoi_panel_info() == {"K": 4, "enabled": True, "stride": 3, "window": 5, "ncycles": 0, "nrecorded": 0}
    s.sample(NCYC)
    assert s.qoi_panel_info() == {"K": 4, "enabled": True, "stride": 3, "window": 5, "ncycles": 12, "nrecorded": 4}
    z = s.qoi_panel_series()
    assert same_bits(z, zf[[2, 5]])  # the first `capacity` records
    n, mean, C = s.qoi_panel_comoments()
    rm, rC, rS = replay(zf[[2, 5, 8, 11]], 5)
    S, nlags = s.qoi_panel_autocovariance()
    assert n == 4 and nlags == 4 and same_bits(mean, rm) and same_bits(C, rC) and same_bits(S[:, :4], rS[:, :4])
    kernels = [s.level_kernels(l) for l in range(3)]
    s.reset_qoi_panel()
    assert [s.level_kernels(l) for l in range(3)] == kernels
    assert s.qoi_panel_info() == {"K": 4, "enabled": True, "stride": 3, "window": 5, "ncycles": 0, "nrecorded": 0}
    n, mean, C = s.qoi_panel_comoments()
    S, nlags = s.qoi_panel_autocovariance()
    assert n == 0 and nlags == 0 and not mean.any() and not C.any() and not S.any()
    assert s.qoi_panel_series().shape == (0, 4)
    s.sample(4)  # cycles 13 .. 16 of the chain are cycles 1 .. 4 of the record: one record, cycle 15's state
    assert s.qoi_panel_info()["nrecorded"] == 1 and s.qoi_panel_info()["ncycles"] == 4
    s.sample(2)
    assert s.qoi_panel_info()["nrecorded"] == 2
    assert same_bits(s.qoi_panel_eval(), s.qoi_panel_series()[1])
    s.close()


def test_batched_chains_equal_one_chain_samplers(hip_device):
    """4. Chain c of a batch of three equals the one-chain sampler with id CHAIN0 + c; chain=None is the host merge."""
    b = panel_run("3d", "posterior", 5, CHAIN0, 3)
    parts = []
    for c in range(3):
        s = panel_run("3d", "posterior", 5, CHAIN0 + c, 1)
        assert same_bits(b.qoi_panel_series(c), s.qoi_panel_series()), c
        nb, mb, Cb = b.qoi_panel_comoments(c)
        n1, m1, C1 = s.qoi_panel_comoments()
        assert nb == n1 == NCYC and same_bits(mb, m1) and same_bits(Cb, C1), c
        assert same_bits(b.qoi_panel_autocovariance(c)[0], s.qoi_panel_autocovariance()[0]), c
        assert same_bits(b.qoi_panel_eval(c), s.qoi_panel_eval()), c
        parts.append((n1, m1, C1))
        s.close()
    n, mean, C = merge_panel_moments(parts)
    gn, gmean, gcov = b.qoi_panel_moments(None)
    assert gn == 3 * NCYC and same_bits(gmean, mean) and same_bits(gcov, C / (n - 1.0))
    # the merge against pooling the three series (the bound of tests/test_qoi_panel_host.py)
    pooled = np.concatenate([b.qoi_panel_series(c) for c in range(3)])
    assert np.max(np.abs(gcov - np.cov(pooled.T))) <= 16 * np.finfo(float).eps * np.linalg.norm(gcov)
    b.close()


def test_the_chain_and_the_other_records_keep_their_bits(hip_device):
    """5. Neutrality: the state, the scalar series and its moments with and without a recording panel; after
    qoi_panel_off the kernels and the next 4 cycles of a sampler that never had one; field statistics and the
    energy record next to the panel."""
    rows, vals = columns("3d")[1]

    def run(panel):
        s = make("3d", "posterior")
        s.set_qoi_vector(rows, vals)
        s.field_stats(2)
        s.energy_record(1, 16)
        if panel:
            s.set_qoi_panel(columns("3d"))
            s.qoi_panel_record(2, 5, 16)
        z = s.sample(NCYC, _native.QOI_VECTOR)
        return s, z

    a, za = run(True)
    b, zb = run(False)
    assert same_bits(za, zb) and same_bits(a.qoi_moments(), b.qoi_moments())
    assert same_bits(a.get_state(), b.get_state())
    assert a.qoi_panel_info()["nrecorded"] == 6
    assert same_bits(a.qoi_panel_series()[:, 1], za[1::2])
    fa, fb = a.field_moments(), b.field_moments()
    assert fa[0] == fb[0] and same_bits(fa[1], fb[1]) and same_bits(fa[2], fb[2])
    assert all(same_bits(u, v) for u, v in zip(a.energy_series(), b.energy_series()))
    assert same_bits(a.energy_moments(), b.energy_moments())
    a.qoi_panel_off()
    assert a.qoi_panel_info()["enabled"] is False and a.qoi_panel_info()["K"] == 6
    for level in range(2):
        assert a.level_kernels(level) == b.level_kernels(level)
    assert same_bits(a.sample(4, _native.QOI_VECTOR), b.sample(4, _native.QOI_VECTOR))
    assert same_bits(a.get_state(), b.get_state())
    a.close()
    b.close()


def test_other_setters_do_not_touch_the_panel(hip_device):
    """set_lowrank, fix_rhs, set_state, set_qoi_vector and reset_moments leave the panel and its records alone."""
    s = panel_run("2d", ncyc=5)
    before = s.qoi_panel_series()
    x = s.get_state()
    s.set_qoi_vector(*columns("2d")[1])
    s.reset_moments()
    s.fix_rhs(np.zeros(s.ndof))
    s.set_state(x)
    s.set_lowrank(None)
    assert s.qoi_panel_info()["nrecorded"] == 5 and same_bits(s.qoi_panel_series(), before)
    s.sample(NCYC - 5)
    ref = panel_run("2d")
    assert same_bits(s.qoi_panel_series(), ref.qoi_panel_series())
    s.close()
    ref.close()


def test_invalid_input_leaves_the_panel_recording(hip_device):
    """6. Every MGMC_E_INVALID case, each followed by a cycle: the 12 records are those of an undisturbed run."""
    lib = mg.load_library()
    P = ctypes.POINTER(ctypes.c_int64)
    D = ctypes.POINTER(ctypes.c_double)

    def raw(h, K, colptr, rows, vals):
        colptr, rows = np.asarray(colptr, dtype=np.int64), np.asarray(rows, dtype=np.int64)
        vals = np.asarray(vals, dtype=np.float64)
        return lib.mgmc_qoi_panel_set(h, K, colptr.ctypes.data_as(P), rows.ctypes.data_as(P), vals.ctypes.data_as(D))

    fresh = make("2d")
    N = fresh.ndof
    assert lib.mgmc_qoi_panel_record_enable(fresh.handle, 1, 5, 8) == _native.MGMC_E_INVALID
    assert "panel" in _native.last_error(fresh.handle)
    out = np.zeros(4)
    assert lib.mgmc_qoi_panel_eval(fresh.handle, out.ctypes.data_as(D)) == _native.MGMC_E_INVALID
    assert lib.mgmc_qoi_panel_record_reset(fresh.handle) == _native.MGMC_E_INVALID
    fresh.set_qoi_panel(columns("2d"))
    for stride, window, cap in [(0, 5, 8), (1, 0, 8), (1, 257, 8), (1, 5, 0)]:
        assert lib.mgmc_qoi_panel_record_enable(fresh.handle, stride, window, cap) == _native.MGMC_E_INVALID
    fresh.close()

    bad = [
        (-1, [0], [0], [1.0]),
        (65, list(range(66)), list(range(65)), [1.0] * 65),
        (2, [1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0]),        # colptr[0] != 0
        (2, [0, 2, 1], [0, 1, 2], [1.0, 1.0, 1.0]),        # colptr decreases
        (2, [0, 2, 3], [3, 3, 2], [1.0, 1.0, 1.0]),        # rows not strictly ascending
        (2, [0, 2, 3], [3, 2, 2], [1.0, 1.0, 1.0]),
        (1, [0, 2], [-1, 2], [1.0, 1.0]),                  # out of range
        (1, [0, 2], [1, N], [1.0, 1.0]),
        (1, [0, 2], [1, 2], [1.0, np.nan]),                # non-finite
        (1, [0, 2], [1, 2], [np.inf, 1.0]),
        (2, [0, 2, 2], [1, 2], [1.0, 1.0]),                # an empty column
    ]
    assert len(bad) <= NCYC
    s = make("2d")
    s.set_qoi_panel(columns("2d"))
    s.qoi_panel_record(1, 5, 64)
    for case in bad:
        assert raw(s.handle, *case) == _native.MGMC_E_INVALID, case
        assert _native.last_error(s.handle).startswith("QoI panel"), case
        assert s.qoi_panel_info()["K"] == 4
        s.sample(1)
    s.sample(NCYC - len(bad))
    ref = panel_run("2d")
    assert same_bits(s.qoi_panel_series(), ref.qoi_panel_series())
    assert same_bits(s.qoi_panel_comoments()[2], ref.qoi_panel_comoments()[2])
    # a new panel while recording starts the records again; removing it ends the recording
    s.set_qoi_panel(columns("2d")[:2])
    assert s.qoi_panel_info() == {"K": 2, "enabled": True, "stride": 1, "window": 5, "ncycles": 0, "nrecorded": 0}
    s.sample(2)
    assert s.qoi_panel_series().shape == (2, 2)
    s.set_qoi_panel([])
    assert s.qoi_panel_info() == {"K": 0, "enabled": False, "stride": 0, "window": 0, "ncycles": 0, "nrecorded": 0}
    s.sample(1)
    s.close()
    ref.close()


def test_poisoned_panel_equals_the_scalar_path(hip_device, monkeypatch):
    """7. Case 1 on the 3D fixture with NaN-filled LDS before every op and NaN-filled scratch (MGMC_POISON=1, read
    at creation): every LDS word and every partial the two kernels read was written by them."""
    monkeypatch.setenv("MGMC_POISON", "1")
    _case1("3d", "posterior", cache=False)
    s = panel_run("3d", "prior", 32)
    z = s.qoi_panel_series()
    n, mean, C = s.qoi_panel_comoments()
    S, nlags = s.qoi_panel_autocovariance()
    rm, rC, rS = replay(z, 32)
    assert same_bits(mean, rm) and same_bits(C, rC) and same_bits(S[:, :nlags], rS[:, :nlags])
    s.close()


def test_merged_moments_against_exact_targets(hip_device):
    """8. 2D 32^2, 3 levels, the template's posterior (8 point measurements, f = B Sigma^-1 y), K = 4: the driver's
    QoI vector and three ball averages (radius 0.1) away from the sites; 4 chains x 2000 cycles after 200 of
    warm-up.  The merged mean and covariance against b_k^T Q^-1 f and b_k^T Q^-1 b_l from the device CG, every
    entry within 5 standard errors: se(mean_k) = sqrt(C_kk tau / n), se(cov_kl) = sqrt((C_kk C_ll + C_kl^2) tau / n)
    with the exact C, tau = max(1, the largest measured tau_int) and n = 8000.
    (The columns have |mean| / std between 1.4 and 4.8.  The predicted data at the sites themselves have
    |mean| / std of 1e3 and more; there the reference's estimator C(j) = S_j - avg^2, statistics.cc:54-62, loses
    its digits to the cancellation, tau_int comes out in the hundreds -- measured 311 -- and a bound scaled by it
    checks nothing.)"""
    import os
    gold = os.path.join(os.path.dirname(__file__), "golden")
    cfg = read_config(os.path.join(gold, "parameters_template.cfg"))
    mp = MeasurementParameters.from_config(cfg, gold)
    lat = mg.Lattice(32, 32)
    op = mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(lat, mg.ConstantCorrelationLengthModel(0.2)), mp)
    p = MultigridParameters(nlevel=3)
    s = mg.MultigridMCSampler(op, SEED, p, device=0, chain_id=0, nchains=4)
    lr = op.get_B()
    y = np.asarray(list(mp.mean[:len(mp.measurement_locations)]), dtype=np.float64)
    f = np.zeros(lat.Nvertex)
    for k in range(len(y)):
        sl = slice(lr.colptr[k], lr.colptr[k + 1])
        f[lr.rows[sl]] += lr.vals[sl] * (y[k] / lr.sigma[k])
    assert len(mg.measurement_panel(op)) == 8
    cols = [mg.measurement_vector(lat, mp.sample_location, mp.radius)] + \
        [mg.measurement_vector(lat, x0, 0.1) for x0 in ([0.2, 0.8], [0.8, 0.2], [0.5, 0.15])]
    K = len(cols)
    Bd = np.zeros((lat.Nvertex, K))
    for k, (r, v) in enumerate(cols):
        Bd[r, k] = v
    solver = mg.MultigridMCSampler(op, SEED, p, device=0)
    sol = [solver.solve(Bd[:, k], method="cg", rtol=1e-12, maxiter=200) for k in range(K)]
    assert all(it < 200 for _, it, _ in sol)
    solver.close()
    U = np.stack([x for x, _, _ in sol], axis=1)
    mean_exact, cov_exact = U.T @ f, Bd.T @ U
    s.fix_rhs(f)
    s.set_qoi_panel(cols)
    s.sample(200)
    s.qoi_panel_record(1, 32, 1)
    s.sample(2000)
    n, mean, cov = s.qoi_panel_moments(None)
    assert n == 8000
    tau = max(1.0, max(float(np.max(s.qoi_panel_tau_int(c))) for c in range(4)))
    d = np.diag(cov_exact)
    se_mean = np.sqrt(d * tau / n)
    se_cov = np.sqrt((np.outer(d, d) + cov_exact ** 2) * tau / n)
    zm, zc = (mean - mean_exact) / se_mean, (cov - cov_exact) / se_cov
    print(f"panel statistics: tau = {tau:.3f}, max |z| mean = {np.max(np.abs(zm)):.2f}, cov = {np.max(np.abs(zc)):.2f}")
    assert np.all(np.abs(zm) < 5.0), zm
    assert np.all(np.abs(zc) < 5.0), zc
    s.close()


def test_predicted_data_against_exact_targets(hip_device):
    """The panel a posterior run records, B^T x at the template's 8 measurement sites (K = 8), same lattice, chains
    and cycles as case 8: merged mean and covariance against the exact b_k^T Q^-1 f and b_k^T Q^-1 b_l, every entry
    within 5 standard errors (the formulas of case 8, exact C, n = 8000).  These columns have |mean| / std of
    1e3 .. 4e3, where S_j - avg^2 cancels (case 8's docstring), so tau is not taken from the device's S: it is
    max(1, the largest tau_int over chains and columns) of the reference's own estimator (mg.panel_statistics,
    window 32) applied to the downloaded series minus the exact mean -- the same estimator without the
    cancellation, the centring constant independent of the chain."""
    import os
    gold = os.path.join(os.path.dirname(__file__), "golden")
    cfg = read_config(os.path.join(gold, "parameters_template.cfg"))
    mp = MeasurementParameters.from_config(cfg, gold)
    lat = mg.Lattice(32, 32)
    op = mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(lat, mg.ConstantCorrelationLengthModel(0.2)), mp)
    p = MultigridParameters(nlevel=3)
    lr = op.get_B()
    y = np.asarray(list(mp.mean[:len(mp.measurement_locations)]), dtype=np.float64)
    Bd = lr.dense()
    K = Bd.shape[1]
    assert K == 8
    f = Bd @ (y / lr.sigma)
    solver = mg.MultigridMCSampler(op, SEED, p, device=0)
    sol = [solver.solve(Bd[:, k], method="cg", rtol=1e-13, maxiter=200) for k in range(K)]
    assert all(it < 200 for _, it, _ in sol)
    solver.close()
    U = np.stack([x for x, _, _ in sol], axis=1)
    mean_exact, cov_exact = U.T @ f, Bd.T @ U
    s = mg.MultigridMCSampler(op, SEED, p, device=0, chain_id=0, nchains=4)
    s.fix_rhs(f)
    s.set_qoi_panel(mg.measurement_panel(op))
    s.sample(200)
    s.qoi_panel_record(1, 32, 2000)
    s.sample(2000)
    n, mean, cov = s.qoi_panel_moments(None)
    assert n == 8000
    tau = max(1.0, max(float(np.max(mg.panel_statistics(s.qoi_panel_series(c) - mean_exact, 32).tau_int_columns()))
                       for c in range(4)))
    d = np.diag(cov_exact)
    se_mean = np.sqrt(d * tau / n)
    se_cov = np.sqrt((np.outer(d, d) + cov_exact ** 2) * tau / n)
    zm, zc = (mean - mean_exact) / se_mean, (cov - cov_exact) / se_cov
    print(f"predicted data: tau = {tau:.3f}, max |z| mean = {np.max(np.abs(zm)):.2f}, cov = {np.max(np.abs(zc)):.2f}")
    assert np.all(np.abs(zm) < 5.0), zm
    assert np.all(np.abs(zc) < 5.0), zc
    s.close()


def test_driver_qoi_panel(hip_device, tmp_path, monkeypatch, capsys):
    """--qoi-panel on the template's 2D posterior: the 8 predicted data and the QoI (K = 9 <= 16, so the exact
    mean and covariance are printed too) in operator<<'s layout; panel_multigridmc.txt holds (cycle, z_0 .. z_8) of
    the 500 samples, its last column the QoI of timeseries_multigridmc.txt (written with 6 digits)."""
    import os
    import re
    from multigridmc_amd.driver import main
    gold = os.path.join(os.path.dirname(__file__), "golden")
    text = open(os.path.join(gold, "parameters_template.cfg")).read()
    text = re.sub(r"nsamples = 10000;", "nsamples = 500;", text)
    text = re.sub(r"nsamples = 1000;", "nsamples = 20;", text)
    text = re.sub(r"save_posterior_statistics = true;", "save_posterior_statistics = false;", text)
    (tmp_path / "parameters.cfg").write_text(text)
    (tmp_path / "measurements_template.cfg").write_text(open(os.path.join(gold, "measurements_template.cfg")).read())
    monkeypatch.chdir(tmp_path)
    assert main(["--qoi-panel", str(tmp_path / "parameters.cfg")]) == 0
    rows = np.loadtxt(tmp_path / "panel_multigridmc.txt")
    assert rows.shape == (500, 10) and np.array_equal(rows[:, 0], np.arange(1.0, 501.0))
    series = np.loadtxt(tmp_path / "timeseries_multigridmc.txt")
    assert np.allclose(rows[:, 9], series, rtol=1e-5, atol=1e-9)
    out = capsys.readouterr().out
    assert len(re.findall(r" MGMC: tau_\{int,j\} = [-0-9.naif]+", out)) == 9
    assert re.search(r" MGMC: window      = 32\n MGMC: # samples   = 500\n", out), out
    avg = [float(v) for v in re.search(r" MGMC: Avg = (.*)", out).group(1).split()]
    exact = [float(v) for v in re.search(r" exact: Avg = (.*)", out).group(1).split()]
    assert len(avg) == len(exact) == 9
    assert np.allclose(avg[:8], exact[:8], atol=0.02)  # the predicted data: pinned by the measurements (std 1e-3)
    assert len(re.findall(r"^ exact: Var = ", out, flags=re.M)) == 1


def test_cpp_sampler_panel_methods_on_the_device(hip_device, tmp_path):
    """include/mgmc_sampler.hh's panel methods from C++ (tests/cpp/qoi_panel_client.cpp, the plain build, no
    sanitizer): 5 recorded cycles of the 2D fixture with a vertex column and a dense constant column equal the Python
    sampler's records to the 17 digits printed, eval is the last record, and K = 0 removes the panel."""
    import subprocess
    from tests.test_qoi_panel_host import build_panel_client
    exe = build_panel_client(tmp_path)
    r = subprocess.run([exe, "record", "5"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "records 5 K 2 count 5 nlags 4"
    zs = np.array([[float(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("z ")])
    assert zs.shape == (5, 2) and lines[6].split()[1:] == lines[5].split()[1:]  # eval = the last record
    assert lines[-1] == "after K 0"
    N = 31 * 23
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(mg.Lattice(32, 24), 25.0), SEED, mg.MultigridParameters(nlevel=3),
                              device=0, chain_id=0)
    s.set_qoi_panel([(np.array([11 * 31 + 15]), np.array([1.0])), (np.arange(N), np.full(N, 1.0 / (32.0 * 24.0)))])
    s.qoi_panel_record(1, 4, 64)
    s.sample(5)
    assert same_bits(s.qoi_panel_series(), zs)
    n, mean, C = s.qoi_panel_comoments()
    assert [float(v) for v in lines[7].split()[1:]] == list(mean)
    assert [float(v) for v in lines[8].split()[1:]] == list(C.ravel())
    s.qoi_panel_off()
    assert s.qoi_panel_series().shape == (0, 2)
    s.close()
