"""Host side of the batch-means field statistics (no GPU): mgmc_field_stats_enable_batched and
MultigridMCSampler.field_mean_stderr / field_iact.

  * BatchMirror, the kernel's update in numpy float64 (shared with tests/test_gpu_field_batch.py): a direct
    transcription of the semantics in include/mgmc.h, held here against a straightforward recomputation of the
    batch means within a rounding bound, and exactly where exactness follows (a partial batch, B = 1);
  * batch_means_estimates, the one place of the stderr and iact formulas, on hand-made arrays;
  * the NULL-handle contract of the new entry points;
  * the estimator itself on a slowly mixing chain of the CPU oracle: the batch-means tau of the centre vertex
    against the windowed estimator the statistical tests use, over 20 chain ids.
"""
import ctypes

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd import _native
from tests import oracle_lib

SEED = 5418513


class BatchMirror:
    """Field statistics with batch means, one recorded cycle at a time: record(xs) takes the K chains' states
    of one recorded cycle, in chain order."""

    def __init__(self, ndof, nchains, batch):
        self.K, self.B = int(nchains), int(batch)
        self.n = 0   # states folded in
        self.r = 0   # recorded cycles
        self.nb = 0  # completed batches
        self.mean, self.m2 = np.zeros(ndof), np.zeros(ndof)
        self.bsum, self.bmean, self.bm2 = np.zeros(ndof), np.zeros(ndof), np.zeros(ndof)

    def record(self, xs):
        assert len(xs) == self.K
        self.r += 1
        for x in xs:
            cnt = float(self.n + 1)
            delta = x - self.mean
            mean = self.mean + delta / cnt
            self.m2 = self.m2 + delta * (x - mean)
            self.mean = mean
            self.n += 1
            self.bsum = self.bsum + x
        if self.r % self.B == 0:
            bm = self.bsum / float(self.B * self.K)
            self.nb = self.r // self.B
            d = bm - self.bmean
            self.bmean = self.bmean + d / float(self.nb)
            self.bm2 = self.bm2 + d * (bm - self.bmean)
            self.bsum = np.zeros_like(self.bsum)

    def reset(self):
        self.__init__(len(self.mean), self.K, self.B)


def iact_windowed(z):
    """the windowed series estimator of the statistical tests (_iact of tests/test_gpu_exact.py)"""
    z = z - z.mean()
    var = z.var()
    tau = 1.0
    for t in range(1, len(z) // 10):
        rho = np.dot(z[:-t], z[t:]) / ((len(z) - t) * var)
        if rho < 0.05:
            break
        tau += 2 * rho
    return tau


def iact_batch_means(z, batch):
    """batch-means tau of one series, through the mirror and batch_means_estimates"""
    m = BatchMirror(1, 1, batch)
    for v in z:
        m.record([np.array([v])])
    return float(mg.batch_means_estimates(batch, m.nb, m.bm2, m.n, m.m2)[1][0])


@pytest.mark.parametrize("K,B,ncycles", [(1, 4, 10), (3, 2, 9), (2, 5, 23), (1, 1, 7), (3, 1, 5), (1, 7, 6)])
def test_mirror_against_a_plain_recomputation(K, B, ncycles):
    """bmean and bM2 against the batch means computed from the whole series at once.  Rounding: a batch sum is
    B K additions and one division, the Welford fold of nb means a few operations per batch, each with a relative
    error of at most eps = 2^-53 on values bounded by xmax, so bmean is within 4 (B K + nb) eps xmax of the plain
    mean of the batch means and bM2 within 4 (B K + nb) eps nb (2 xmax)^2 of their sum of squared deviations."""
    ndof = 37
    X = np.random.default_rng(100 * K + B).standard_normal((ncycles, K, ndof))
    m = BatchMirror(ndof, K, B)
    for cyc in X:
        m.record(list(cyc))
    nb = ncycles // B
    assert m.nb == nb and m.r == ncycles and m.n == ncycles * K
    eps, xmax = 2.0 ** -53, float(np.abs(X).max())
    if nb:
        means = X[:nb * B].reshape(nb, B * K, ndof).mean(axis=1)
        assert np.abs(m.bmean - means.mean(axis=0)).max() <= 4 * (B * K + nb) * eps * xmax
        dev = ((means - means.mean(axis=0)) ** 2).sum(axis=0)
        assert np.abs(m.bm2 - dev).max() <= 4 * (B * K + nb) * eps * nb * (2 * xmax) ** 2
        assert nb < 2 or np.all(m.bm2 > 0)
    else:
        assert not m.bmean.any() and not m.bm2.any()
    # the Welford fields are those of the mirror without batching (tests/test_gpu_field_stats.py)
    flat = X.reshape(-1, ndof)
    assert np.abs(m.mean - flat.mean(axis=0)).max() <= 4 * len(flat) * eps * xmax
    # the partial batch: in bsum alone, summed in recording order from +0.0
    part = np.zeros(ndof)
    for cyc in X[nb * B:]:
        for x in cyc:
            part = part + x
    assert np.array_equal(m.bsum, part)
    if ncycles % B == 0:  # just completed: +0.0
        assert not m.bsum.any() and not np.signbit(m.bsum).any()


def test_partial_batch_leaves_the_batch_fields_alone():
    ndof, K, B = 11, 2, 4
    X = np.random.default_rng(5).standard_normal((10, K, ndof))
    full, part = BatchMirror(ndof, K, B), BatchMirror(ndof, K, B)
    for cyc in X[:8]:
        full.record(list(cyc))
    for cyc in X:
        part.record(list(cyc))
    assert full.nb == part.nb == 2
    assert np.array_equal(full.bmean, part.bmean) and np.array_equal(full.bm2, part.bm2)
    assert not full.bsum.any() and part.bsum.any()
    part.reset()
    assert part.n == part.r == part.nb == 0 and not part.bsum.any() and not part.bmean.any()


def test_batch_of_one_cycle_of_one_chain_is_the_welford_update():
    """B = 1, K = 1: bsum = +0.0 + x = x and x / 1.0 = x exactly, so bmean and bM2 go through the arithmetic of
    mean and M2 on the same values: equal bit for bit."""
    X = np.random.default_rng(6).standard_normal((9, 1, 13))
    m = BatchMirror(13, 1, 1)
    for cyc in X:
        m.record(list(cyc))
    assert m.nb == 9
    assert np.array_equal(m.bmean, m.mean) and np.array_equal(m.bm2, m.m2)


def test_estimates_on_hand_made_arrays():
    # 4 batches of 6 states; bM2 = 12 -> batch variance 4, stderr sqrt(4 / 4) = 1
    # 24 states with M2 = 46 -> variance 2, iact = 6 * 4 / 2 = 12
    stderr, iact = mg.batch_means_estimates(6, 4, np.array([12.0, 0.0, 3.0]), 24, np.array([46.0, 46.0, 23.0]))
    assert np.array_equal(stderr, [1.0, 0.0, 0.5])
    assert np.array_equal(iact, [12.0, 0.0, 6.0])
    # an uncorrelated series: batch variance = variance / (B K), so iact = 1
    stderr, iact = mg.batch_means_estimates(10, 3, np.array([0.2 * 2]), 30, np.array([2.0 * 29]))
    assert iact[0] == pytest.approx(1.0, rel=1e-15) and stderr[0] == pytest.approx(np.sqrt(0.2 / 3), rel=1e-15)
    # a vertex that never moved has no autocorrelation time
    assert np.isnan(mg.batch_means_estimates(2, 2, np.zeros(1), 4, np.zeros(1))[1][0])


@pytest.mark.parametrize("nb", [0, 1])
def test_estimates_need_two_batches(nb):
    with pytest.raises(ValueError):
        mg.batch_means_estimates(4, nb, np.zeros(3), 4 * nb, np.ones(3))


def test_batch_entry_points_reject_a_null_handle():
    lib = mg.load_library()
    b, nb = ctypes.c_int(), ctypes.c_uint64()
    buf = np.zeros(4)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert lib.mgmc_field_stats_enable_batched(None, 1, 4) == _native.MGMC_E_INVALID
    assert lib.mgmc_field_stats_batch_info(None, ctypes.byref(b), ctypes.byref(nb)) == _native.MGMC_E_INVALID
    assert lib.mgmc_field_stats_get_batch(None, p, p, 4) == _native.MGMC_E_INVALID
    assert "null handle" in _native.last_error()
    assert lib.mgmc_abi_version() == 5


# The slowly mixing chain of the statistical tests (here and in tests/test_gpu_field_batch.py): the prior of a
# 2D 12 x 12 lattice with kappa^2 = 1 on a single level, f = 0; one cycle is the level's symmetric sweep, so the
# smooth modes decay slowly.  Centre vertex, 200 warm-up cycles, 20,000 samples, batches of 250 cycles.
SLOW_SHAPE, SLOW_KAPPA_SQ = (12, 12), 1.0
SLOW_WARMUP, SLOW_N, SLOW_BATCH = 200, 20000, 250


def slow_parameters():
    return mg.MultigridParameters(nlevel=1)


def test_batch_means_tau_agrees_with_the_windowed_estimator_on_the_oracle():
    """20 chain ids of the slow chain on the CPU oracle (the multicolour replay of the device's cycle).  Measured:
    windowed tau of the centre vertex 9.23 on average (8.08 to 10.72), so B = 250 >= 20 tau; batch-means tau minus
    windowed tau: mean +0.59, standard deviation 1.79 over the 20 chains, so the two agree on average within 5
    standard errors of that mean (5 x 1.79 / sqrt(20) = 2.00; the windowed estimator drops the tail of the
    autocorrelation below 0.05, which accounts for a difference of this sign).  The standard deviation is the
    yardstick of the device test (test_tau_at_the_qoi_vertex_against_the_series_estimator)."""
    q = mg.measurement_vector_index(mg.Lattice(*SLOW_SHAPE), [0.5, 0.5])
    diffs, taus = [], []
    for chain in range(20):
        o = oracle_lib.Oracle.fd(SLOW_SHAPE, slow_parameters(), SLOW_KAPPA_SQ, mode=oracle_lib.MULTICOLOUR, seed=SEED,
                                 chain=chain)
        o.sample(SLOW_WARMUP)
        z = o.sample(SLOW_N, q)
        tw, tb = iact_windowed(z), iact_batch_means(z, SLOW_BATCH)
        taus.append(tw)
        diffs.append(tb - tw)
    diffs, taus = np.array(diffs), np.array(taus)
    sd = diffs.std(ddof=1)
    print(f"slow chain: windowed tau mean {taus.mean():.3f} (min {taus.min():.3f}, max {taus.max():.3f}); "
          f"batch-means tau - windowed tau: mean {diffs.mean():+.3f}, sd {sd:.3f} over {len(diffs)} chains")
    assert taus.min() >= 5.0
    assert SLOW_BATCH >= 20 * taus.mean()
    assert abs(diffs.mean()) <= 5 * sd / np.sqrt(len(diffs))
