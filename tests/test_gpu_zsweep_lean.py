"""The zero-right-hand-side fine z-sweeps after their instruction diet, bit for bit against the CPU oracle (-m gpu).

The two FZ instances of k_zsweep_rb7 (mgmc_zsweep.hpp) issue fewer vector instructions per pair than they did: the
fused-prolongation sweep runs its two colour sections compiled per first-colour element under a wave-uniform branch
(BranchE0), and the noise routine builds its uniforms and clamps its radius with fewer instructions
(philox_normal.h).  None of that may change a bit.  Every case asserts through
level_kernels(0) that level 0 runs k_zsweep_rb7 with the fused-prolongation post-sweep and rhs=zero, then compares
uint64 views with the MULTICOLOUR oracle.

The lattices are the smallest that reach every branch the change touches (the oracle was run on each on the CPU
first; they take 0.1 s, the 20-row one 2 s):

  * nx must be a multiple of 64 for level 0 to take the z-sweep at all (mgmc_level_plan.hpp), so there is no partial
    x tile; 128 gives two x tiles whose halo columns overlap.
  * ny = 36: 35 interior rows = two 16-row tiles and one of 3 rows.  In that last tile the core waves 2 .. 7 have
    both their rows past ny - 1 (they take the sections' branches with no interior lane); wave 1 (rows 34, 36) has
    one row in and one out.
  * Below 256^3 every z-chunk is 8 planes deep (zsweep_depth).  nz is even, so a last chunk has 1, 3, 5 or 7 planes:
    nz = 18 gives 8 + 8 + 1 (a last chunk of one plane, 3 steps; the pre-sweep's chunk pairs get an empty fourth
    tile), nz = 22 gives 8 + 8 + 5 and nz = 20 (the three-level case: nz % 4 == 0) 8 + 8 + 3.  A full chunk marches
    10 steps (2 mod 4), the partial ones 3, 5 and 7.
  * The 20-row plain sweep of the 512^3 benchmark needs 512 tiles: 128 x 84 x 416 (test_gpu_rhs_zero.py), whose 83
    interior rows leave 3 in the fifth 20-row tile (core waves 2 .. 9 wholly outside) and 3 in the sixth 16-row tile
    of the post-sweep.
  * SOR sweeps forward only (first colour 0); SSOR adds the backward sweeps (first colour 1), so both values of the
    first-colour element are taken on every plane parity and row parity.
  * coarse_scaling 1.0 is a power of two (PROLONG = 2, fma terms), 0.75 is not (PROLONG = 1).
"""
import functools

import numpy as np
import pytest

import multigridmc_amd as mg
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 5418513
KAPPA_SQ = 25.0

SOR1 = dict(nlevel=2, coarse_scaling=1.0)
SSOR1 = dict(nlevel=2, smoother="SSOR", npresmooth=2, omega=1.1, coarse_scaling=1.0)
SSOR075 = dict(nlevel=2, smoother="SSOR", npresmooth=2, omega=1.1, coarse_scaling=0.75)
# name: shape, parameters, samples, level 0's "sweep" label
CASES = {
    "64x36x18_sor_cs1": ((64, 36, 18), SOR1, 3, "k_zsweep_rb7<32,16,...,0>"),
    "64x36x18_ssor_cs075": ((64, 36, 18), SSOR075, 3, "k_zsweep_rb7<32,16,...,0>"),
    "128x36x22_ssor_cs1": ((128, 36, 22), SSOR1, 3, "k_zsweep_rb7<32,16,...,0>"),
    "128x36x22_sor_cs075": ((128, 36, 22), dict(SOR1, coarse_scaling=0.75), 3, "k_zsweep_rb7<32,16,...,0>"),
    "128x84x416_ssor_cs1_20rows": ((128, 84, 416), SSOR1, 2, "k_zsweep_rb7<32,20,...,0>"),
    # one whole three-level V-cycle per sample, a QoI series of three
    "64x36x20_3lvl": ((64, 36, 20), dict(nlevel=3, coarse_scaling=1.0), 3, "k_zsweep_rb7<32,16,...,0>"),
}


def params(**kw):
    return mg.MultigridParameters(**{"smoother": "SOR", "coarse_solver": "SSOR", **kw})


def make(shape, kw, chain=0, nchains=1):
    p = params(**kw)
    lat = mg.Lattice(*shape)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, KAPPA_SQ), SEED, p, device=0, chain_id=chain,
                              nchains=nchains)
    return s, p, lat


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def start_state(lat):
    return 0.01 * np.random.default_rng(12).standard_normal(lat.Nvertex)


def centre(lat):
    return mg.measurement_vector_index(lat, [0.5] * lat.dim)


@functools.lru_cache(maxsize=None)
def oracle_chain(name, chain=0):
    """(QoI series, final state) of the oracle from f = +0, computed once per case and chain and left unchanged"""
    shape, kw, nsamples, _ = CASES[name]
    p, lat = params(**kw), mg.Lattice(*shape)
    O.set_threads(min(16, O.cpu_share()))
    try:
        mc = O.Oracle.fd_own(lat.shape, p, KAPPA_SQ, mode=O.MULTICOLOUR, seed=SEED, chain=chain)
        mc.set_rhs(np.zeros(lat.Nvertex))
        mc.set_state(start_state(lat))
        mc.set_sample_index(7)
        z = mc.sample(nsamples, centre(lat))
        x = mc.get_state()
    finally:
        O.set_threads(1)
    z.setflags(write=False)
    x.setflags(write=False)
    return z, x


def assert_lean_labels(s, sweep, zero=True):
    k = s.level_kernels(0)
    assert k["sweep"] == sweep, k
    assert k.get("post_sweep", "").startswith("k_zsweep_rb7<") and k["post_sweep"].endswith("PROLONG>"), k
    assert (k.get("rhs") == "zero") == zero, k


def run_chain(s, lat, f, nsamples, chain=0):
    s.fix_rhs(f)
    s.set_state(start_state(lat))
    s.set_sample_index(7)
    return s.sample(nsamples, centre(lat)), s.get_state()


@pytest.mark.parametrize("name", list(CASES))
def test_zero_f_cycles_bitwise(hip_device, name):
    """Prior cycles from f = 0: QoI series and final state against the oracle."""
    shape, kw, nsamples, sweep = CASES[name]
    s, p, lat = make(shape, kw)
    assert_lean_labels(s, sweep)
    z, x = run_chain(s, lat, np.zeros(lat.Nvertex), nsamples)
    assert_lean_labels(s, sweep)
    zo, xo = oracle_chain(name)
    assert np.all(np.isfinite(x))
    assert same_bits(z, zo), (name, z, zo)
    assert same_bits(x, xo), (name, int(np.count_nonzero(bits(x) != bits(xo))))
    s.close()


@pytest.mark.parametrize("name", ["64x36x18_sor_cs1", "64x36x18_ssor_cs075", "128x36x22_ssor_cs1"])
def test_zero_f_cycles_on_poisoned_lds_bitwise(hip_device, monkeypatch, name):
    """The same chains with NaN in every compute unit's LDS before every launch (MGMC_POISON, read at creation): a
    section that read a ring slot, a table entry or the coarse ring before its barrier would compute with NaN."""
    monkeypatch.setenv("MGMC_POISON", "1")
    shape, kw, nsamples, sweep = CASES[name]
    s, p, lat = make(shape, kw)
    assert_lean_labels(s, sweep)
    z, x = run_chain(s, lat, np.zeros(lat.Nvertex), nsamples)
    zo, xo = oracle_chain(name)
    assert np.all(np.isfinite(x))
    assert same_bits(z, zo) and same_bits(x, xo)
    s.close()


def test_batched_handle_bitwise(hip_device):
    """nchains = 2 (blockIdx.z picks the chain and its Philox key): each chain against the oracle's."""
    name = "64x36x18_ssor_cs075"
    shape, kw, nsamples, sweep = CASES[name]
    batch, p, lat = make(shape, kw, nchains=2)
    assert_lean_labels(batch, sweep)
    batch.fix_rhs(np.zeros(lat.Nvertex))
    batch.set_state(start_state(lat))
    batch.set_sample_index(7)
    zb = batch.sample(nsamples, centre(lat), chain=None)
    xb = batch.get_state(None)
    assert_lean_labels(batch, sweep)
    for c in range(2):
        zo, xo = oracle_chain(name, c)
        assert same_bits(zb[c], zo) and same_bits(xb[c], xo), c
    batch.close()


@pytest.mark.parametrize("name", ["64x36x18_ssor_cs075", "128x36x22_ssor_cs1"])
def test_control_rhs_takes_general_instances_same_chain(hip_device, name):
    """Zeros with one -0.0 are not all-bits-zero: the general instances (one copy of the post-sweep's march, with
    selects) run, and give the chain of the zero instances and of the oracle."""
    shape, kw, nsamples, sweep = CASES[name]
    s, p, lat = make(shape, kw)
    f = np.zeros(lat.Nvertex)
    f[lat.Nvertex - 1] = -0.0
    z, x = run_chain(s, lat, f, nsamples)
    assert_lean_labels(s, sweep, zero=False)
    zo, xo = oracle_chain(name)
    assert same_bits(z, zo) and same_bits(x, xo)
    s.close()
