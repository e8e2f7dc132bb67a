"""The fine level's zero right-hand side taken as a constant (-m gpu).

Prior sampling has f = A 0 = 0 on level 0.  While every chain's f is all-bits-zero the cycle's fine
z-marching sweeps and the 7-point z-marching residual + restriction run instances that do not load f
(level_kernels(0)["rhs"] == "zero"); the chain is the same bit for bit.

The control is data, not a switch: a right-hand side of zeros with one -0.0 entry is not all-bits-zero, so
it takes the general instances, and it gives the same chain bit for bit (f only enters as
c = fma(sd, z, f) and r = f - A x: a -0.0 changes a bit only where sd z or A x is exactly zero as well).
For every shape used here the MULTICOLOUR oracle was run on the CPU with +0 and with one -0.0
(x0 = 0.01 N(0,1) from default_rng(12), sample index 7, 3 samples): identical QoI series and final state
(compared as uint64).  The tests below assert it again on the device: A (zeros) == B (one -0.0) == oracle.
"""
import functools

import numpy as np
import pytest

import multigridmc_amd as mg
from multigridmc_amd.parameters import MeasurementParameters
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 5418513
KAPPA_SQ = 25.0

SSOR = dict(smoother="SSOR", npresmooth=2, omega=1.1, coarse_scaling=0.9)
# the smallest lattices that reach each path (nx % 64 == 0 puts level 0 on the z-sweep)
SHAPES = {
    # partial y tiles, an up / down z-chunk pair with a short second chunk
    "64x44x40": ((64, 44, 40), dict(nlevel=2)),
    "192x48x40": ((192, 48, 40), dict(nlevel=2)),
    # backward direction, an alpha that is no power of two (the PROLONG = 1 instance), the copy back
    "128x36x24_ssor": ((128, 36, 24), dict(nlevel=2, **SSOR)),
    # the <7,64,4,256> residual + restriction with partial tiles
    "256x40x48": ((256, 40, 48), dict(nlevel=2)),
    # the zero-f instances above a hierarchy of three-load window quad passes (48- and 24-pair rows) and a tail
    "192x48x48_5lvl": ((192, 48, 48), dict(nlevel=5)),
}


def params(**kw):
    return mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **kw})


def make(shape, chain=0, nchains=1, **kw):
    p = params(**kw)
    lat = mg.Lattice(*shape)
    s = mg.MultigridMCSampler(mg.ShiftedLaplaceFDOperator(lat, KAPPA_SQ), SEED, p, device=0, chain_id=chain,
                              nchains=nchains)
    return s, p, lat


def oracle_for(p, lat, chain=0):
    return O.Oracle.fd_own(lat.shape, p, KAPPA_SQ, mode=O.MULTICOLOUR, seed=SEED, chain=chain)


def start_state(lat):
    return 0.01 * np.random.default_rng(12).standard_normal(lat.Nvertex)


def zeros_with(lat, index=None, value=-0.0):
    f = np.zeros(lat.Nvertex)
    if index is not None:
        f[index] = value
    return f


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def centre(lat):
    return mg.measurement_vector_index(lat, [0.5] * lat.dim)


def run_chain(s, lat, f, nsamples):
    """fix_rhs(f), the common start state, sample index 7, nsamples cycles: (series, state)"""
    s.fix_rhs(f)
    s.set_state(start_state(lat))
    s.set_sample_index(7)
    z = s.sample(nsamples, centre(lat))
    return z, s.get_state()


@functools.lru_cache(maxsize=None)
def oracle_chain(name):
    """the oracle's 3 samples from f = +0 (computed once per shape)"""
    shape, kw = SHAPES[name]
    p, lat = params(**kw), mg.Lattice(*shape)
    mc = oracle_for(p, lat)
    mc.set_rhs(np.zeros(lat.Nvertex))
    mc.set_state(start_state(lat))
    mc.set_sample_index(7)
    z = mc.sample(3, centre(lat))
    return z, mc.get_state()


def has_zero_label(s):
    return s.level_kernels(0).get("rhs") == "zero"


@pytest.mark.parametrize("name", list(SHAPES))
def test_zero_path_equals_control_and_oracle(hip_device, name):
    """Handle A (f = zeros: the zero instances) against handle B (zeros with one -0.0 at the last vertex: the
    general instances) and against the oracle: series and state bitwise."""
    shape, kw = SHAPES[name]
    a, p, lat = make(shape, **kw)
    b = make(shape, **kw)[0]
    za, xa = run_chain(a, lat, zeros_with(lat), 3)
    zb, xb = run_chain(b, lat, zeros_with(lat, lat.Nvertex - 1), 3)
    assert a.level_kernels(0).get("rhs") == "zero"
    assert "rhs" not in b.level_kernels(0)
    assert all("rhs" not in a.level_kernels(l) for l in range(1, p.nlevel))
    zo, xo = oracle_chain(name)
    assert same_bits(za, zb) and same_bits(xa, xb)
    assert same_bits(za, zo) and same_bits(xa, xo)
    a.close()
    b.close()


def test_plain_20_row_instance(hip_device):
    """At small sizes the plain sweep runs the 16-row tiles; this lattice is just large enough (520 tiles of 20
    rows >= the 512 workgroup slots) for the 20-row instance the 512^3 benchmark runs.  A against B on the
    device, 2 samples (the oracle covers this instance at 512^3 in test_gpu_headline.py)."""
    shape, kw = (128, 84, 416), dict(nlevel=2)
    a, p, lat = make(shape, **kw)
    b = make(shape, **kw)[0]
    assert a.level_kernels(0)["sweep"] == "k_zsweep_rb7<32,20,...,0>"
    za, xa = run_chain(a, lat, zeros_with(lat), 2)
    zb, xb = run_chain(b, lat, zeros_with(lat, lat.Nvertex - 1), 2)
    assert has_zero_label(a) and "rhs" not in b.level_kernels(0)
    assert a.level_kernels(0)["sweep"] == b.level_kernels(0)["sweep"] == "k_zsweep_rb7<32,20,...,0>"
    assert same_bits(za, zb) and same_bits(xa, xb)
    a.close()
    b.close()


def test_flips_on_one_handle(hip_device):
    """zero -> random -> zero -> mgmc_apply(zeros) -> mgmc_apply(random) on one handle: the label follows f and
    every step equals the oracle fed the same sequence (the graph rebuild, the detection, the apply path)."""
    shape, kw = SHAPES["64x44x40"]
    s, p, lat = make(shape, **kw)
    mc = oracle_for(p, lat)
    q = centre(lat)
    rng = np.random.default_rng(21)
    f1, f2 = rng.standard_normal(lat.Nvertex), rng.standard_normal(lat.Nvertex)
    zero = np.zeros(lat.Nvertex)

    def step(n):
        assert same_bits(s.sample(n, q), mc.sample(n, q))
        assert same_bits(s.get_state(), mc.get_state())

    assert has_zero_label(s)  # a fresh handle: f is the creation's memset
    s.set_state(start_state(lat))
    mc.set_rhs(zero)
    mc.set_state(start_state(lat))
    step(2)
    s.fix_rhs(f1)
    mc.set_rhs(f1)
    assert "rhs" not in s.level_kernels(0)
    step(2)
    s.fix_rhs(zero)
    mc.set_rhs(zero)
    assert has_zero_label(s)
    step(2)
    s.unfix_rhs()  # apply() uploads its f again: mgmc_apply
    xd, xo = s.get_state(), mc.get_state()
    s.apply(zero, xd)
    mc.apply(zero, xo)
    assert has_zero_label(s) and same_bits(xd, xo)
    s.apply(f2, xd)
    mc.apply(f2, xo)
    assert "rhs" not in s.level_kernels(0) and same_bits(xd, xo)
    s.apply(zero, xd)
    mc.apply(zero, xo)
    assert has_zero_label(s) and same_bits(xd, xo)
    s.close()


def test_timed_graph(hip_device):
    """graph_timed is rebuilt with the zero instances too: sample_timed on a zero-f handle gives the chain of
    sample on a second one."""
    shape, kw = SHAPES["64x44x40"]
    s, p, lat = make(shape, **kw)
    t = make(shape, **kw)[0]
    q = centre(lat)
    for h in (s, t):
        h.fix_rhs(np.random.default_rng(4).standard_normal(lat.Nvertex))  # away from the creation's state
        h.fix_rhs(zeros_with(lat))
        h.set_state(start_state(lat))
        assert has_zero_label(h)
    r = s.sample_timed(5, q, stride=2)
    assert r["npre"] > 0 and r["npost"] > 0
    assert same_bits(s.get_series(5), t.sample(5, q))
    assert same_bits(s.get_state(), t.get_state())
    s.close()
    t.close()


def test_batched_chains(hip_device):
    """nchains = 2 with f = 0 equals two single-chain handles with chain_id 0 and 1."""
    shape, kw = SHAPES["64x44x40"]
    batch, p, lat = make(shape, nchains=2, **kw)
    q = centre(lat)
    assert has_zero_label(batch)
    batch.fix_rhs(zeros_with(lat))
    assert has_zero_label(batch)
    batch.set_state(start_state(lat))
    batch.set_sample_index(7)
    zb = batch.sample(3, q, chain=None)
    xb = batch.get_state(None)
    for c in range(2):
        one = make(shape, chain=c, **kw)[0]
        z, x = run_chain(one, lat, zeros_with(lat), 3)
        assert has_zero_label(one)
        assert same_bits(zb[c], z) and same_bits(xb[c], x)
        one.close()
    batch.close()


def test_posterior_level_keeps_general_instances(hip_device):
    """A level with a low-rank part patches its f: no rhs=zero with f = 0, the cycle equals the oracle's; dropping
    the low-rank part brings the zero instances back."""
    shape, kw = SHAPES["64x44x40"]
    rng = np.random.default_rng(1212417)
    lat = mg.Lattice(*shape)
    mp = MeasurementParameters(radius=0.0, variance_scaling=1e-3, measure_global=False, variance_global=0.02)
    mp.measurement_locations = [list(rng.uniform(0.15, 0.85, 3)) for _ in range(3)]
    mp.variance = list(1.0 + 2.0 * rng.random(3))
    op = mg.MeasuredOperator(mg.ShiftedLaplaceFDOperator(lat, KAPPA_SQ), mp)
    s, p, lat = make(shape, **kw)
    assert has_zero_label(s)
    s.set_lowrank(op.get_B())
    assert "rhs" not in s.level_kernels(0) and "lowrank" in s.level_kernels(0)
    mc = oracle_for(p, lat)
    mc.set_lowrank(op.get_B())
    mc.set_rhs(np.zeros(lat.Nvertex))
    mc.set_state(start_state(lat))
    mc.set_sample_index(7)
    z, x = run_chain(s, lat, zeros_with(lat), 3)
    assert "rhs" not in s.level_kernels(0)
    assert same_bits(z, mc.sample(3, centre(lat))) and same_bits(x, mc.get_state())
    s.set_lowrank(None)
    assert has_zero_label(s)
    zo, xo = oracle_chain("64x44x40")
    z, x = run_chain(s, lat, zeros_with(lat), 3)
    assert same_bits(z, zo) and same_bits(x, xo)
    s.close()


@pytest.mark.parametrize("index,value", [(0, -0.0), (-1, 5e-324)], ids=["minus_zero_first", "denormal_last"])
def test_zero_looking_values_are_not_zero(hip_device, index, value):
    """-0.0 (here at the first vertex) and a denormal have bits set: the general instances."""
    shape, kw = SHAPES["64x44x40"]
    s, p, lat = make(shape, **kw)
    assert has_zero_label(s)
    s.fix_rhs(zeros_with(lat, index, value))
    assert "rhs" not in s.level_kernels(0)
    s.fix_rhs(zeros_with(lat))
    assert has_zero_label(s)
    s.close()
