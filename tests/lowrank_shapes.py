"""Low-rank parts B, Sigma at the documented limits of mgmc_set_lowrank (m = 64, dense and multi-block columns).

TEST INFRASTRUCTURE: helpers only, shared by tests/test_lowrank_shapes_host.py (the CPU oracle against exact algebra)
and tests/test_gpu_lowrank_shapes.py (the device against the oracle).  build(family, shape) returns a
multigridmc_amd.measured.LowRankUpdate for the FD prior on `shape` cells; every builder draws from one numpy
generator seeded with SEED (as tests/test_gpu_lowrank.measured does), Sigma_k = 1e-3 (1 + 2 u), a constant
global-average column gets 0.02.  Each builder asserts on the CSC arrays what its family is there for.

  P64   64 radius-0 columns (value 1.0) at distinct interior vertices: 48 random ones, a patch of 8 mutually adjacent
        vertices (2D 4 x 2, 3D 2 x 2 x 2) and 8 on the first / last interior lines, interior corners included; the 64
        columns in one random order, so that the prefixes below hold some of each kind
  P8, P9, P17   the first 8 / 9 / 17 columns of P64 (lr_small_launch's m <= 8 edge; the second round of the 16-wave
        column loops of k_lr_small and the tail's lr_dots)
  OV64  64 columns; 0, 31, 32, 33 and 63 are ball averages (measurement_vector) with centres 1.5 cells apart along
        x, overlapping, each scaled by its own factor; the other 59 are points away from the balls: rows of B with
        several mask bits, among them bits 31 / 32 / 33 / 63
  DC64  63 points and the constant global average (the cell volume) as column 63: m = 64 on the dense-column path
  BLK   three entry lists of exactly 4096, 4097 and N - 1 sorted random vertices (values normal / sqrt(n)) and a
        point: sparse dots over more than one LR_BLK block; N - 1 entries must stay an entry list
  DV    a point, a dense column of distinct values (normal / sqrt(N)), a point and a ball: the dense-column path with
        a streamed value array (cflag == 0)
  D2    the constant global average, a dense column of distinct values and a point: two dense columns
"""
from __future__ import annotations

import functools

import numpy as np

import multigridmc_amd as mg
from multigridmc_amd.measured import LowRankUpdate, measurement_vector

SEED = 1212417
LR_BLK = 4096  # mgmc_lowrank.hpp
KAPPA_SQ = 25.0
VARIANCE_GLOBAL = 0.02

# name -> (cells, multigrid levels).  F2: N_0 = 6745 > LR_BLK, so a dense column is dense on level 0 and an entry list
# below.  F3: two levels (N_0 = 6555, N_1 = 693); a third would be 60 unknowns under 64 measurements.  FZ: the
# smallest 3D shape found whose level 0 runs k_zsweep_rb7 (asserted where it is used, tests/test_gpu_lowrank_shapes.py)
LATTICES = {"F2": ((96, 72), 3), "F3": ((24, 16, 20), 2), "FZ": ((64, 16, 16), 2)}
# ball radius per lattice: the five OV64 balls, 1.5 cells apart along x, must overlap in rows (asserted in ov64)
BALL_RADIUS = {(96, 72): 0.05, (24, 16, 20): 0.09, (64, 16, 16): 0.09}
OV_COLUMNS = (0, 31, 32, 33, 63)
OV_SCALES = (1.0, 0.75, 1.5, 1.25, 0.5)
FAMILIES = ("P64", "P8", "P9", "P17", "OV64", "DC64", "BLK", "DV", "D2")
SMALL_FAMILIES = ("P64", "P8", "P9", "P17", "OV64")
# the (lattice, family) pairs of the GPU tests; the host test pins the oracle on every one of them
PAIRS = ([("F2", f) for f in FAMILIES] + [("F3", f) for f in ("P64", "P8", "P9", "P17", "OV64", "BLK", "DV", "D2")] +
         [("FZ", f) for f in ("DC64", "DV", "P9")])


def _sigma(rng, m):
    return 1e-3 * (1.0 + 2.0 * rng.random(m))


def _linear(lat, idx):
    return lat.vertexidx_euclidean2linear([int(v) for v in idx])


def _random_vertices(rng, lat, count, exclude):
    """`count` distinct interior vertices (linear indices, in drawing order) outside `exclude`."""
    out, taken = [], set(int(v) for v in exclude)
    while len(out) < count:
        v = int(rng.integers(0, lat.Nvertex))
        if v not in taken:
            taken.add(v)
            out.append(v)
    return out


def _point(v):
    return np.array([v], dtype=np.int64), np.array([1.0])


def _dense_values(rng, n):
    vals = rng.standard_normal(n) / np.sqrt(n)
    assert len(np.unique(vals)) == n and np.all(vals != 0.0)
    return np.arange(n, dtype=np.int64), vals


def _global_average(lat):
    cell_volume = 1.0
    for d in range(lat.dim):
        cell_volume /= float(lat.shape[d])
    return np.arange(lat.Nvertex, dtype=np.int64), np.full(lat.Nvertex, cell_volume)


def column_lengths(lr):
    return np.diff(lr.colptr)


def constant_columns(lr):
    """Per column: all its stored values are one bit pattern."""
    out = []
    for k in range(lr.m):
        v = lr.vals[lr.colptr[k]:lr.colptr[k + 1]].view(np.uint64)
        out.append(bool(len(v)) and bool(np.all(v == v[0])))
    return out


def row_masks(lr):
    """Per row of B its 64-bit column mask (bit k: B_ik stored), as mgmc_lowrank_setup.hip builds rows_mask."""
    mask = np.zeros(lr.n, dtype=np.uint64)
    for k in range(lr.m):
        mask[lr.rows[lr.colptr[k]:lr.colptr[k + 1]]] |= np.uint64(1) << np.uint64(k)
    return mask


def _bits(columns):
    return np.uint64(sum(1 << k for k in columns))


def _p64_sites(rng, lat):
    n = lat.shape
    o = [v // 2 for v in n]  # the patch's lowest corner
    if lat.dim == 2:
        patch = [(o[0] + a, o[1] + b) for b in range(2) for a in range(4)]
        hi = (n[0] - 1, n[1] - 1)
        edge = [(1, 1), (hi[0], 1), (1, hi[1]), hi, (n[0] // 3, 1), (hi[0], n[1] // 3), (1, 2 * n[1] // 3),
                (2 * n[0] // 3, hi[1])]
    else:
        patch = [(o[0] + a, o[1] + b, o[2] + c) for c in range(2) for b in range(2) for a in range(2)]
        hi = (n[0] - 1, n[1] - 1, n[2] - 1)
        edge = [(1, 1, 1), hi, (hi[0], 1, 1), (1, hi[1], hi[2]), (n[0] // 3, 1, n[2] // 2), (hi[0], n[1] // 3, 1),
                (1, hi[1], n[2] // 3), (2 * n[0] // 3, n[1] // 2, hi[2])]
    fixed = [_linear(lat, p) for p in patch + edge]
    assert len(set(fixed)) == 16
    sites = _random_vertices(rng, lat, 48, fixed) + fixed
    return [sites[q] for q in rng.permutation(64)]


def p64(lat, m=64):
    rng = np.random.default_rng(SEED)
    sites = _p64_sites(rng, lat)
    sigma = _sigma(rng, 64)
    assert len(set(sites)) == 64
    lr = LowRankUpdate.from_columns(lat.Nvertex, [_point(v) for v in sites[:m]], sigma[:m])
    assert lr.m == m and np.all(column_lengths(lr) == 1)
    return lr


def ball_centres(lat):
    """Five centres 1.5 cells apart along x around the middle of the lattice, off the vertices in every direction."""
    h = [1.0 / n for n in lat.shape]
    base = [(lat.shape[d] // 2 + 0.25) * h[d] for d in range(lat.dim)]
    return [[base[0] + (q - 2) * 1.5 * h[0]] + base[1:] for q in range(5)]


def _away_from(lat, centres, distance):
    """The vertices within `distance` of one of the centres."""
    xyz = np.array([lat.vertex_coordinates(v) for v in range(lat.Nvertex)])
    near = np.zeros(lat.Nvertex, dtype=bool)
    for c in centres:
        near |= np.sqrt(((xyz - np.asarray(c)) ** 2).sum(axis=1)) < distance
    return np.flatnonzero(near)


def ov64(lat):
    rng = np.random.default_rng(SEED)
    radius = BALL_RADIUS[lat.shape]
    centres = ball_centres(lat)
    points = iter(_random_vertices(rng, lat, 59, _away_from(lat, centres, 2.0 * radius)))
    balls = {}
    for k, c, scale in zip(OV_COLUMNS, centres, OV_SCALES):
        rows, vals = measurement_vector(lat, c, radius)
        balls[k] = (rows, scale * vals)
    lr = LowRankUpdate.from_columns(lat.Nvertex, [balls[k] if k in balls else _point(next(points)) for k in range(64)],
                                    _sigma(rng, 64))
    mask = row_masks(lr)
    nbits = np.array([bin(int(v)).count("1") for v in mask])
    both = [int(np.count_nonzero((mask & _bits(c)) == _bits(c))) for c in ((0, 31, 32, 33), (32, 33, 63))]
    assert both[0] > 0 or both[1] > 0, f"no row of B carries bits 0/31/32/33 or 32/33/63 together (radius {radius})"
    assert nbits.max() >= 3
    lens = column_lengths(lr)
    assert all(lens[k] > 1 for k in OV_COLUMNS) and np.count_nonzero(lens == 1) == 59
    return lr


def dc64(lat):
    rng = np.random.default_rng(SEED)
    cols = [_point(v) for v in _random_vertices(rng, lat, 63, ())] + [_global_average(lat)]
    sigma = np.append(_sigma(rng, 63), VARIANCE_GLOBAL)
    lr = LowRankUpdate.from_columns(lat.Nvertex, cols, sigma)
    lens, const = column_lengths(lr), constant_columns(lr)
    assert lr.m == 64 and np.flatnonzero(lens == lat.Nvertex).tolist() == [63] and const[63]
    return lr


def blk(lat):
    rng = np.random.default_rng(SEED)
    n = lat.Nvertex
    assert n - 1 > LR_BLK + 1
    cols = []
    for count in (LR_BLK, LR_BLK + 1, n - 1):
        rows = np.sort(rng.choice(n, size=count, replace=False)).astype(np.int64)
        cols.append((rows, rng.standard_normal(count) / np.sqrt(count)))
    cols.append(_point(_random_vertices(rng, lat, 1, ())[0]))
    lr = LowRankUpdate.from_columns(n, cols, _sigma(rng, 4))
    assert column_lengths(lr).tolist() == [LR_BLK, LR_BLK + 1, n - 1, 1]  # no column has N entries: none is dense
    return lr


def dv(lat):
    rng = np.random.default_rng(SEED)
    n = lat.Nvertex
    centre = ball_centres(lat)[2]
    pts = _random_vertices(rng, lat, 2, _away_from(lat, [centre], 2.0 * BALL_RADIUS[lat.shape]))
    cols = [_point(pts[0]), _dense_values(rng, n), _point(pts[1]), measurement_vector(lat, centre, BALL_RADIUS[lat.shape])]
    lr = LowRankUpdate.from_columns(n, cols, _sigma(rng, 4))
    lens, const = column_lengths(lr), constant_columns(lr)
    assert np.flatnonzero(lens == n).tolist() == [1] and not const[1] and 1 < lens[3] < n
    return lr


def d2(lat):
    rng = np.random.default_rng(SEED)
    n = lat.Nvertex
    cols = [_global_average(lat), _dense_values(rng, n), _point(_random_vertices(rng, lat, 1, ())[0])]
    sigma = _sigma(rng, 3)
    sigma[0] = VARIANCE_GLOBAL
    lr = LowRankUpdate.from_columns(n, cols, sigma)
    lens, const = column_lengths(lr), constant_columns(lr)
    assert np.flatnonzero(lens == n).tolist() == [0, 1] and const[0] and not const[1]
    return lr


_BUILDERS = {"P64": p64, "P8": lambda lat: p64(lat, 8), "P9": lambda lat: p64(lat, 9), "P17": lambda lat: p64(lat, 17),
             "OV64": ov64, "DC64": dc64, "BLK": blk, "DV": dv, "D2": d2}


@functools.lru_cache(maxsize=None)
def build(family, shape):
    """The family's LowRankUpdate on `shape` cells (cached: treat it as read-only)."""
    lr = _BUILDERS[family](mg.Lattice(*shape))
    for a in (lr.colptr, lr.rows, lr.vals, lr.sigma):
        a.setflags(write=False)
    return lr


def params(lattice, **kw):
    shape, nlevel = LATTICES[lattice]
    return mg.MultigridParameters(**{"nlevel": nlevel, "smoother": "SOR", "coarse_solver": "SSOR", **kw})


def problem(lattice, family, **kw):
    """tests.algebra.Problem of a (lattice, family) pair: FD prior, kappa^2 = 25."""
    from tests import algebra as AL
    shape, nlevel = LATTICES[lattice]
    return AL.Problem("fd", shape, {"nlevel": nlevel, **kw}, meas=lambda lat: build(family, lat.shape),
                      kappa_sq=KAPPA_SQ)


def split_columns(colptr_rows_vals, nrows):
    """The split column of a level, from its CSC columns alone: the level's only column with N entries, over more
    than LR_BLK rows, all values one bit pattern (LowRankDev::split_g; the oracle's LowRank::split); else None."""
    colptr, rows, vals = colptr_rows_vals
    full = [k for k in range(len(colptr) - 1) if colptr[k + 1] - colptr[k] == nrows]
    if nrows <= LR_BLK or len(full) != 1:
        return None
    v = np.ascontiguousarray(vals[colptr[full[0]]:colptr[full[0] + 1]]).view(np.uint64)
    return full[0] if bool(np.all(v == v[0])) else None
