"""The CPU oracle's MULTICOLOUR replay against exact algebra at the low-rank shapes of tests/lowrank_shapes.py (no GPU).

tests/test_gpu_lowrank_shapes.py compares the device with the oracle bit for bit at m = 64, with rows of B that carry
several mask bits, with entry lists over more than one block, with a dense column of distinct values and with two
dense columns.  These tests pin the oracle itself at the same (lattice, family) pairs, so that the comparison is
against something checked independently: every sweep is the SOR splitting of Q = A + B Sigma^-1 B^T with unit noise
(identities A and B of tests/algebra.py, both directions, every level, bound C_TOL = 8), the residual + restriction
is P^T (f - Q x), the coarse columns are P^T B_(l-1), and the split column of lr_row_patch -- stated here from the
columns alone -- is taken on level 0 of DC64 and nowhere in BLK, DV and D2.

The bound's scale.  With the scale s of tests/algebra.py as it was, the oracle's largest ratios were (cases of this
file, per lattice; the bound is 8)
              P64    P17    OV64   DC64   others
    F2        65.1   3.35   13.5   9.97   <= 3.2
    F3        23.8   7.85   14.4   -      <= 4.7
    FZ        -      -      -      3.86   <= 4.1
each worst on the coarsest level (391 / 693 unknowns under 64 measurements), at vertices that carry several entries
of the restricted B (8 at the worst vertex of F2 P64): s held the rounding of x' = y - u but not the rounding inside
u = B_bar (B^T y), an m-term fma chain against the stored B_bar = Y K^-1 that cancels where the columns of Y overlap.
LevelAlgebra._lowrank_terms now adds gamma_m |M~| |B_bar| |B^T y|, B_bar and K assembled on the host in extended
precision from B, Sigma and the splitting (LevelAlgebra._bbar).  K is well conditioned in every case (cond(K) <=
5.3e3), so no input was moved.  The term only enlarges s, so no earlier ratio can grow: of the cases of
tests/test_algebra_host.py the two with a low-rank part went from 0.57 / 0.85 / 0.78 to 0.45 / 0.68 / 0.34
(2d32_point_global) and from 0.08 / 0.21 / 0.12 to 0.07 / 0.15 / 0.11 (3d32_ball_global); the others have no such term.

Largest ratio measured on the oracle with the term, A / B / A and B at once (bound 8):
    F2 P64 2.11 / 3.17 / 2.35    F2 P8 2.22 / 3.17 / 2.35     F2 P9 2.22 / 3.17 / 2.35    F2 P17 2.11 / 3.17 / 2.35
    F2 OV64 2.11 / 3.17 / 2.35   F2 DC64 0.61 / 0.17 / 0.20   F2 BLK 0.00 / 0.00 / 0.00   F2 DV 0.06 / 0.07 / 0.02
    F2 D2 0.05 / 0.08 / 0.01     F3 P64 2.03 / 3.55 / 2.61    F3 P8 2.47 / 4.70 / 2.61    F3 P9 2.47 / 4.70 / 2.61
    F3 P17 2.18 / 4.70 / 2.61    F3 OV64 2.03 / 3.55 / 2.61   F3 BLK 0.00 / 0.00 / 0.00   F3 DV 0.01 / 0.01 / 0.00
    F3 D2 0.16 / 0.37 / 0.27     FZ DC64 0.95 / 0.09 / 0.13   FZ DV 0.00 / 0.02 / 0.01    FZ P9 2.24 / 4.09 / 2.50
(the figures shared by the point families are those of vertices away from every measurement; a dense column's dots
carry their length, 6555 .. 14175, in s, hence the small ratios of BLK, DV and D2).
Residuals (bound: largest row of A + 1 + 3^d + fullest row of B + 2 = 18 .. 41): at most 3.29 (F3 OV64, level 0);
0.00 in BLK, DV and D2.
"""
import functools

import numpy as np
import pytest

from tests import algebra as AL
from tests import lowrank_shapes as LS

SEED = 5418513 + (7 << 32)
CHAIN = 5
TAG = 3
SAMPLE = (1 << 32) + 17
IDS = [f"{lat}-{fam}" for lat, fam in LS.PAIRS]


@functools.lru_cache(maxsize=None)
def case(lattice, family):
    """(problem, MULTICOLOUR oracle, level algebras) of a pair, built once for the tests of this file."""
    prob = LS.problem(lattice, family)
    return prob, prob.oracle(seed=SEED, chain=CHAIN), AL.level_algebras(prob)


@pytest.mark.parametrize("lattice,family", LS.PAIRS, ids=IDS)
def test_oracle_sweeps_are_the_sor_splitting_with_unit_noise(lattice, family):
    """A and B on every level, both directions."""
    prob, be, las = case(lattice, family)
    ratios = AL.check_sweeps(prob, be, AL.oracle_normals(SEED, CHAIN), TAG, SAMPLE, np.random.default_rng(1),
                             algebras=las)
    worst = AL.report(f"{lattice} {family}", ratios)
    assert worst <= AL.C_TOL, ratios


@pytest.mark.parametrize("lattice,family", LS.PAIRS, ids=IDS)
def test_oracle_residuals_are_the_restricted_posterior_residual(lattice, family):
    """R with Q_l = A_l + B_l Sigma^-1 B_l^T on every level that has a coarser one."""
    prob, be, las = case(lattice, family)
    out = AL.check_residuals(prob, be, np.random.default_rng(8), las)
    assert len(out) == prob.params.nlevel - 1
    for level, (ratio, bound) in out.items():
        assert ratio <= bound, (level, ratio, bound)


@pytest.mark.parametrize("lattice,family", LS.PAIRS, ids=IDS)
def test_oracle_coarse_columns_are_the_restricted_columns(lattice, family):
    """B_l = P^T B_(l-1), P assembled from its definition, against the oracle's columns on every level."""
    prob, mc, _ = case(lattice, family)
    lr = prob.lowrank()
    for level, (B, sig, cnt) in enumerate(prob.lowrank_levels()):
        colptr, rows, vals = mc.lowrank(level)
        ref = AL.sp.csc_matrix((vals, rows, colptr), shape=B.shape)
        assert abs(ref - B).max() <= 4 * AL.EPS * abs(ref).max(), level
        assert np.array_equal(cnt, np.diff(colptr)) and np.array_equal(sig, lr.sigma), level


@pytest.mark.parametrize("lattice,family", LS.PAIRS, ids=IDS)
def test_split_column_rule_from_the_columns(lattice, family):
    """The split column of every level -- the level's only column with N entries, over more than 4096 rows, all values
    one bit pattern -- stated from the oracle's columns and the level sizes: column 63 on level 0 of DC64, none on
    any level of the other families (DV: the column's values differ; D2: two such columns; BLK: N - 1 entries;
    below level 0 no level has more than 4096 rows)."""
    prob, mc, las = case(lattice, family)
    split = [LS.split_columns(mc.lowrank(level), las[level].n) for level in range(prob.params.nlevel)]
    print(f"split columns {lattice} {family}: {split}  level sizes {[la.n for la in las]}")
    assert las[0].n > LS.LR_BLK and all(la.n <= LS.LR_BLK for la in las[1:])
    assert split == ([63] if family == "DC64" else [None]) + [None] * (prob.params.nlevel - 1)
