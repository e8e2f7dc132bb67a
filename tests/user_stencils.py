"""Constant-coefficient stencils that are NOT the shifted-Laplace family, for the user-stencil parity tests
(tests/test_user_stencil_host.py, tests/test_gpu_user_stencil.py).

TEST INFRASTRUCTURE.  Every stencil is a function returning the 27-entry (3D) or 9-entry (2D) array in
mgmc_level_desc.stencil order, index (dz+1)*9 + (dy+1)*3 + (dx+1) / (dy+1)*3 + (dx+1).  The FD / FEM stencils and
their Galerkin products have mirror partners a(-d), a(+d) that are equal or one ulp apart, so a kernel that reads
a mirrored or permuted coefficient passes most bitwise tests on them; here

  C27, C9   every off-centre entry distinct, -(0.25 + U), U in [0,1); centre 34 / 11 (rows strictly diagonally
            dominant whatever the draw: 26 * 1.25 = 32.5 < 34, 8 * 1.25 = 10 < 11); no symmetry of any kind
  C7, C5    axis neighbours only, -(0.5 + U), all distinct (a(-x) != a(+x)); centre 9.5 / 6.5
  S7        dyadic, anisotropic, FD-symmetric: x -1, y -2, z -4, centre 16
  S27       dyadic and reflection-symmetric: -w(|d|_1) (1 + [dz != 0] / 2) (1 + [dy != 0] / 4), w = 1, 1/2, 1/4,
            centre 24: 8 distinct fold classes; dyadic, so every Galerkin level is exact and stays bitwise
            reflection-symmetric
  P27       a symmetric matrix (a(d) = a(-d)), 13 distinct off-centre values as for C27, centre 34; not
            reflection-symmetric

The random draws come from numpy's default_rng with the seed written at each stencil."""
import numpy as np

SEEDS = {"C27": 270027, "C9": 90009, "C7": 70007, "C5": 50005, "P27": 131313}


def _offsets(dim):
    zr = 1 if dim == 3 else 0
    return [(dx, dy, dz) for dz in range(-zr, zr + 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def C27():
    st = -(0.25 + np.random.default_rng(SEEDS["C27"]).random(27))
    st[13] = 34.0
    return st


def C9():
    st = -(0.25 + np.random.default_rng(SEEDS["C9"]).random(9))
    st[4] = 11.0
    return st


def _axis(dim, seed, centre):
    u = np.random.default_rng(seed).random(2 * dim)
    st = np.zeros(3 ** dim)
    k = 0
    for t, d in enumerate(_offsets(dim)):
        if sum(abs(v) for v in d) == 1:
            st[t] = -(0.5 + u[k])
            k += 1
    st[len(st) // 2] = centre
    return st


def C7():
    return _axis(3, SEEDS["C7"], 9.5)


def C5():
    return _axis(2, SEEDS["C5"], 6.5)


def S7():
    st = np.zeros(27)
    st[12] = st[14] = -1.0
    st[10] = st[16] = -2.0
    st[4] = st[22] = -4.0
    st[13] = 16.0
    return st


def S27():
    st = np.zeros(27)
    w = {1: 1.0, 2: 0.5, 3: 0.25}
    for t, (dx, dy, dz) in enumerate(_offsets(3)):
        n1 = abs(dx) + abs(dy) + abs(dz)
        st[t] = 24.0 if n1 == 0 else -w[n1] * (1.5 if dz else 1.0) * (1.25 if dy else 1.0)
    return st


def P27():
    u = -(0.25 + np.random.default_rng(SEEDS["P27"]).random(13))
    st = np.zeros(27)
    st[:13] = u
    st[14:] = u[::-1]  # offset t <-> 26 - t is d <-> -d
    st[13] = 34.0
    return st


STENCILS = {"C27": C27, "C9": C9, "C7": C7, "C5": C5, "S7": S7, "S27": S27, "P27": P27}


# The GPU cases (tests/test_gpu_user_stencil.py): name -> (stencil, shape, MultigridParameters keywords over
# SOR / SSOR-coarse defaults).  The smallest shapes of the existing suites that reach each kernel instance.
CASES = {
    "c27_24x20x12": ("C27", (24, 20, 12), dict(nlevel=3)),
    "c27_96x48x48": ("C27", (96, 48, 48), dict(nlevel=4)),
    "c27_64": ("C27", (64, 64, 64), dict(nlevel=5)),
    "c27_320x24x16": ("C27", (320, 24, 16), dict(nlevel=3)),
    "c27_512x24x20_ssor": ("C27", (512, 24, 20), dict(nlevel=3, smoother="SSOR")),
    "c7_64x44x40": ("C7", (64, 44, 40), dict(nlevel=2)),
    "s7_192x48x40": ("S7", (192, 48, 40), dict(nlevel=2)),
    "s7_128x36x24_ssor": ("S7", (128, 36, 24), dict(nlevel=2, smoother="SSOR", coarse_scaling=0.9)),
    "s7_512x24x24": ("S7", (512, 24, 24), dict(nlevel=4)),
    "s27_96x48x48": ("S27", (96, 48, 48), dict(nlevel=4)),
    "s27_80x48x40_ssor_W": ("S27", (80, 48, 40), dict(nlevel=3, cycle=2, smoother="SSOR", npresmooth=2, omega=1.1)),
    "s27_24x20x12": ("S27", (24, 20, 12), dict(nlevel=3)),
    "s27_320x24x16": ("S27", (320, 24, 16), dict(nlevel=3)),
    "p27_32_chol": ("P27", (32, 32, 32), dict(nlevel=3, smoother="SSOR", coarse_solver="Cholesky")),
    "c5_200x120": ("C5", (200, 120), dict(nlevel=4)),
    "c9_256x128_ssor_W": ("C9", (256, 128), dict(nlevel=3, cycle=2, smoother="SSOR", npresmooth=2, omega=1.1)),
    "c9_100x60": ("C9", (100, 60), dict(nlevel=3)),
}
# the cases whose operator product and residual + restriction are also checked against np.longdouble
HIGHPREC = [n for n, c in CASES.items() if c[0] in ("C27", "C5")]


def dim_of(st):
    return 3 if len(st) == 27 else 2


def csr(shape, st):
    """The stencil truncated at the Dirichlet boundary of a lattice of `shape` cells: scipy CSR over the interior
    vertices (x fastest), columns ascending, zero coefficients not stored -- what SparseMatrixOperator takes."""
    import scipy.sparse as sp
    dim = len(shape)
    assert len(st) == 3 ** dim
    ni = [n - 1 for n in shape] + [1] * (3 - dim)
    k, j, i = np.meshgrid(np.arange(ni[2]), np.arange(ni[1]), np.arange(ni[0]), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    n = i.size
    rows, cols, vals = [], [], []
    for t, (dx, dy, dz) in enumerate(_offsets(dim)):
        if st[t] == 0.0:
            continue
        ok = (i + dx >= 0) & (i + dx < ni[0]) & (j + dy >= 0) & (j + dy < ni[1]) & (k + dz >= 0) & (k + dz < ni[2])
        r = np.flatnonzero(ok)
        rows.append(r)
        cols.append(((k[r] + dz) * ni[1] + (j[r] + dy)) * ni[0] + (i[r] + dx))
        vals.append(np.full(r.size, st[t]))
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    A.sort_indices()
    return A


def galerkin_exact(dim, st):
    """R A R^T of a constant 3^d stencil with the (1/2, 1, 1/2)^d linear interpolation, in exact rational
    arithmetic: A_c(delta) = sum_{sigma, tau} w(sigma) w(tau) a(2 delta + tau - sigma) (row 2i + sigma of A, column
    2j + tau, delta = j - i).  Returns (values, sum of |terms|) as lists of Fractions in stencil order; the terms
    are those of the two-step sum (R A) R^T, whose weights are powers of two (their products are exact)."""
    from fractions import Fraction
    offs = _offsets(dim)
    a = {d: Fraction(float(v)) for d, v in zip(offs, st)}
    w = {d: Fraction(1, 2 ** sum(abs(v) for v in d)) for d in offs}
    out, mag = [], []
    for delta in offs:
        s, m = Fraction(0), Fraction(0)
        for sigma in offs:
            for tau in offs:
                d = tuple(2 * delta[q] + tau[q] - sigma[q] for q in range(3))
                if d in a:
                    t = w[sigma] * w[tau] * a[d]
                    s += t
                    m += abs(t)
        out.append(s)
        mag.append(m)
    return out, mag


def restriction(shape):
    """The linear-interpolation restriction of a lattice of `shape` cells onto shape / 2 as a scipy CSR matrix
    (coarse vertex I gathers the fine vertices 2I + sigma with weight 2^-|sigma|_1), columns ascending."""
    import scipy.sparse as sp
    dim = len(shape)
    nf = [n - 1 for n in shape] + [1] * (3 - dim)
    nc = [n // 2 - 1 for n in shape] + [1] * (3 - dim)
    K, J, I = np.meshgrid(np.arange(nc[2]), np.arange(nc[1]), np.arange(nc[0]), indexing="ij")
    I, J, K = I.ravel(), J.ravel(), K.ravel()
    rows, cols, vals = [], [], []
    for (dx, dy, dz) in _offsets(dim):
        # coarse vertex I (0-based interior) is Euclidean I + 1, its fine image 2 (I + 1), 0-based 2 I + 1
        fi, fj, fk = 2 * I + 1 + dx, 2 * J + 1 + dy, (2 * K + 1 + dz if dim == 3 else K)
        rows.append(np.arange(I.size))
        cols.append((fk * nf[1] + fj) * nf[0] + fi)
        vals.append(np.full(I.size, 0.5 ** (abs(dx) + abs(dy) + abs(dz))))
    R = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(I.size, nf[0] * nf[1] * nf[2]))
    R.sort_indices()
    return R


def _rowsum_ld(M, v):
    """M v with every product and sum in np.longdouble (M: scipy CSR without empty rows)."""
    t = M.data.astype(np.longdouble) * np.asarray(v, dtype=np.longdouble)[M.indices]
    return np.add.reduceat(t, M.indptr[:-1])


def gamma(k, u=2.0 ** -53):
    """gamma_k = k u / (1 - k u): the relative error bound of a k-term floating-point sum of products."""
    k = np.asarray(k, dtype=np.float64)
    return k * u / (1.0 - k * u)


def highprec_ratios(shape, st, x, f, y, fc):
    """A level's operator product y = A x and residual + restriction fc = R (f - A x) (fc None on the coarsest
    level) against the same products of the level's CSR -- the stencil `st` truncated on the lattice, assembled
    here -- in np.longdouble.  Any summation order of a row's k terms, fused or not, keeps
        |y - A x| <= gamma_k |A||x|,   |r - (f - A x)| <= gamma_(k+1) (|A||x| + |f|),
    with k the row's entry count (the residual row has one more term, f), gamma_k = k u / (1 - k u), u = 2^-53;
    the residual's bound is pushed through R (non-negative weights; the rounding of the restriction's own sum of
    at most 27 exactly weighted terms is not added, which only makes the check stricter).  The longdouble
    reference's own error (the same bound with u = 2^-64) is added.  Returns (max |error| / bound of A x, of R (f - A x) or None)."""
    A = csr(shape, st)
    k = np.diff(A.indptr)
    absA = abs(A)
    ax = _rowsum_ld(A, x)
    mag = _rowsum_ld(absA, np.abs(x))
    b_op = (gamma(k) + gamma(k, 2.0 ** -64)) * mag
    r_op = float(np.max(np.abs(np.asarray(y, dtype=np.longdouble) - ax) / b_op))
    if fc is None:
        return r_op, None
    R = restriction(shape)
    fl = np.asarray(f, dtype=np.longdouble)
    ref = _rowsum_ld(R, fl - ax)
    b_res = _rowsum_ld(R, (gamma(k + 1) + gamma(k + 1, 2.0 ** -64)) * (mag + np.abs(fl)))
    return r_op, float(np.max(np.abs(np.asarray(fc, dtype=np.longdouble) - ref) / b_res))


def reflection_symmetric(st):
    """Bitwise equal under each of dx, dy, dz -> -d (3D, 27 entries): the device's fold / SYM condition."""
    b = np.ascontiguousarray(st, dtype=np.float64).view(np.uint64).reshape(3, 3, 3)
    return bool(np.array_equal(b, b[::-1]) and np.array_equal(b, b[:, ::-1]) and np.array_equal(b, b[:, :, ::-1]))
