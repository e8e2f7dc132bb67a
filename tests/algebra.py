"""Exact linear-algebra identities of the multicolour sweeps and of whole MGMC cycles.

TEST INFRASTRUCTURE: helpers only, shared by tests/test_algebra_host.py (the CPU oracle in MULTICOLOUR mode) and
tests/test_gpu_algebra.py (the device).  A backend is a MultigridMCSampler or an oracle_lib.Oracle: both have
smoother_apply, sor_sampler_apply, residual_restrict, restrict, prolongate_add, apply and set_sample_index.

Nothing here takes a matrix from the code under test.  A_l is the FAITHFUL oracle's csr_matrix(l) (pinned to the
reference's known answers and to the full SpGEMM, tests/test_oracle.py), B and Sigma come from the operator's
get_B(), B_l = P^T B_(l-1) with the linear interpolation P assembled here from its definition, the colours from the
documented rule (colour_of, mgmc_kernels.hpp), the normals from the documented counter contract (DESIGN.md
section 4, philox_normal.h, the header of mgmc_lowrank.hpp).

  A  a noise-free sweep is the SOR splitting it claims to be, in residual form (no solves):
         (M_dir + B Sigma^-1 B^T)(x' - x) = b - (A + B Sigma^-1 B^T) x,
     M_fwd = D / omega + {a_vu : colour(u) < colour(v)}, M_bwd = D / omega + {colour(u) > colour(v)} = M_fwd^T;
  B  a noisy sweep adds one unit normal per vertex, scaled by sd = sqrt(d (2 - omega) / omega), and one per
     measurement through B Sigma^-1/2:  M~_dir (x' - x) - (f - Q x) = sd o xi + B Sigma^-1/2 xi';
  C  a whole cycle x' = S x + G f + W xi leaves N(Q^-1 f, Q^-1) invariant: S + G Q = I and
     W W^T = Q^-1 - S Q^-1 S^T, W fitted against every normal the counter contract lets the cycle draw;
  D  a cycle is the composition of these pieces: the reference's recursion (multigridmc_sampler.cc:103-138)
     restated over the component entry points reproduces apply() bit for bit;
  R  the residual + restriction is P^T (b - A_l x) componentwise (LevelAlgebra.residual_ratio, bound derived:
     residual_bound);
  G  the level matrices themselves are the Galerkin products P^T A_(l-1) P (galerkin_defects).
Matrix-built problems (Problem kind "matrix": what the library takes through mgmc_create_csr) get all of them; the
colours of their reach-2 levels are the coordinates mod 3.

Tolerance of A and B (componentwise, |lhs - rhs| <= C_TOL * EPS * s): s is the same expression with absolute
values, every low-rank dot product weighted with the number of entries of its column (the gamma factor of a sum of
that length; the blocked dots of a dense column otherwise reach 44 units), plus the two terms of the sweep's
Woodbury fix x' = y - B_bar (B^T y) (LevelAlgebra._lowrank_terms).  The checks return max |lhs - rhs| /
(EPS * s); the tests assert it against C_TOL = 8 (measured: up to 4.2 for A, 6.8 for B; per case in the test files'
docstrings)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import multigridmc_amd as mg
from tests import oracle_lib as O

EPS = 2.0 ** -53
C_TOL = 8.0
LR_PAIR0 = 0xFFFFF000  # Philox pair ids of the low-rank noise (mgmc_lowrank.hpp)
FORWARD, BACKWARD = 1, 2
KAPPA_SQ = 25.0


# ------------------------------------------------------------------------------------------------
# problems: one operator, and the three things built from it (device sampler, replay oracle, FAITHFUL oracle)
# ------------------------------------------------------------------------------------------------
PERIODIC = mg.PeriodicCorrelationLengthModel(0.2, 0.4)
CONSTANT = mg.ConstantCorrelationLengthModel(0.2)  # kappa^2 = 25
MATRIX_OPERATORS = {"fd": (mg.ShiftedLaplaceFDOperator, 0), "fem": (mg.ShiftedLaplaceFEMOperator, 1),
                    "squared": (mg.SquaredShiftedLaplaceFDOperator, 2)}  # (class, the oracle's pde code)


class Problem:
    """kind "fd" | "fem" | "stencil" (stencil: a tests/user_stencils.py name) on `shape` cells; kw over the SOR /
    SSOR-coarse defaults; meas = (radius, number of measurements, measure_global) as in tests/test_gpu_lowrank.py,
    or the low-rank part itself: a measured.LowRankUpdate, or a callable lattice -> LowRankUpdate
    (tests/lowrank_shapes.py).  The sampler of such a problem is the prior's with set_lowrank called on it.

    kind "matrix": an operator the library takes as a matrix (mgmc_create_csr).  pde "fd" | "fem" | "squared" with
    model "periodic" (PERIODIC) or "constant" (CONSTANT), or pde "dominant": the hand-made anisotropic matrix
    tests.test_vardiag_host.dominant_matrix (cx != cy != cz, random dominant diagonal).  The sampler gets the
    library's operator; the oracles get the oracle's own assembly of the same operator (O.operator_csr), so that
    matrix(0)'s assertion compares two assemblies."""

    def __init__(self, kind, shape, kw, meas=None, stencil=None, kappa_sq=KAPPA_SQ, pde=None, model="periodic"):
        self.kind, self.shape, self.meas, self.stencil, self.kappa_sq = kind, tuple(shape), meas, stencil, kappa_sq
        self.pde, self.model = pde, model
        assert (kind == "matrix") == (pde is not None) and model in ("periodic", "constant")
        self.params = mg.MultigridParameters(**{"nlevel": 3, "smoother": "SOR", "coarse_solver": "SSOR", **kw})
        self.lat = mg.Lattice(*shape)
        self._faithful = None
        self._lr = None
        self._meas_is_lowrank = meas is not None and not isinstance(meas, tuple)
        assert not self._meas_is_lowrank or kind == "fd"

    def _dominant(self):
        from tests.test_vardiag_host import dominant_matrix
        return dominant_matrix(self.shape)

    def operator(self):
        if self.kind == "matrix":
            assert self.meas is None
            if self.pde == "dominant":
                return mg.SparseMatrixOperator(self.lat, self._dominant())
            return MATRIX_OPERATORS[self.pde][0](self.lat, PERIODIC if self.model == "periodic" else CONSTANT)
        if self.kind == "fd":
            op = mg.ShiftedLaplaceFDOperator(self.lat, self.kappa_sq)
        elif self.kind == "fem":
            op = mg.ShiftedLaplaceFEMOperator(self.lat, self.kappa_sq)
        else:
            from tests import user_stencils as US
            op = mg.SparseMatrixOperator(self.lat, US.csr(self.shape, US.STENCILS[self.stencil]()))
        if self.meas is not None and not self._meas_is_lowrank:
            from tests.test_gpu_lowrank import measured
            radius, nmeas, glob = self.meas
            assert self.kind == "fd"
            op, _ = measured(self.shape, self.kappa_sq, radius, nmeas, glob)
        return op

    def lowrank(self):
        if self._meas_is_lowrank:
            if self._lr is None:
                self._lr = self.meas(self.lat) if callable(self.meas) else self.meas
                assert self._lr.n == self.lat.Nvertex
            return self._lr
        return self.operator().get_B() if self.meas is not None else None

    def oracle(self, mode=O.MULTICOLOUR, seed=0, chain=0):
        if self.kind == "matrix":
            if self.pde == "dominant":
                A = self._dominant()
                rowptr, col, val = A.indptr, A.indices, A.data
            else:
                rowptr, col, val = O.operator_csr(self.shape, MATRIX_OPERATORS[self.pde][1], self.model == "periodic",
                                                  Lambda=CONSTANT.Lambda, Lambda_min=PERIODIC.Lambda_min,
                                                  Lambda_max=PERIODIC.Lambda_max)
            o = O.Oracle.csr(self.shape, self.params, rowptr, col, val, mode=mode, seed=seed)
            o.reseed(seed, chain)  # (orc_create_csr takes no chain id)
            return o
        if self.kind == "fd":
            o = O.Oracle.fd_own(self.shape, self.params, self.kappa_sq, mode=mode, seed=seed, chain=chain)
        elif self.kind == "fem":
            o = O.Oracle.fem(self.shape, self.params, self.kappa_sq, mode=mode, seed=seed, chain=chain)
        else:
            from tests import user_stencils as US
            o = O.Oracle.stencil(self.shape, self.params, US.STENCILS[self.stencil](), mode=mode, seed=seed,
                                 chain=chain)
        if self.meas is not None:
            o.set_lowrank(self.lowrank())
        return o

    def sampler(self, seed=0, chain=0, nchains=1):
        s = mg.MultigridMCSampler(self.operator(), seed, self.params, device=0, chain_id=chain, nchains=nchains)
        if self._meas_is_lowrank:
            s.set_lowrank(self.lowrank())
        return s

    def faithful(self):
        if self._faithful is None:
            self._faithful = self.oracle(mode=O.FAITHFUL)
        return self._faithful

    def level_shape(self, level):
        return tuple(n >> level for n in self.shape)

    def matrix(self, level):
        """A_l: the FAITHFUL oracle's CSR; on level 0 it must be the operator's own matrix."""
        A = self.faithful().csr_matrix(level)
        if level == 0 and self.kind != "fd":
            base = self.operator()
            own = getattr(base, "base_operator", base).matrix()
            assert abs(A - own).max() == 0.0, "level 0: the FAITHFUL oracle's matrix is not the operator's own CSR"
        return A

    def lowrank_levels(self):
        """[(B_l as CSC, Sigma, entries per column)] per level, B_l = P^T B_(l-1); None for a prior."""
        lr = self.lowrank()
        if lr is None:
            return [None] * self.params.nlevel
        B = sp.csc_matrix((lr.vals, lr.rows, lr.colptr), shape=(lr.n, lr.m))
        out = []
        for level in range(self.params.nlevel):
            if level > 0:
                B = sp.csc_matrix(interpolation(self.level_shape(level - 1)).T @ B)
                B.eliminate_zeros()
            out.append((B, lr.sigma.copy(), np.diff(B.indptr).astype(np.float64)))
        return out

    def precision(self):
        """Q = A_0 + B Sigma^-1 B^T, dense (tiny lattices only)."""
        Q = self.matrix(0).toarray()
        lr = self.lowrank()
        if lr is not None:
            Q = Q + lr.precision_update()
        return Q


# ------------------------------------------------------------------------------------------------
# lattice, colours, splitting, interpolation
# ------------------------------------------------------------------------------------------------
def coords(shape):
    """(dim, N) Euclidean indices 1..n-1 of the interior vertices, x fastest."""
    e = np.arange(int(np.prod([n - 1 for n in shape])))
    out = []
    for n in shape:
        out.append(e % (n - 1) + 1)
        e = e // (n - 1)
    return np.stack(out)


def colour_of(A, shape, level):
    """The documented colours: (i + j + k) & 1 on a fine level whose couplings are all axis neighbours (5 / 7
    point), the parity bits (i & 1) | (j & 1) << 1 | (k & 1) << 2 on 9 / 27-point levels; a level with a coupling
    two vertices apart in a direction (the squared operator and its Galerkin levels) takes the coordinates mod 3,
    (i % 3) + 3 (j % 3) + 9 (k % 3), ascending forward (the header of mgmc_field.hpp)."""
    xyz = coords(shape)
    C = A.tocoo()
    apart = np.abs(xyz[:, C.row] - xyz[:, C.col])
    if ((apart.max(axis=0) > 1) & (C.data != 0.0)).any():
        return sum((xyz[d] % 3) * 3 ** d for d in range(len(shape)))
    off_axis = (apart.sum(axis=0) > 1) & (C.data != 0.0)
    if level == 0 and not off_axis.any():
        return xyz.sum(axis=0) & 1
    return sum((xyz[d] & 1) << d for d in range(len(shape)))


def splitting(A, colour, omega, symmetric=True):
    """(M_fwd, M_bwd): D / omega plus the entries towards lower / higher colours.  No two vertices of a colour are
    coupled; for a symmetric A, M_bwd -- built from "colour(u) > colour(v)" -- is the transpose of M_fwd (an
    entry of R A R^T and its mirror partner are sums of the same terms, as large as the diagonal, in two orders:
    compared within 8 EPS max |A|)."""
    C = A.tocoo()
    cr, cc = colour[C.row], colour[C.col]
    assert not ((cr == cc) & (C.row != C.col) & (C.data != 0.0)).any(), "two vertices of one colour are coupled"
    D = sp.diags(A.diagonal() / omega)
    lo, hi = cc < cr, cc > cr
    Mf = (D + sp.csr_matrix((C.data[lo], (C.row[lo], C.col[lo])), shape=A.shape)).tocsr()
    Mb = (D + sp.csr_matrix((C.data[hi], (C.row[hi], C.col[hi])), shape=A.shape)).tocsr()
    if symmetric:
        diff = abs(Mb - Mf.T.tocsr())
        assert diff.nnz == 0 or diff.max() <= 8 * EPS * abs(A).max(), "M_bwd is not the transpose of M_fwd"
    return Mf, Mb


def interpolation(shape):
    """P: linear interpolation from the lattice of shape / 2 cells to `shape` cells (fine x coarse): coarse vertex
    I sits on fine vertex 2 I with weight 1 and feeds 2 I +- 1 with weight 1/2 per direction."""
    P = None
    for n in shape:
        nf, nc = n - 1, n // 2 - 1
        I = np.arange(1, nc + 1)
        rows = np.concatenate([2 * I - 1, 2 * I - 2, 2 * I])  # 0-based fine indices of 2 I, 2 I - 1, 2 I + 1
        cols = np.concatenate([I - 1, I - 1, I - 1])
        vals = np.concatenate([np.ones(nc), np.full(nc, 0.5), np.full(nc, 0.5)])
        P1 = sp.csr_matrix((vals, (rows, cols)), shape=(nf, nc))
        P = P1 if P is None else sp.kron(P1, P, format="csr")  # x fastest
    return P


def normal_index(shape):
    """Per vertex, its index into normals(0, 2 * npairs, tag, sample): 2 * pair + (i even), pair = row * (n_x / 2) +
    (i - 1) / 2 with row the lexicographic (j, k) index; and the level's number of pairs."""
    xyz = coords(shape)
    nx = shape[0]
    row = np.zeros(xyz.shape[1], dtype=np.int64)
    stride = 1
    for d in range(1, len(shape)):
        row += (xyz[d] - 1) * stride
        stride *= shape[d] - 1
    idx = 2 * (row * (nx // 2) + (xyz[0] - 1) // 2) + (1 - (xyz[0] & 1))
    assert len(np.unique(idx)) == len(idx), "two vertices share one draw"
    return idx, stride * (nx // 2)


def oracle_normals(seed, chain):
    """normals(pair0, n, tag, sample) of a (seed, chain) from the oracle's Philox (test_normals_bitwise pins it to
    the device's)."""
    return lambda pair0, n, tag, sample: O.philox_normals(seed, chain, pair0, n, tag, sample)


def lowrank_normals(normals, m, tag, sample):
    """xi'_k: pair LR_PAIR0 + k / 2 of the sweep's tag, cos branch for even k."""
    return normals(LR_PAIR0, 2 * ((m + 1) // 2), tag, sample)[:m]


# ------------------------------------------------------------------------------------------------
# A and B
# ------------------------------------------------------------------------------------------------
class LevelAlgebra:
    """The matrices of one level of a problem."""

    def __init__(self, prob, level, symmetric=True):
        self.level = level
        self.shape = prob.level_shape(level)
        self.A = prob.matrix(level).tocsr()
        self.absA = abs(self.A)
        self.n = self.A.shape[0]
        omega = prob.params.omega
        self.colour = colour_of(self.A, self.shape, level)
        Mf, Mb = splitting(self.A, self.colour, omega, symmetric)
        self.M = {FORWARD: Mf, BACKWARD: Mb}
        self.absM = {FORWARD: abs(Mf), BACKWARD: abs(Mb)}
        self.sd = np.sqrt(self.A.diagonal() * (2.0 - omega) / omega)
        self.xi_index, self.npairs = normal_index(self.shape)
        self.lr = None
        self.bbar_term = True  # (False only to measure what the term of _lowrank_terms is worth)
        self._bbar_cache = {}

    def _solve_split(self, direction, rhs):
        """M_dir^-1 rhs by substitution over the colour classes in sweep order (for the tolerance's scale only)."""
        M = self.M[direction]
        diag = M.diagonal()
        u = np.zeros(self.n)
        order = sorted(np.unique(self.colour), reverse=direction == BACKWARD)
        for c in order:
            idx = np.flatnonzero(self.colour == c)
            u[idx] = (rhs[idx] - M[idx] @ u) / diag[idx]  # u is still zero on this and the later classes
        return u

    def _bbar(self, direction):
        """(|B_bar|, K) of a direction, from B, Sigma and the splitting assembled here (nothing from the library or
        the oracle): Y = M_dir^-1 B column by column (_solve_split), K = Sigma + B^T Y, B_bar = Y K^-1 with K
        inverted in extended precision (Gauss-Jordan with partial pivoting on long doubles)."""
        if direction not in self._bbar_cache:
            B, sig, _ = self.lr
            m = len(sig)
            Bd = B.toarray()
            Y = np.stack([self._solve_split(direction, Bd[:, k]) for k in range(m)], axis=1).astype(np.longdouble)
            K = np.diag(sig.astype(np.longdouble)) + Bd.T.astype(np.longdouble) @ Y
            W = np.concatenate([K, np.eye(m, dtype=np.longdouble)], axis=1)
            for c in range(m):
                p = c + int(np.argmax(np.abs(W[c:, c])))
                W[[c, p]] = W[[p, c]]
                W[c] = W[c] / W[c, c]
                rest = np.arange(m) != c
                W[rest] = W[rest] - np.outer(W[rest, c], W[c])
            self._bbar_cache[direction] = (np.abs(Y @ W[:, m:]).astype(np.float64), K)
        return self._bbar_cache[direction]

    def _lowrank_terms(self, direction, xn, x):
        """(B Sigma^-1 B^T (x' - x), B Sigma^-1 B^T x, the low-rank part of s).  s takes the two products with
        absolute values, every dot with its column's length; and the term of the Woodbury form: the sweep's fix
        forms x' = y - u from the swept vector y, u = B_bar B^T y = M^-1 B Sigma^-1 B^T x' exactly (B^T x' = Sigma
        K^-1 B^T y, K = Sigma + B^T M^-1 B), so x' carries a rounding of EPS (|y| + |u|) <= EPS (|x'| + 2 |u|) that
        |M~| = |M| + |B| Sigma^-1 |B|^T carries into the identity.  At a measured vertex with a small variance
        |u| is the larger by d Sigma / omega (170 at the 2D point measurements): without this term their ratio is
        76 on the oracle, with it 1."""
        B, sig, cnt = self.lr
        aB = abs(B)
        mag_d = np.abs(xn) + np.abs(x)
        u = 2.0 * np.abs(self._solve_split(direction, B @ ((B.T @ xn) / sig)))
        woodbury = self.absM[direction] @ u + aB @ (cnt * (aB.T @ u) / sig)
        if self.bbar_term:
            # ... and the rounding inside u = B_bar (B^T y) itself: an m-term fma chain against the stored B_bar =
            # Y K^-1, gamma_m |B_bar| |B^T y| per component (B^T y = K Sigma^-1 B^T x'), which cancels heavily when
            # the columns of Y are nearly collinear (64 measurements close together); carried by |M~| like the rest
            abar, K = self._bbar(direction)
            bty = np.abs((K @ ((B.T @ xn) / sig).astype(np.longdouble)).astype(np.float64))
            v = len(sig) * (abar @ bty)
            woodbury = woodbury + self.absM[direction] @ v + aB @ (cnt * (aB.T @ v) / sig)
        return (B @ ((B.T @ (xn - x)) / sig), B @ ((B.T @ x) / sig),
                aB @ (cnt * (aB.T @ mag_d) / sig) + aB @ (cnt * (aB.T @ np.abs(x)) / sig) + woodbury)

    def sweep_ratio(self, be, direction, b, x):
        """A: one noise-free sweep x' = smoother_apply(level, direction, 1, b, x)."""
        xn = be.smoother_apply(self.level, direction, 1, b, x)
        d = xn - x
        lhs = self.M[direction] @ d
        rhs = b - self.A @ x
        s = self.absM[direction] @ (np.abs(xn) + np.abs(x)) + np.abs(b) + self.absA @ np.abs(x)
        if self.lr is not None:
            ld, lx, ls = self._lowrank_terms(direction, xn, x)
            lhs, rhs, s = lhs + ld, rhs - lx, s + ls
        assert np.all(np.isfinite(xn))
        return float(np.max(np.abs(lhs - rhs) / (EPS * s)))

    def noise_ratio(self, be, normals, direction, tag, sample, f=None, x=None, xn=None):
        """B: one noisy sweep x' = sor_sampler_apply(level, direction, tag, sample, f, x) (f = x = 0 unless given):
        (M~ (x' - x) - (f - Q x) - B Sigma^-1/2 xi') / sd = xi, componentwise.  With f and x given it is A and B at
        once, through the kernel the cycle runs on this level.  xn: the sweep's result if it was run elsewhere."""
        zero = f is None
        if zero:
            f = x = np.zeros(self.n)
        if xn is None:
            xn = be.sor_sampler_apply(self.level, direction, tag, sample, f, x)
        assert np.all(np.isfinite(xn))
        xi = normals(0, 2 * self.npairs, tag, sample)[self.xi_index]
        assert len(np.unique(xi)) == self.n, "two vertices drew the same normal"
        d = xn - x
        got = self.M[direction] @ d
        s = self.absM[direction] @ (np.abs(xn) + np.abs(x))
        if not zero:
            got = got - (f - self.A @ x)
            s = s + np.abs(f) + self.absA @ np.abs(x)
        if self.lr is not None:
            B, sig, cnt = self.lr
            ld, lx, ls = self._lowrank_terms(direction, xn, x)
            xip = lowrank_normals(normals, len(sig), tag, sample)
            got = got + ld + lx - B @ (xip / np.sqrt(sig))
            s = s + ls + abs(B) @ (np.abs(xip) / np.sqrt(sig))
        return float(np.max(np.abs(got / self.sd - xi) / (EPS * s / self.sd)))


    # R: the residual + restriction onto the next level
    def residual_bound(self):
        """The bound of residual_ratio, derived: the row sum's rounding factor (its number of terms, the largest
        row's), one for the subtraction from b, and 3^d for the restriction's sum (its weights are powers of two).
        A posterior level subtracts B Sigma^-1 B^T x as well: per row one term per stored B_ik (the fullest row's
        count), each a product and a quotient (2), on a dot whose own factor -- its column's length -- is in s."""
        bound = float(np.diff(self.A.indptr).max() + 1 + 3 ** len(self.shape))
        if self.lr is not None:
            bound += float(np.diff(self.lr[0].tocsr().indptr).max() + 2)
        return bound

    def residual_ratio(self, be, b, x):
        """R: residual_restrict(level, b, x) = P^T (b - Q_l x) componentwise, P from its definition, Q_l = A_l (+
        B_l Sigma^-1 B_l^T on a posterior level); the ratio |got - ref| / (EPS P^T (|b| + |A_l| |x| + |B_l| Sigma^-1
        (column lengths o |B_l|^T |x|)))."""
        P = interpolation(self.shape)
        got = be.residual_restrict(self.level, b, x)
        assert got.shape == (P.shape[1],) and np.all(np.isfinite(got))
        r = b - self.A @ x
        mag = np.abs(b) + self.absA @ np.abs(x)
        if self.lr is not None:
            B, sig, cnt = self.lr
            r = r - B @ ((B.T @ x) / sig)
            mag = mag + abs(B) @ (cnt * (abs(B).T @ np.abs(x)) / sig)
        return float(np.max(np.abs(got - P.T @ r) / (EPS * (P.T @ mag))))


def check_residuals(prob, be, rng, algebras):
    """R on every level that has a coarser one: {level: (ratio, its bound)}; prints the largest ratio."""
    out = {}
    for la in algebras[:-1]:
        b, x = rng.standard_normal(la.n), rng.standard_normal(la.n)
        out[la.level] = (la.residual_ratio(be, b, x), la.residual_bound())
    print("algebra R (residual + restriction): " + "  ".join(f"level {l} ratio {r:.2f} (bound {c:.0f})"
                                                              for l, (r, c) in out.items()))
    return out


GALERKIN_TOL = 64.0  # in EPS max |A_l|: the association of at most 3^d x 3^d terms per entry


def galerkin_defects(prob):
    """G: A_l = P^T A_(l-1) P with P = interpolation(...) on the FAITHFUL oracle's level matrices, which makes them
    independent of any Galerkin code: [max |A_l - P^T A_(l-1) P| / (EPS max |A_l|)] for l = 1 .. nlevel - 1."""
    out = []
    for level in range(1, prob.params.nlevel):
        P = interpolation(prob.level_shape(level - 1))
        A = prob.matrix(level)
        D = abs(sp.csr_matrix(P.T @ prob.matrix(level - 1) @ P) - A)
        out.append(float((D.max() if D.nnz else 0.0) / (EPS * abs(A).max())))
    print("algebra G (Galerkin products), per level from 1: " + "  ".join(f"{v:.3g}" for v in out))
    return out


def level_algebras(prob, symmetric=True):
    lrs = prob.lowrank_levels()
    out = []
    for level in range(prob.params.nlevel):
        la = LevelAlgebra(prob, level, symmetric)
        la.lr = lrs[level]
        out.append(la)
    return out


def check_sweeps(prob, be, normals, tag, sample, rng, symmetric=True, algebras=None):
    """A and B on every level and in both directions; {(level, direction): (ratio A, ratio B, ratio of A and B at
    once on the level's own kernel)}."""
    out = {}
    for la in algebras or level_algebras(prob, symmetric):
        for direction in (FORWARD, BACKWARD):
            x, b = rng.standard_normal(la.n), rng.standard_normal(la.n)
            out[(la.level, direction)] = (
                la.sweep_ratio(be, direction, b, x),
                la.noise_ratio(be, normals, direction, tag + la.level, sample),
                la.noise_ratio(be, normals, direction, tag + la.level + 1, sample + 1, b, x))
    return out


def report(name, ratios):
    """One line per case for the logs; returns the largest ratio."""
    worst = max(max(v) for v in ratios.values())
    cols = [max(v[q] for v in ratios.values()) for q in range(3)]
    print(f"algebra {name}: max ratio A {cols[0]:.2f}  B {cols[1]:.2f}  A+B on the level's kernel {cols[2]:.2f}")
    return worst


# ------------------------------------------------------------------------------------------------
# C: whole cycles
# ------------------------------------------------------------------------------------------------
def sweep_tags(params, level=0):
    """T: the sweep tags one cycle uses, by the reference's recursion (multigridmc_sampler.cc:103-131): a SOR
    sampler one per sweep, an SSOR sampler two, the Cholesky coarse sampler one."""
    per = 2 if params.smoother == "SSOR" else 1
    if level == params.nlevel - 1:
        return 1 if params.coarse_solver == "Cholesky" else 2 * params.ncoarsesmooth
    visits = params.cycle if level > 0 else 1
    return visits * (per * params.npresmooth + sweep_tags(params, level + 1) + per * params.npostsmooth)


def cycle(be, k, x, f):
    """T_k(x, f): one cycle with sample index k."""
    be.set_sample_index(k)
    out = np.array(x, dtype=np.float64)
    be.apply(np.asarray(f, dtype=np.float64), out)
    return out


def probe_cycle(be, n, k):
    """x' = S x + G f + eta_k: S and G column by column at a fixed sample index."""
    z = np.zeros(n)
    e0 = cycle(be, k, z, z)
    S, G = np.empty((n, n)), np.empty((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        S[:, i] = cycle(be, k, e, z) - e0
        G[:, i] = cycle(be, k, z, e) - e0
    return S, G


def contract_normals(normals, npairs, m, ntags, sample):
    """Every normal the counter contract lets a cycle with this sample index draw under tags 0 .. ntags - 1: the
    fine level's pair range (coarser levels use a prefix of it), then the low-rank pairs."""
    cols = []
    for tag in range(ntags):
        cols.append(normals(0, 2 * npairs, tag, sample))
        if m:
            cols.append(lowrank_normals(normals, m, tag, sample))
    return np.concatenate(cols)


def fit_noise(Xi, H):
    """W^T of the least-squares problem Xi W^T = H (K x columns, K x n), with the conditions that keep the fit
    from hiding a failure: K >= 1.5 columns, full column rank, residual <= 1e-11 max |eta|."""
    import scipy.linalg as sl
    K, c = Xi.shape
    assert K >= 1.5 * c, (K, c)
    Qf, R = sl.qr(Xi, mode="economic", overwrite_a=False, check_finite=True)
    dR = np.abs(np.diag(R))
    assert dR.min() > 1e-8 * dR.max(), "the normals' matrix has no full column rank"
    Wt = sl.solve_triangular(R, Qf.T @ H)
    resid = float(np.max(np.abs(Xi @ Wt - H)))
    return Wt, resid / float(np.max(np.abs(H)))


def cycle_identities(prob, T, normals_of, samples, SG):
    """C for one problem.  T(q, x, f): one cycle with the q-th entry of `samples` = (chain, sample index) pairs;
    normals_of(chain) -> normals(); SG = probe_cycle's (S, G).  Returns {"consistency", "stationarity", "extra_rows", "fit", "K", "columns"}:
    max |S + G Q - I|, max |W W^T - (Q^-1 - S Q^-1 S^T)| / max |Q^-1|, max |rows of W for tags T, T + 1| / max
    |eta|, the fit's residual / max |eta|."""
    p = prob.params
    Q = prob.precision()
    n = Q.shape[0]
    ntags = sweep_tags(p)
    _, npairs = normal_index(prob.shape)
    lr = prob.lowrank()
    m = lr.m if lr is not None else 0
    percol = 2 * npairs + m
    S, G = SG
    Qinv = np.linalg.inv(Q)
    consistency = float(np.max(np.abs(S + G @ Q - np.eye(n))))
    z = np.zeros(n)
    H = np.stack([T(q, z, z) for q in range(len(samples))])
    Xi = np.stack([contract_normals(normals_of(chain), npairs, m, ntags + 2, k) for chain, k in samples])
    assert Xi.shape[1] == (ntags + 2) * percol
    Wt, fit = fit_noise(Xi, H)
    scale = float(np.max(np.abs(Qinv)))
    stationarity = float(np.max(np.abs(Wt.T @ Wt - (Qinv - S @ Qinv @ S.T)))) / scale
    extra = float(np.max(np.abs(Wt[ntags * percol:]))) / float(np.max(np.abs(H)))
    return {"consistency": consistency, "stationarity": stationarity, "extra_rows": extra, "fit": fit,
            "K": len(samples), "columns": Xi.shape[1], "tags": ntags}


# ------------------------------------------------------------------------------------------------
# D: the cycle as a composition of the component entry points
# ------------------------------------------------------------------------------------------------
def replay_cycle(be, params, sample, f, x):
    """MultigridMCSampler::apply (multigridmc_sampler.cc:103-138) over the component entry points: sweep tags 0, 1,
    2, ... in op order, one sample index (SSOR coarse sampler only)."""
    assert params.coarse_solver == "SSOR"
    tag = [0]

    def sweeps(level, count, first, symmetric, f, x):
        for _ in range(count):
            for direction in ((FORWARD, BACKWARD) if symmetric else (first,)):
                x = be.sor_sampler_apply(level, direction, tag[0], sample, f, x)
                tag[0] += 1
        return x

    def sample_level(level, f, x):
        if level == params.nlevel - 1:
            return sweeps(level, params.ncoarsesmooth, FORWARD, True, f, x)
        ssor = params.smoother == "SSOR"
        for _ in range(params.cycle if level > 0 else 1):
            x = sweeps(level, params.npresmooth, FORWARD, ssor, f, x)
            fc = be.residual_restrict(level, f, x)
            xc = sample_level(level + 1, fc, np.zeros(len(fc)))
            x = be.prolongate_add(level, params.coarse_scaling, xc, x)
            x = sweeps(level, params.npostsmooth, BACKWARD, ssor, f, x)
        return x

    out = sample_level(0, np.asarray(f, dtype=np.float64), np.asarray(x, dtype=np.float64))
    assert tag[0] == sweep_tags(params)
    return out


def apply_precision(prob, v):
    """Q v in scipy: A_0 v + B Sigma^-1 B^T v."""
    out = prob.matrix(0) @ v
    lr = prob.lowrank()
    if lr is not None:
        B = sp.csc_matrix((lr.vals, lr.rows, lr.colptr), shape=(lr.n, lr.m))
        out = out + B @ ((B.T @ v) / lr.sigma)
    return out


def composition(prob, be, sample, rng):
    """D: (relative error of T_k(mu, Q mu) - T_k(0, 0) = mu, apply() == the replay bit for bit after + 0.0)."""
    n = prob.lat.Nvertex
    mu = rng.standard_normal(n)
    z = np.zeros(n)
    got = cycle(be, sample, mu, apply_precision(prob, mu)) - cycle(be, sample, z, z)
    consistency = float(np.max(np.abs(got - mu)) / np.max(np.abs(mu)))
    f, x = rng.standard_normal(n), rng.standard_normal(n)
    whole = cycle(be, sample, x, f) + 0.0
    parts = replay_cycle(be, prob.params, sample, f, x) + 0.0
    same = bool(np.array_equal(whole.view(np.uint64), parts.view(np.uint64)))
    return consistency, same, float(np.max(np.abs(whole - parts)))
