"""The reference of the whole-field energy tests (tests/test_energy_host.py, tests/test_gpu_energy.py), host only.

energy_reference(op, f, x) evaluates, in np.longdouble and from the operator's own data (its assembled matrix
get_csr(), its low-rank part get_B(), the right-hand side f),

    xqx_ref = x^T A x + sum_k (B_k^T x)^2 / Sigma_k,        fx_ref = f^T x,
    S = |x|^T |A| |x| + sum_k (|B_k|^T |x|)^2 / Sigma_k,    T = |f|^T |x|,

and n = nnz(A) + 2 nnz(B) + N + 4 m, the number of rounded operations of any evaluation of xqx in float64: one
product and one addition per matrix entry folded into the nnz(A) + N terms of the double sum, two per entry of B,
and square, scale, and two additions per column.  Any summation order of n rounded terms is within n u S (1 + O(n u))
of the exact value (u = 2^-53; Higham, Accuracy and Stability, section 4.2); the tests allow twice that, and
2 N u T for fx.  The longdouble reference itself is off by at most n 2^-64 S, 2^-11 of the bound.
"""
import numpy as np

U = 2.0 ** -53


def energy_reference(op, f, x):
    """(xqx_ref, fx_ref, S, T, n) as Python floats / int; f None: zero."""
    ld = np.longdouble
    base = getattr(op, "base_operator", op)
    rowptr, col, val = base.get_csr()
    N = len(rowptr) - 1
    assert x.shape == (N,)
    xl = x.astype(ld)
    xa = np.abs(xl)
    vl = val.astype(ld)
    starts = rowptr[:-1]
    assert np.all(np.diff(rowptr) > 0)  # (reduceat: no empty row)
    ax = np.add.reduceat(vl * xl[col], starts)
    aax = np.add.reduceat(np.abs(vl) * xa[col], starts)
    xqx = np.sum(xl * ax)
    S = np.sum(xa * aax)
    n = len(val) + N
    if op.get_m_lowrank() > 0:
        B = op.get_B()
        for k in range(B.m):
            s = slice(B.colptr[k], B.colptr[k + 1])
            bv = B.vals[s].astype(ld)
            w = np.sum(bv * xl[B.rows[s]])
            wa = np.sum(np.abs(bv) * xa[B.rows[s]])
            xqx = xqx + w * w / ld(B.sigma[k])
            S = S + wa * wa / ld(B.sigma[k])
        n += 2 * len(B.vals) + 4 * B.m
    if f is None:
        fx, T = ld(0), ld(0)
    else:
        fl = np.asarray(f).astype(ld)
        fx = np.sum(fl * xl)
        T = np.sum(np.abs(fl) * xa)
    return float(xqx), float(fx), float(S), float(T), int(n)


def within_bound(xqx, fx, ref):
    """(ok, ratio_xqx, ratio_fx): |xqx - xqx_ref| <= 2 n u S and |fx - fx_ref| <= 2 N u T; the ratios are the
    errors over the bounds (0 where the bound is 0 and the value exact)."""
    xr, fr, S, T, n = ref[:5]
    N = ref[5]
    bq, bf = 2.0 * n * U * S, 2.0 * N * U * T
    eq, ef = abs(xqx - xr), abs(fx - fr)
    rq = eq / bq if bq > 0 else (0.0 if eq == 0 else np.inf)
    rf = ef / bf if bf > 0 else (0.0 if ef == 0 else np.inf)
    return eq <= bq and ef <= bf, rq, rf


def reference(op, f, x):
    """energy_reference with N appended, for within_bound"""
    return energy_reference(op, f, x) + (op.get_ndof(),)


def welford(values):
    """(n, mean, M2) of the device's update, one value at a time in float64"""
    n, mean, m2 = 0.0, 0.0, 0.0
    for e in values:
        e = float(e)
        cnt = n + 1.0
        delta = e - mean
        mean_new = mean + delta / cnt
        m2 = m2 + delta * (e - mean_new)
        mean = mean_new
        n = cnt
    return np.array([n, mean, m2])


def iact_windowed(z):
    """the windowed series estimator of the statistical tests (tests/test_field_batch_host.py, test_gpu_exact.py)"""
    z = np.asarray(z, dtype=np.float64)
    z = z - z.mean()
    var = z.var()
    tau = 1.0
    for t in range(1, len(z) // 10):
        rho = np.dot(z[:-t], z[t:]) / ((len(z) - t) * var)
        if rho < 0.05:
            break
        tau += 2 * rho
    return tau
