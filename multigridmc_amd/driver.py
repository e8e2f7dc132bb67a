"""driver_mgmc for the device sampler: `python -m multigridmc_amd.driver parameters.cfg`.

Mirrors the Multigrid MC part of the reference's driver (src/driver_mgmc.cc):
  * main: read the parameters file, build the lattice, the FD prior, the posterior
    (MeasuredOperator, always built) and the MGMC sampler with seed 5418513 ........ :319-535
  * measure_sampling_time: fix f = Q mean_x, nwarmup + nsamples cycles, QoI z = b^T x per
    sample, "time per sample", timeseries_multigridmc.txt, mean / variance against the exact
    observed mean and variance ......................................................... :40-107
    (--energy-stride S: also the whole-field energy x^T Q x, f^T x of every S-th of those samples, reduced
    on the device, to energy_multigridmc.txt, and the chi-square check of its mean; not in the reference)
    (--qoi-panel: also the QoI panel -- the predicted data B^T x at every measurement site and the QoI vector as
    the last column -- recorded on the device with its covariance and tau_int, printed in the layout of the
    reference's Statistics, auxilliary/statistics.cc:88-108, and written to panel_multigridmc.txt)
  * measure_convergence: nsamplesconvergence chains from x = 0, nstepsconvergence cycles
    each; |E[z^k] - E[z]| and |Var[z^k] - Var[z]| with error bars to
    convergence_multigridmc.txt ........................................................ :188-314
  * posterior_statistics: nwarmup + nsamples cycles, the sample mean and the pointwise variance
    of the whole field (accumulated on the device, MultigridMCSampler.field_stats) with the exact
    mean to posterior.vtk, in 2D the sample location to sample_location.vtk ............ :118-171
The exact targets (LinearOperator::mean, observed_mean_and_variance, linear_operator.hh:119-174)
come from the device multigrid-preconditioned CG on the posterior operator (mgmc_solve) instead of
a sparse Cholesky factorisation.  As in the reference, the "exact" observed statistics always
refer to the measured (posterior) operator built on top of the chosen operator.

Out of scope (not the device hot path): the Cholesky and SSOR samplers of the whole lattice
(do_cholesky / do_ssor are reported and skipped).
Every prior of the reference is on the device path (driver_mgmc.cc:398-429): pdemodel =
"shiftedlaplace_fd", "shiftedlaplace_fem" and "squared_shiftedlaplace_fd" (2D), with the
"constant" or the "periodic" correlation length model; operators with per-vertex coefficients go to
the device as matrices (mgmc_create_csr).
"""
from __future__ import annotations

import datetime
import os
import sys
import time

import numpy as np

from . import _native as mg_native
from .measured import MeasuredOperator, measurement_panel, measurement_vector
from .parameters import (ConfigError, ConstantCorrelationLengthModelParameters, GeneralParameters,
                         LatticeParameters, MeasurementFileError, MeasurementParameters, MultigridParameters,
                         PeriodicCorrelationLengthModelParameters, PriorParameters, SamplingParameters, read_config)
from .sampler import (ConstantCorrelationLengthModel, Lattice, MultigridMCSampler, PeriodicCorrelationLengthModel,
                      ShiftedLaplaceFDOperator, ShiftedLaplaceFEMOperator, SquaredShiftedLaplaceFDOperator)
from .vtk import write_vtk, write_vtk_circle

SEED = 5418513  # driver_mgmc.cc:448


def _measured_values(mp: MeasurementParameters) -> np.ndarray:
    y = list(mp.mean[:len(mp.measurement_locations)])
    if mp.measure_global:
        y.append(mp.mean_global)
    return np.asarray(y, dtype=np.float64)


class ExactTargets:
    """LinearOperator::mean / observed_mean_and_variance (linear_operator.hh:119-174) with xbar = 0,
    from device CG solves with the posterior precision Q = A + B Sigma^-1 B^T:
    x_post = Q^-1 B Sigma^-1 y,  mean z = b^T x_post,  Var z = b^T Q^-1 b."""

    def __init__(self, posterior_sampler: MultigridMCSampler, rtol: float = 1e-12, maxiter: int = 200):
        self.s = posterior_sampler
        self.rtol = rtol
        self.maxiter = maxiter

    def solve(self, b):
        x, it, rn = self.s.solve(b, method="cg", rtol=self.rtol, maxiter=self.maxiter)
        if it >= self.maxiter:
            raise RuntimeError(f"exact-statistics solve did not converge (||r|| = {rn})")
        return x

    def posterior_mean(self, y) -> np.ndarray:
        lr = self.s.linear_operator.get_B()
        g = np.zeros(lr.n)
        for k in range(lr.m):
            sl = slice(lr.colptr[k], lr.colptr[k + 1])
            g[lr.rows[sl]] += lr.vals[sl] * (y[k] / lr.sigma[k])
        return self.solve(g)

    def observed_mean_and_variance(self, y, rows, vals):
        b = np.zeros(self.s.ndof)
        b[rows] = vals
        bbar = self.solve(b)
        x_post = self.posterior_mean(y)
        return float(np.dot(b, x_post)), float(np.dot(b, bbar))


def _qoi_series(sampler: MultigridMCSampler, nsteps: int, rows, vals) -> np.ndarray:
    """z = b^T x after every cycle (driver_mgmc.cc:76), recorded on the device inside the cycle graph:
    radius 0 reads the vertex, radius > 0 the dot with the installed vector (mgmc_set_qoi_vector,
    blocked order) -- the state never leaves HBM."""
    if len(rows) == 1 and vals[0] == 1.0:
        return sampler.sample(nsteps, int(rows[0]))
    if getattr(sampler, "_qv", None) is None or not (np.array_equal(sampler._qv[0], rows)
                                                      and np.array_equal(sampler._qv[1], vals)):
        sampler.set_qoi_vector(rows, vals)
    return sampler.sample(nsteps, mg_native.QOI_VECTOR)


def _iact_windowed(z) -> float:
    """integrated autocorrelation time of a series: 1 + 2 sum of the autocorrelations down to the first below 0.05"""
    z = np.asarray(z, dtype=np.float64) - np.mean(z)
    var = z.var()
    tau = 1.0
    for t in range(1, len(z) // 10):
        rho = np.dot(z[:-t], z[t:]) / ((len(z) - t) * var)
        if rho < 0.05:
            break
        tau += 2 * rho
    return tau


def report_energy(sampler, label: str, f, mean_x_exact, filename: str = "energy_multigridmc.txt"):
    """The recorded whole-field energy (MultigridMCSampler.energy_record): (cycle, xqx, fx) per record to
    `filename`, and E = xqx - 2 fx + f^T Q^-1 f against chi-square with N degrees of freedom: its mean, N and the
    z-score (mean - N) / sqrt(2 N tau / n), tau the windowed autocorrelation time of the records (at least 1).
    f = Q mean_x_exact (measure_sampling_time), so f^T Q^-1 f = f^T mean_x_exact with the solve of mgmc_solve."""
    info = sampler.energy_record_info()
    xqx, fx = sampler.energy_series(0)
    with open(filename, "w") as out:
        for r in range(len(xqx)):
            out.write(f"{(r + 1) * info['stride']:d} {xqx[r]:.17g} {fx[r]:.17g}\n")
    const = float(np.dot(f, mean_x_exact))
    e = xqx - 2.0 * fx + const
    n, N = len(e), sampler.ndof
    if n == 0:
        print(f"  {label:>12s} energy   : no cycle recorded")
        return None
    tau = max(1.0, _iact_windowed(e)) if n >= 20 else 1.0
    z = (e.mean() - N) / np.sqrt(2.0 * N * tau / n)
    print(f"  {label:>12s} energy   = {e.mean():12.6e} over {n} records (x^T Q x - 2 f^T x + f^T Q^-1 f, "
          f"f^T Q^-1 f = {const:.6e})")
    print(f"  {'chi-square':>12s} N        = {N:12d}   z-score = {z:+.2f}   [tau = {tau:.2f}]")
    return float(e.mean()), N, float(z)


PANEL_WINDOW = 32      # autocorrelation window of --qoi-panel
PANEL_EXACT_MAX_K = 16  # the exact mean and covariance take K solves


def report_panel(sampler, label: str, exact: ExactTargets, columns, mean_x_exact,
                 filename: str = "panel_multigridmc.txt"):
    """The recorded QoI panel (MultigridMCSampler.qoi_panel_record) in the layout of the reference's
    operator<<(Statistics) (statistics.cc:88-108): Avg, Var, tau_{int,j} per column, window, # samples; the
    records (cycle, z_0 .. z_{K-1}) go to `filename`.  With at most PANEL_EXACT_MAX_K columns also the exact mean
    b_k^T Q^-1 f = b_k^T mean_x_exact and covariance b_k^T Q^-1 b_l (one solve per column)."""
    info = sampler.qoi_panel_info()
    z = sampler.qoi_panel_series(0)
    with open(filename, "w") as out:
        for r in range(len(z)):
            out.write(f"{(r + 1) * info['stride']:d} " + " ".join(f"{v:.17g}" for v in z[r]) + "\n")
    n, mean, cov = sampler.qoi_panel_moments(0)
    tau = sampler.qoi_panel_tau_int(0)
    K = info["K"]

    def vec(v):
        return " ".join(f"{x:.6f}" for x in v)

    def mat(m):
        return "\n".join(("" if r == 0 else " " * (len(label) + 9)) + vec(m[r]) for r in range(len(m)))

    print(f" {label}: Avg = {vec(mean)}")
    print(f" {label}: Var = {mat(cov)}")
    for j in range(K):
        print(f" {label}: tau_{{int,j}} = {tau[j]:.3f}")
    print(f" {label}: window      = {info['window']}")
    print(f" {label}: # samples   = {int(n)}")
    if K > PANEL_EXACT_MAX_K:
        print(f" {'exact'}: skipped, the exact mean and covariance of {K} > {PANEL_EXACT_MAX_K} columns take {K} solves\n")
        return mean, cov, tau, None, None
    B = np.zeros((sampler.ndof, K))
    for k, (rows, vals) in enumerate(columns):
        B[rows, k] = vals
    U = np.stack([exact.solve(B[:, k]) for k in range(K)], axis=1)
    mean_exact, cov_exact = B.T @ mean_x_exact, B.T @ U
    print(f" {'exact'}: Avg = {vec(mean_exact)}")
    print(f" {'exact'}: Var = {mat(cov_exact)}\n")
    return mean, cov, tau, mean_exact, cov_exact


def measure_sampling_time(sampler, exact: ExactTargets, sampling_params: SamplingParameters,
                          measurement_params: MeasurementParameters, label: str, filename: str,
                          energy_stride=None, qoi_panel=None):
    """driver_mgmc.cc:40-107.  energy_stride=S (--energy-stride S): the energy of every S-th sample is recorded on
    the device (report_energy).  qoi_panel (--qoi-panel): the measured operator whose columns, with the QoI vector
    as the last one, are recorded as a panel (report_panel)."""
    op = sampler.get_linear_operator()
    y = _measured_values(measurement_params)
    mean_x_exact = exact.posterior_mean(y) if op.get_m_lowrank() > 0 else np.zeros(op.get_ndof())
    rows, vals = measurement_vector(op.get_lattice(), measurement_params.sample_location, measurement_params.radius)
    f = sampler.operator_apply(0, mean_x_exact)
    sampler.fix_rhs(f)
    sampler.set_state(np.zeros(op.get_ndof()))
    _qoi_series(sampler, sampling_params.nwarmup, rows, vals)
    if energy_stride is not None:
        sampler.energy_record(energy_stride, max(1, sampling_params.nsamples // energy_stride))
    panel_columns = None
    if qoi_panel is not None:
        panel_columns = measurement_panel(qoi_panel, extra=[(rows, vals)])
        sampler.set_qoi_panel(panel_columns)
        sampler.qoi_panel_record(1, PANEL_WINDOW, max(1, sampling_params.nsamples))
    t0 = time.perf_counter()
    data = _qoi_series(sampler, sampling_params.nsamples, rows, vals)
    t_elapsed = (time.perf_counter() - t0) * 1e3 / sampling_params.nsamples
    print(f"  {label:>12s} time per sample = {t_elapsed:12.4f} ms")
    if energy_stride is not None:
        try:
            report_energy(sampler, label, f, mean_x_exact)
        finally:
            sampler.energy_record_off()
    if panel_columns is not None:
        try:
            report_panel(sampler, label, exact, panel_columns, mean_x_exact)
        finally:
            sampler.set_qoi_panel(None)
    with open(filename, "w") as out:
        for v in data:
            out.write(f"{v:g}\n")
    x_avg = 0.0
    xsq_avg = 0.0
    for k, d in enumerate(data):
        x_avg += (d - x_avg) / (k + 1.0)
        xsq_avg += (d * d - xsq_avg) / (k + 1.0)
    variance = xsq_avg - x_avg * x_avg
    x_error = np.sqrt(variance / sampling_params.nsamples)
    mean_exact, variance_exact = exact.observed_mean_and_variance(y, rows, vals)
    print(f"  {label:>12s} mean     = {x_avg:12.4e} +/- {x_error:12.4e} [ignoring IACT]")
    print(f"  {'exact':>12s} mean     = {mean_exact:12.4e}")
    print(f"  {label:>12s} variance = {variance:12.4e}")
    print(f"  {'exact':>12s} variance = {variance_exact:12.4e}\n")
    return data, (mean_exact, variance_exact)


def convergence_series(sampler, nsamples: int, nsteps: int, rows, vals, batch: int = 1) -> np.ndarray:
    """QoI series z[k, j] of nsamples chains from x = 0, nsteps cycles each (driver_mgmc.cc:236-254).
    Chain k draws sample indices s0 + k nsteps .. s0 + (k+1) nsteps - 1, exactly as one handle running
    the chains one after the other.  batch > 1 runs that many chains at a time on
    clones of the handle, each on its own HIP stream, with those sample indices: the same draws, so
    the same series bit for bit, with the small lattices' idle GPU filled by the concurrent chains.
    A radius > 0 QoI is the device-side dot with the measurement vector on every handle."""
    x0 = np.zeros(sampler.ndof)
    z = np.empty((nsamples, nsteps))
    if batch <= 1:
        for k in range(nsamples):
            sampler.set_state(x0)
            z[k] = _qoi_series(sampler, nsteps, rows, vals)
        return z
    s0 = sampler.get_sample_index()
    handles = [sampler] + [sampler.clone() for _ in range(min(batch, nsamples) - 1)]
    vertex = len(rows) == 1 and vals[0] == 1.0
    if not vertex:  # radius > 0: every handle records the dot with the measurement vector
        for h in handles:
            h.set_qoi_vector(rows, vals)
    q = int(rows[0]) if vertex else mg_native.QOI_VECTOR
    try:
        for k0 in range(0, nsamples, len(handles)):
            ks = list(range(k0, min(k0 + len(handles), nsamples)))
            for h, k in zip(handles, ks):
                h.set_sample_index(s0 + k * nsteps)
                h.set_state(x0)
                h.sample_async(nsteps, q)
            for h, k in zip(handles, ks):
                z[k] = h.get_series(nsteps)
        sampler.set_sample_index(s0 + nsamples * nsteps)
    finally:
        for h in handles[1:]:
            h.close()
    return z


def measure_convergence(sampler, exact: ExactTargets, sampling_params: SamplingParameters,
                        measurement_params: MeasurementParameters, filename: str, batch: int = 1):
    """driver_mgmc.cc:188-314: nsamplesconvergence independent chains from x = 0 (batch: chains run
    concurrently, convergence_series)."""
    op = sampler.get_linear_operator()
    y = _measured_values(measurement_params)
    mean_x_exact = exact.posterior_mean(y) if op.get_m_lowrank() > 0 else np.zeros(op.get_ndof())
    rows, vals = measurement_vector(op.get_lattice(), measurement_params.sample_location, measurement_params.radius)
    sampler.fix_rhs(sampler.operator_apply(0, mean_x_exact))
    nsteps = sampling_params.nstepsconvergence
    nsamples = sampling_params.nsamplesconvergence
    avg = np.zeros((4, nsteps + 1))
    zs = convergence_series(sampler, nsamples, nsteps, rows, vals, batch)
    for k in range(nsamples):
        z = zs[k]
        for j in range(1, nsteps + 1):
            for a in range(4):
                avg[a, j] += (z[j - 1] ** (a + 1) - avg[a, j]) / (k + 1.0)
    mean_exact, variance_exact = exact.observed_mean_and_variance(y, rows, vals)
    x1, x2, x3, x4 = avg
    diff_mean = np.abs(x1 - mean_exact)
    diff_variance = np.abs(x2 - x1 * x1 - variance_exact)
    sigma_sq = nsamples / (nsamples - 1.0) * (x2 - x1 * x1)
    mu4 = x4 - 4 * x1 * x3 + 6 * x1 ** 2 * x2 - 3 * x1 ** 4
    error_mean = np.sqrt(sigma_sq / nsamples)
    error_variance = np.sqrt(np.maximum(mu4 - (nsamples - 3.0) / (nsamples - 1.0) * sigma_sq * sigma_sq, 0.0) / nsamples)
    with open(filename, "w") as out:
        for q, (label, diff, err) in enumerate([("mean", diff_mean, error_mean),
                                                ("variance", diff_variance, error_variance)]):
            out.write("**** q_k = |E[z^k] - E[z]| **** \n" if q == 0 else "**** q_k = |Var[z^k] - Var[z]| **** \n")
            out.write(f"  {'':>12s}   {'k':>3s} : {'q_k':>12s} {'q_k/q_0':>35s} {'q_k/q_{k-1}':>35s}\n")
            for j in range(nsteps + 1):
                out.write(f"  {label:>12s}   {j:3d} : {diff[j]:12.8f} +/- {err[j]:12.8f}       "
                          f"{diff[j] / diff[0]:12.8f} +/- {err[j] / diff[0]:12.8f}      ")
                if j > 0:
                    rel = diff[j] / diff[j - 1] * np.sqrt((err[j] / diff[j]) ** 2 + (err[j - 1] / diff[j - 1]) ** 2)
                    out.write(f" {diff[j] / diff[j - 1]:12.8f} +/- {rel:12.8f} \n")
                else:
                    out.write(f" {'---':>12s}\n")
            out.write("\n")
    return diff_mean, diff_variance


def posterior_statistics(sampler, exact: ExactTargets, sampling_params: SamplingParameters,
                         measurement_params: MeasurementParameters, stderr_batch=None, rao_blackwell=False):
    """driver_mgmc.cc:118-171: the sample mean and the pointwise variance of the field over nsamples
    cycles after nwarmup, to posterior.vtk with the exact mean (2D: the sample location's circle to
    sample_location.vtk).  The moments are accumulated on the device (field_stats): the state never
    leaves HBM.  stderr_batch=B (--stderr-batch B): batch means of B cycles on the device too, and
    posterior.vtk also carries mean_stderr, the Monte Carlo standard error of the mean field, and iact, the
    integrated autocorrelation time per vertex; nsamples must hold at least two batches.
    rao_blackwell=True (--rao-blackwell): the device folds the conditional mean c = x + D^-1 (f - Q x) of every
    vertex given the rest in place of x; mean and variance are then the Rao-Blackwell estimates
    (rao_blackwell_estimates), variance_conditional = 1 / diag(Q) is the part of the variance they know
    exactly, and mean_stderr / iact describe the Rao-Blackwell mean."""
    op = sampler.get_linear_operator()
    y = _measured_values(measurement_params)
    mean_x_exact = exact.posterior_mean(y) if op.get_m_lowrank() > 0 else np.zeros(op.get_ndof())
    sampler.fix_rhs(sampler.operator_apply(0, mean_x_exact))
    sampler.set_state(np.zeros(op.get_ndof()))
    sampler.sample(sampling_params.nwarmup)
    sampler.field_stats(1, batch=stderr_batch, conditional=rao_blackwell)
    fields = {"mean_exact": mean_x_exact}
    try:
        sampler.sample(sampling_params.nsamples)
        if rao_blackwell:
            fields["mean"], fields["variance"] = mean, variance = sampler.field_rb_mean_variance()
            fields["variance_conditional"] = 1.0 / sampler.field_conditional_precision()
        else:
            fields["mean"], fields["variance"] = mean, variance = sampler.field_mean_variance()
        if stderr_batch is not None:
            fields["mean_stderr"] = sampler.field_mean_stderr()[1]
            fields["iact"] = sampler.field_iact()
    finally:
        sampler.field_stats_off()
    write_vtk("posterior.vtk", op.get_lattice(), fields)
    if measurement_params.dim == 2:
        write_vtk_circle(measurement_params.sample_location, measurement_params.radius, "sample_location.vtk")
    return mean, variance, mean_x_exact


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    batch = 1
    stderr_batch = None
    energy_stride = None
    rao_blackwell = False
    qoi_panel = False
    while (len(argv) >= 3 and argv[0] in ("--convergence-batch", "--stderr-batch", "--energy-stride")) or \
            (len(argv) >= 2 and argv[0] in ("--rao-blackwell", "--qoi-panel")):
        if argv[0] == "--rao-blackwell":  # posterior_statistics: the Rao-Blackwell estimates of mean and variance
            rao_blackwell = True
            argv = argv[1:]
            continue
        if argv[0] == "--qoi-panel":  # measure_sampling_time: the predicted data and the QoI as a panel
            qoi_panel = True
            argv = argv[1:]
            continue
        if argv[0] == "--convergence-batch":  # concurrent measure_convergence chains
            batch = int(argv[1])
        elif argv[0] == "--energy-stride":  # measure_sampling_time: x^T Q x, f^T x of every S-th sample
            energy_stride = int(argv[1])
        else:  # posterior_statistics: batch means of this many cycles (mean_stderr and iact in posterior.vtk)
            stderr_batch = int(argv[1])
        argv = argv[2:]
    if len(argv) != 1:
        print(f"Usage: {sys.argv[0]} [--convergence-batch N] [--stderr-batch B] [--energy-stride S] "
              "[--rao-blackwell] [--qoi-panel] CONFIGURATIONFILE")
        return -1
    t_start = time.time()
    print("\n+--------------------------------+")
    print("! Multigrid Monte Carlo sampling !")
    print("+--------------------------------+\n")
    print(f"Starting run at {datetime.datetime.now().ctime()}\n")
    filename = argv[0]
    print(f"Reading parameters from file '{filename}'")
    cfg = read_config(filename)
    base = os.path.dirname(os.path.abspath(filename))
    general = GeneralParameters.from_config(cfg)
    lattice_params = LatticeParameters.from_config(cfg)
    mg_params = MultigridParameters.from_config(cfg)
    sampling_params = SamplingParameters.from_config(cfg)
    prior_params = PriorParameters.from_config(cfg)
    try:
        measurement_params = MeasurementParameters.from_config(cfg, base)
    except MeasurementFileError as e:  # parameters.cc:273-276: message on stderr, exit(-1)
        print(str(e), file=sys.stderr)
        return -1
    if measurement_params.dim != general.dim:
        print("ERROR: dimension of measurement locations differs from problem dimension")
        return -1
    if general.dim == 2:
        lattice = Lattice(lattice_params.nx, lattice_params.ny)
    elif general.dim == 3:
        lattice = Lattice(lattice_params.nx, lattice_params.ny, lattice_params.nz)
    else:
        print(f"ERROR: Invalid dimension : {general.dim}")
        return -1
    # driver_mgmc.cc:398-429
    try:
        if prior_params.correlationlength_model == "constant":
            model = ConstantCorrelationLengthModel(ConstantCorrelationLengthModelParameters.from_config(cfg).Lambda)
        elif prior_params.correlationlength_model == "periodic":
            pp = PeriodicCorrelationLengthModelParameters.from_config(cfg)
            model = PeriodicCorrelationLengthModel(pp.Lambda_min, pp.Lambda_max)
        else:
            print(f"Error: invalid correlationlengthmodel '{prior_params.correlationlength_model}'")
            return -1
    except ConfigError as e:
        print(str(e))
        return -1
    prior_classes = {"shiftedlaplace_fd": ShiftedLaplaceFDOperator, "shiftedlaplace_fem": ShiftedLaplaceFEMOperator,
                     "squared_shiftedlaplace_fd": SquaredShiftedLaplaceFDOperator}
    if prior_params.pde_model not in prior_classes:
        print(f"Error: invalid prior '{prior_params.pde_model}'")
        return -1
    try:
        prior = prior_classes[prior_params.pde_model](lattice, model)
    except ValueError as e:  # squared_shiftedlaplace_fd in 3D (squared_shiftedlaplace_fd_operator.cc:15-19)
        print(f"ERROR: {e}")
        return -1
    posterior = MeasuredOperator(prior, measurement_params)
    if general.operator_name == "prior":
        linear_operator = prior
    elif general.operator_name == "posterior":
        linear_operator = posterior
    else:
        print(f"ERROR: invalid operator : {general.operator_name}")
        return -1
    sampler = MultigridMCSampler(linear_operator, SEED, mg_params)
    # the exact observed statistics always refer to the measured operator (driver_mgmc.cc:58-60)
    solver_sampler = sampler if linear_operator is posterior else MultigridMCSampler(posterior, SEED, mg_params)
    exact = ExactTargets(solver_sampler)
    print()
    for flag, name in ((general.do_cholesky, "Cholesky"), (general.do_ssor, "SSOR")):
        if flag:
            print(f"**** {name} **** skipped: the whole-lattice {name} sampler is not on the device path\n")
    if general.do_multigridmc:
        print("**** Multigrid MC ****")
        measure_sampling_time(sampler, exact, sampling_params, measurement_params, "MGMC",
                              "timeseries_multigridmc.txt", energy_stride, posterior if qoi_panel else None)
        measure_convergence(sampler, exact, sampling_params, measurement_params, "convergence_multigridmc.txt",
                            batch)
        if general.save_posterior_statistics:
            posterior_statistics(sampler, exact, sampling_params, measurement_params, stderr_batch, rao_blackwell)
            print("  posterior_statistics: mean, variance and mean_exact written to posterior.vtk"
                  + ("; Rao-Blackwell estimates, with variance_conditional" if rao_blackwell else "")
                  + ("" if stderr_batch is None else f"; mean_stderr and iact from batches of {stderr_batch} cycles"))
        print()
    secs = int(time.time() - t_start)
    print(f"Completed run at {datetime.datetime.now().ctime()}")
    print(f"Total elapsed time = {secs // 3600:3d} h {(secs // 60) % 60:2d} m {secs % 60:2d} s\n")
    if solver_sampler is not sampler:
        solver_sampler.close()
    sampler.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
