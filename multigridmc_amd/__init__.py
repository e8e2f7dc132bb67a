"""multigridmc_amd -- MI355X-native Multigrid Monte Carlo sampler (HIP / gfx950).

The hot path (one MGMC cycle: multicolour Gibbs sweeps with fused Philox noise, fused
residual+restriction, prolongate-add, single-workgroup coarse SSOR sampler) lives in
csrc/*.hip behind the C-ABI of include/mgmc.h; this package is the host-side mirror of the
reference's Sampler / LinearOperator interfaces.
"""
from ._native import QOI_VECTOR, MgmcError, load_library  # noqa: F401
from .measured import (  # noqa: F401
    LowRankUpdate,
    MeasuredOperator,
    measurement_panel,
    measurement_vector,
    synthetic_posterior,
)
from .parameters import MultigridParameters, read_config  # noqa: F401
from .sampler import (  # noqa: F401
    BACKWARD,
    FORWARD,
    HipMulticolourSORSmoother,
    Lattice,
    Lattice2d,
    Lattice3d,
    MultigridMCSampler,
    ShiftedLaplaceFDOperator,
    ShiftedLaplaceFEMOperator,
    SquaredShiftedLaplaceFDOperator,
    SparseMatrixOperator,
    SORSmoother,
    SORSmootherFactory,
    SSORSmoother,
    SSORSmootherFactory,
    ConstantCorrelationLengthModel,
    PeriodicCorrelationLengthModel,
    PanelStatistics,
    batch_means_estimates,
    panel_statistics,
    tau_int_from_autocov,
    rao_blackwell_estimates,
    comm_unique_id,
    csr_colour_scheme,
    describe,
    make_config,
    measurement_vector_index,
    sampler_csr_matrix,
)
from .vtk import write_vtk, write_vtk_circle  # noqa: F401

__version__ = "0.1.0"
