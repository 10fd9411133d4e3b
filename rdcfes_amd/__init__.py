"""rdcfes_amd — MI355X-native element assembly for the rdcFEs reaction-diffusion-convection models.

The compute path is the HIP library ``lib/librdc_assembly.so`` (C-ABI in ``include/rdc_assembly.h``).
This Python package is the test / benchmark harness above that ABI plus the host-side partitioning
logic; it contains no numerical fallback: without the built library and a GPU every compute call
raises.
"""
from .params import (PihnaParams, RipfParams, HccParams, SolidParams, SolidMaterial, RipfCheckParams, AdpmParams, ProteasParams, PihnaRanges, RipfRanges, AdpmRanges, SolveParams, SolveInfo,
                     pihna_params_from_dict, ripf_params_from_dict, hcc_params_from_dict,
                     adpm_params_from_dict, proteas_params_from_dict)
from .context import (AssemblyContext, RdcError, TET4, HEX8, SCATTER_AUTO, SCATTER_COLOURED,
                      SCATTER_ROWGATHER, FIELD_OLD_SOLUTION, FIELD_AUX_NODAL,
                      FIELD_UNDEFORMED_XYZ, FIELD_ELEM_FIBRE, FIELD_PREV_SOLUTION, FIELD_TIME_DERIV,
                      FIELD_RT_DOSE, FIELD_ELEM_TRACTS, PRECOND_NONE, PRECOND_JACOBI, PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, PRECOND_ILU0, PRECOND_ILU0_LOCAL, PRECOND_MULTIGRID_GS_LOCAL,
                      SOLVE_CONVERGED, SOLVE_MAX_ITS, SOLVE_BREAKDOWN, SOLVE_BAD_DIAGONAL, SOLVE_NOT_FINITE, ERR_COMM,
                      NEWTON_CONVERGED_RESIDUAL, NEWTON_CONVERGED_STEP, NEWTON_MAX_ITS, NEWTON_LINEAR_FAILED, NEWTON_NOT_FINITE)
from .params import SolidNewtonParams, SolidNewtonInfo


def __getattr__(name):
    # halo.py needs torch; the rest of the package imports without it
    if name == "SolveComm":
        from .halo import SolveComm
        return SolveComm
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = [
    "PihnaParams", "RipfParams", "HccParams", "SolidParams", "SolidMaterial", "RipfCheckParams", "AdpmParams", "adpm_params_from_dict", "ProteasParams", "proteas_params_from_dict", "PihnaRanges", "RipfRanges", "AdpmRanges",
    "pihna_params_from_dict", "ripf_params_from_dict", "hcc_params_from_dict",
    "AssemblyContext", "RdcError", "TET4", "HEX8", "SCATTER_AUTO", "SCATTER_COLOURED",
    "SCATTER_ROWGATHER", "FIELD_OLD_SOLUTION", "FIELD_AUX_NODAL", "FIELD_UNDEFORMED_XYZ",
    "FIELD_ELEM_FIBRE", "FIELD_PREV_SOLUTION", "FIELD_TIME_DERIV", "FIELD_RT_DOSE", "FIELD_ELEM_TRACTS",
    "SolveParams", "SolveInfo", "PRECOND_NONE", "PRECOND_JACOBI", "PRECOND_BLOCK_JACOBI", "PRECOND_MULTIGRID", "PRECOND_ILU0", "PRECOND_ILU0_LOCAL", "PRECOND_MULTIGRID_GS_LOCAL",
    "SOLVE_CONVERGED", "SOLVE_MAX_ITS", "SOLVE_BREAKDOWN", "SOLVE_BAD_DIAGONAL", "SOLVE_NOT_FINITE", "ERR_COMM", "SolveComm",
    "SolidNewtonParams", "SolidNewtonInfo", "NEWTON_CONVERGED_RESIDUAL", "NEWTON_CONVERGED_STEP", "NEWTON_MAX_ITS", "NEWTON_LINEAR_FAILED",
    "NEWTON_NOT_FINITE",
]
