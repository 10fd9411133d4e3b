"""numpy restatement of rdc_solve_mixed (rdcfes_amd/csrc/rdc_solve.hip): solve_ref.bicgstab itself, with the two
operator applications INSIDE an iteration replaced by A32 @ y (its `operator` hook), A32 = fl32(D^-1 A) held as float64 (values rounded to fp32,
accumulation in fp64).  Everything that decides -- the first residual, the confirmation of a claimed convergence, the
restart, the closing residual -- stays M @ (b - A @ x) in fp64, with the flags and the break-down count of solve_ref.
Yardstick for the iteration counts of the mixed GPU tests."""
import numpy as np

import solve_ref
from solve_ref import precond_inverse


def scaled_f32(A, nv, precond):
    """fl32(D^-1 A) as a float64 CSR matrix"""
    M, _, _ = precond_inverse(A, nv, precond)
    S = (M @ A).tocsr()
    with np.errstate(over="ignore"):
        S.data = S.data.astype(np.float32).astype(np.float64)
    return S


def bicgstab(A, b, x0, rel_tol, abs_tol=0.0, max_its=10000, precond=2, nv=1):
    """-> (x, dict(reason, iterations, restarts, rhs_norm, residual_norm)), as solve_ref.bicgstab"""
    A32 = scaled_f32(A, nv, precond)
    return solve_ref.bicgstab(A, b, x0, rel_tol, abs_tol, max_its, precond, nv, operator=lambda y: A32 @ y)


__all__ = ["bicgstab", "scaled_f32", "solve_ref"]
