"""numpy restatement of rdc_solve_mixed (rdcfes_amd/csrc/rdc_solve.hip): the algorithm of solve_ref.bicgstab with the two
operator applications INSIDE an iteration replaced by A32 @ y, A32 = fl32(D^-1 A) held as float64 (values rounded to fp32,
accumulation in fp64).  Everything that decides -- the first residual, the confirmation of a claimed convergence, the
restart, the closing residual -- stays M @ (b - A @ x) in fp64, with the flags and the break-down count of solve_ref.
Yardstick for the iteration counts of the mixed GPU tests."""
import numpy as np

import solve_ref
from solve_ref import BREAKDOWN, CONVERGED, MAX_BREAKDOWNS, MAX_ITS, NOT_FINITE, precond_inverse


def scaled_f32(A, nv, precond):
    """fl32(D^-1 A) as a float64 CSR matrix"""
    M, _, _ = precond_inverse(A, nv, precond)
    S = (M @ A).tocsr()
    with np.errstate(over="ignore"):
        S.data = S.data.astype(np.float32).astype(np.float64)
    return S


def bicgstab(A, b, x0, rel_tol, abs_tol=0.0, max_its=10000, precond=2, nv=1):
    """-> (x, dict(reason, iterations, restarts, rhs_norm, residual_norm)), as solve_ref.bicgstab"""
    M, _, _ = precond_inverse(A, nv, precond)
    A32 = scaled_f32(A, nv, precond)
    x = np.array(x0, dtype=np.float64, copy=True)
    info = dict(reason=CONVERGED, iterations=0, restarts=0)
    bn = float(np.linalg.norm(M @ b))
    info["rhs_norm"] = bn

    def restart():
        r = M @ (b - A @ x)
        return r, r.copy(), np.zeros_like(r), np.zeros_like(r), float(r @ r), 1.0, 1.0, 0.0

    def done(reason, rn2):
        info["reason"], info["residual_norm"] = reason, float(np.sqrt(rn2))
        return x, info

    r, rh, p, v, rn2, alpha, omega, beta = restart()
    rho = rn2
    if not (np.isfinite(bn) and np.isfinite(rn2)):
        return done(NOT_FINITE, rn2)
    if bn == 0.0:
        x[:] = 0.0
        return done(CONVERGED, 0.0)
    tol = max(rel_tol * bn, abs_tol)
    if np.sqrt(rn2) <= tol:
        return done(CONVERGED, rn2)
    breakdowns = 0
    while True:
        if info["iterations"] >= max_its:
            r = M @ (b - A @ x)
            rn2 = float(r @ r)
            return done(CONVERGED if np.sqrt(rn2) <= tol else MAX_ITS, rn2)
        info["iterations"] += 1
        flag = 0
        with np.errstate(all="ignore"):
            p = r + beta * (p - omega * v)
            v = A32 @ p
            r0v = float(rh @ v)
            alpha = rho / r0v if r0v != 0.0 else np.inf
            if r0v == 0.0 or not np.isfinite(alpha):
                flag = 1
            if not flag:
                s = r - alpha * v
                t = A32 @ s
                ts, tt = float(t @ s), float(t @ t)
                omega = ts / tt if tt > 0.0 else 0.0
                if omega == 0.0 or not np.isfinite(omega):
                    flag = 1
            if not flag:
                x += alpha * p + omega * s
                r = s - omega * t
                rho1, rn2 = float(rh @ r), float(r @ r)
                beta = (rho1 / rho) * (alpha / omega)
                rho = rho1
                if not (np.isfinite(rn2) and np.isfinite(beta)):
                    flag = 1
                elif rho1 == 0.0:
                    flag = 2
        claims = not (flag & 1) and np.sqrt(rn2) <= tol
        if not claims and not flag:
            continue
        if not claims:
            breakdowns += 1
        r, rh, p, v, rn2, alpha, omega, beta = restart()
        rho = rn2
        if not claims and breakdowns > MAX_BREAKDOWNS:
            return done(BREAKDOWN if np.isfinite(rn2) else NOT_FINITE, rn2)
        if not np.isfinite(rn2):
            return done(NOT_FINITE, rn2)
        if np.sqrt(rn2) <= tol:
            return done(CONVERGED, rn2)
        info["restarts"] += 1


__all__ = ["bicgstab", "scaled_f32", "solve_ref"]
