"""numpy restatement of the GMRES path of rdc_solve (rdcfes_amd/csrc/rdc_solve.hip: run_gmres, gmres_step; the option "solve_method" = 1):
right-preconditioned restarted GMRES(m) on block Jacobi's system D^-1 A x = D^-1 b, classical Gram-Schmidt (one pass, or two with
refine), Givens rotations on the Hessenberg matrix, the stopping test of solve_ref.bicgstab on the preconditioned residual, and the
TRUE residual M @ (b - A @ x) at the start of every cycle, which alone decides.  It takes the hooks of solve_ref.bicgstab:
operator(y) is what an Arnoldi step applies (default M @ (A @ y); solve_ref_mixed: the fp32 copy), right(y) a right preconditioner
(the multigrid cycle, the ILU(0) sweeps).  The one yardstick for the iteration counts of the GMRES tests.

arnoldi() is the Arnoldi process alone, in any dtype: the extended-precision form is what tests/test_gpu_solve_gmres.py holds the
device's basis and Hessenberg matrix to."""
import numpy as np

import solve_ref

CONVERGED, MAX_ITS, BREAKDOWN, BAD_DIAGONAL, NOT_FINITE = 0, 1, 2, 3, 4


def arnoldi(op, v0, steps, refine=False, dtype=np.float64):
    """-> (V [done + 1][n], H [steps + 1][steps] raw, done): v_0 = v0 / ||v0||, then per step w = op(v_j), h = V_j^T w, w -= V_j h
    (refine: once more, the second h added to the first), h_{j+1,j} = ||w||, v_{j+1} = w / h_{j+1,j}.  Stops behind a step whose
    h_{j+1,j} is 0."""
    v0 = np.asarray(v0, dtype=dtype)
    V = np.zeros((steps + 1, v0.size), dtype=dtype)
    H = np.zeros((steps + 1, steps), dtype=dtype)
    V[0] = v0 / np.sqrt(v0 @ v0)
    done = 0
    for j in range(steps):
        w = np.asarray(op(V[j]), dtype=dtype)
        for _ in range(2 if refine else 1):
            h = V[:j + 1] @ w
            w = w - h @ V[:j + 1]
            H[:j + 1, j] += h
        hn = np.sqrt(w @ w)
        H[j + 1, j] = hn
        done = j + 1
        if hn == 0:
            break
        V[j + 1] = w / hn
    return V[:done + 1], H, done


def givens_step(j, hcol, cs, sn, g):
    """gmres_givens_step of rdc_solve.h: the rotated column (rows 0 .. j + 1), or None if the column cannot be taken"""
    r = np.array(hcol[:j + 2], dtype=np.float64)
    if not np.all(np.isfinite(r)):
        return None
    for i in range(j):
        a, b = r[i], r[i + 1]
        r[i], r[i + 1] = cs[i] * a + sn[i] * b, cs[i] * b - sn[i] * a
    d = float(np.hypot(r[j], r[j + 1]))
    if not np.isfinite(d) or d == 0.0:
        return None
    cs[j], sn[j] = r[j] / d, r[j + 1] / d
    r[j], r[j + 1] = d, 0.0
    g[j + 1] = -sn[j] * g[j]
    g[j] = cs[j] * g[j]
    return r


def back_substitute(R, g, k):
    y = np.zeros(k)
    for i in range(k - 1, -1, -1):
        y[i] = (g[i] - R[i, i + 1:k] @ y[i + 1:k]) / R[i, i]
    return y


def gmres(A, b, x0, rel_tol, abs_tol=0.0, max_its=10000, precond=2, nv=1, operator=None, right=None, restart=30, refine=False):
    """-> (x, dict(reason, iterations, restarts, cycles, rhs_norm, residual_norm)).  iterations = Arnoldi steps, restarts = cycles
    begun after the first."""
    M, _, _ = solve_ref.precond_inverse(A, nv, precond)
    if operator is None:
        def operator(y):
            return M @ (A @ y)
    x = np.array(x0, dtype=np.float64, copy=True)
    info = dict(reason=CONVERGED, iterations=0, restarts=0, cycles=0)
    bn = float(np.linalg.norm(M @ b))
    info["rhs_norm"] = bn

    def done(reason, rn):
        info["reason"], info["residual_norm"] = reason, float(rn)
        return x, info

    r = M @ (b - A @ x)
    rn = float(np.sqrt(r @ r))
    if not (np.isfinite(bn) and np.isfinite(rn)):
        return done(NOT_FINITE, rn)
    if bn == 0.0:
        x[:] = 0.0
        return done(CONVERGED, 0.0)
    tol = max(rel_tol * bn, abs_tol)
    if rn <= tol:
        return done(CONVERGED, rn)
    m = restart
    while True:
        info["cycles"] += 1
        V = np.zeros((m + 1, x.size))
        R = np.zeros((m + 1, m))
        cs, sn, g = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        V[0], g[0] = r / rn, rn
        k, bad = 0, False
        with np.errstate(all="ignore"):
            while k < m and info["iterations"] < max_its:
                j = k
                w = operator(right(V[j]) if right else V[j])
                info["iterations"] += 1
                hcol = np.zeros(j + 2)
                for _ in range(2 if refine else 1):
                    h = V[:j + 1] @ w
                    w = w - h @ V[:j + 1]
                    hcol[:j + 1] += h
                hcol[j + 1] = np.sqrt(w @ w)
                col = givens_step(j, hcol, cs, sn, g)
                if col is None:
                    bad = True
                    break
                R[:j + 2, j] = col
                k += 1
                if hcol[j + 1] == 0.0:
                    break
                V[j + 1] = w / hcol[j + 1]
                if abs(g[k]) <= tol:
                    break
            if k > 0:
                u = back_substitute(R, g, k) @ V[:k]
                x += right(u) if right else u
        r = M @ (b - A @ x)
        rn = float(np.sqrt(r @ r))
        if not np.isfinite(rn) or (bad and not np.all(np.isfinite(hcol))):
            return done(NOT_FINITE, rn)
        if rn <= tol:
            return done(CONVERGED, rn)
        if bad:
            return done(BREAKDOWN, rn)
        if info["iterations"] >= max_its:
            return done(MAX_ITS, rn)
        info["restarts"] += 1
