"""numpy / scipy restatement of the algorithm of rdc_solve (rdcfes_amd/csrc/rdc_solve.hip: run, iteration): BiCGStab, LEFT-preconditioned
by node-block Jacobi (2), point Jacobi (1) or nothing (0), the recurrences of the host mirror's bicgstab_ilu0, the
stopping test on the preconditioned residual ||D^-1 (b - A x)|| <= max(rel_tol ||D^-1 b||, abs_tol), the true residual
recomputed whenever the recurrence claims convergence or breaks down (that recomputation IS the restart: r_hat = r,
p = v = 0).  Yardstick for the iteration counts of the GPU tests, and the place where the residual checks those tests
apply are written down once (check_solution).  bicgstab is the only driver: solve_ref_mixed and solve_ref_mg call it with
the operator of an iteration, or a right preconditioner, of their own."""
import numpy as np
import scipy.sparse as sps

CONVERGED, MAX_ITS, BREAKDOWN, BAD_DIAGONAL, NOT_FINITE = 0, 1, 2, 3, 4
MAX_BREAKDOWNS = 10
EPS = np.finfo(np.float64).eps


def diag_blocks(A, nv):
    """[n_nodes][nv][nv] diagonal blocks of a scalar CSR matrix with dof = node * nv + var"""
    n = A.shape[0] // nv
    B = sps.bsr_matrix(A, blocksize=(nv, nv))
    B.sort_indices()
    out = np.zeros((n, nv, nv))
    rows = np.repeat(np.arange(n), np.diff(B.indptr))
    on = B.indices == rows
    out[rows[on]] = B.data[on]
    return out


def precond_inverse(A, nv, precond):
    """(D^-1 as a sparse block-diagonal matrix, its dense blocks, max cond_inf of the blocks of D)"""
    n = A.shape[0] // nv
    D = diag_blocks(A, nv)
    if precond == 1:
        D = D * np.eye(nv)[None]
    elif precond == 0:
        D = np.broadcast_to(np.eye(nv), D.shape).copy()
    Di = np.linalg.inv(D)
    cond = float((np.abs(D).sum(axis=2).max(axis=1) * np.abs(Di).sum(axis=2).max(axis=1)).max())
    M = sps.bsr_matrix((Di, np.arange(n), np.arange(n + 1)), shape=A.shape).tocsr()
    return M, Di, cond


def bicgstab(A, b, x0, rel_tol, abs_tol=0.0, max_its=10000, precond=2, nv=1, operator=None, right=None):
    """-> (x, dict(reason, iterations, restarts, rhs_norm, residual_norm)).  The one driver of every yardstick; two hooks:
    operator(y): what the two applications INSIDE an iteration compute, default M @ (A @ y) (solve_ref_mixed: the fp32 copy);
    right(y): a right preconditioner (solve_ref_mg: the cycle), whose outputs take the place of p and s in those two
    applications and in the update of x.  Everything that decides stays M @ (b - A @ x) whatever the hooks are."""
    M, _, _ = precond_inverse(A, nv, precond)
    if operator is None:
        def operator(y):
            return M @ (A @ y)
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
            px = right(p) if right else p
            v = operator(px)
            r0v = float(rh @ v)
            alpha = rho / r0v if r0v != 0.0 else np.inf
            if r0v == 0.0 or not np.isfinite(alpha):
                flag = 1
            if not flag:
                s = r - alpha * v
                sx = right(s) if right else s
                t = operator(sx)
                ts, tt = float(t @ s), float(t @ t)
                omega = ts / tt if tt > 0.0 else 0.0
                if omega == 0.0 or not np.isfinite(omega):
                    flag = 1
            if not flag:
                x += alpha * px + omega * sx
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


def longest_row(A):
    return int(np.diff(A.indptr).max())


def check_solution(A, b, x, nv, precond, rel_tol, extra_rel=0.0):
    """The residual inequality the solver tests hold a returned x to, with A, b given and D^-1 formed here by numpy:

      ||D^-1 (b - A x)|| <= (1 + 64 eps max cond_inf(D_block)) rel_tol ||D^-1 b|| + rho,
      rho = (4 L eps + extra_rel) || |D^-1| (|A||x| + |b|) ||,    L = longest row in entries

    globally and for the rows of every unknown taken alone.  rho is the rounding of evaluating such a residual at all
    (extra_rel: the tolerance of an assembly that produced A, b).  Returns the figures; raises AssertionError."""
    M, _, cond = precond_inverse(A, nv, precond)
    res = M @ (b - A @ x)
    bn = float(np.linalg.norm(M @ b))
    scale = abs(M) @ (abs(A) @ np.abs(x) + np.abs(b))
    fac = 4.0 * longest_row(A) * EPS + extra_rel
    rho = fac * float(np.linalg.norm(scale))
    bound = (1.0 + 64.0 * EPS * cond) * rel_tol * bn + rho
    rn = float(np.linalg.norm(res))
    out = dict(residual_norm=rn, rhs_norm=bn, rho=rho, bound=bound, cond=cond,
               plain_residual_norm=float(np.linalg.norm(b - A @ x)), plain_rhs_norm=float(np.linalg.norm(b)),
               plain_rho=fac * float(np.linalg.norm(abs(A) @ np.abs(x) + np.abs(b))), per_unknown=[])
    assert np.all(np.isfinite(x)), "x is not finite"
    assert rn <= bound, f"||D^-1(b - Ax)|| = {rn:.3e} > {bound:.3e} (rel_tol {rel_tol:g}, ||D^-1 b|| {bn:.3e}, rho {rho:.3e})"
    for a in range(nv):
        ra = float(np.linalg.norm(res[a::nv]))
        ba = (1.0 + 64.0 * EPS * cond) * rel_tol * bn + fac * float(np.linalg.norm(scale[a::nv]))
        out["per_unknown"].append((ra, ba))
        assert ra <= ba, f"unknown {a}: ||D^-1(b - Ax)||_rows = {ra:.3e} > {ba:.3e}"
    return out
