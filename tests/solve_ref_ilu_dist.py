"""numpy yardstick of the rank-local block ILU(0) of the partitioned solve (RDC_PRECOND_ILU0_LOCAL = 5; rdc_solve_dist): block Jacobi
between the ranks, ILU(0) inside each, which is what PETSc runs by default under mpirun.

Built on tests/solve_ref_dist.py (the ranks of a system, the exchange through the send lists, inner products as the sum in rank
order of the ranks' own sums) and tests/solve_ref_ilu.py: every rank factors the OWNED SQUARE of its rows, A[:, :n_owned * nv] --
its greedy colours are those of the owned nodes in local order, the blocks in ghost columns are left out of the factor -- and
M = diag over the ranks of (L U)^-1 is applied from the right on block Jacobi's system, as solve_ref.bicgstab applies a right
preconditioner: the operator sees M p and M s, x advances along them, everything that decides stays D^-1 (b - A x).  An apply
needs no exchange; the ghost tails of M p and M s are filled by the exchange of the operator application that follows.

bicgstab_dist restates the driver of solve_ref_dist.bicgstab_dist with that hook (the file it is built on has none and stays as
it is).  With one rank the owned square is the matrix and this is solve_ref_ilu.bicgstab."""
import numpy as np

import solve_ref
import solve_ref_dist
import solve_ref_ilu
from solve_ref import BREAKDOWN, CONVERGED, MAX_BREAKDOWNS, MAX_ITS, NOT_FINITE

_YARD = {}


def owned_square(rk, nv):
    """the rows of a rank over its owned columns: what the rank factors"""
    return rk.A[:, :rk.lp.n_owned * nv].tocsr()


def factors(ranks, nv, dtype=np.float64):
    """[solve_ref_ilu.Factor] of every rank's owned square"""
    return [solve_ref_ilu.Factor(owned_square(rk, nv), nv, dtype=dtype) for rk in ranks]


def bicgstab_dist(ranks, x0s, rel_tol, abs_tol=0.0, max_its=10000, nv=1, right=None):
    """solve_ref_dist.bicgstab_dist with precond = 2 and right[r](owned vector of rank r) applied from the right (None: the
    factors of the owned squares) -> (xs, info)"""
    right = right or [f.apply for f in factors(ranks, nv)]
    R = range(len(ranks))
    no = [rk.lp.n_owned * nv for rk in ranks]
    M = [solve_ref.precond_inverse(owned_square(rk, nv), nv, 2)[0] for rk in ranks]
    xs = [np.array(x, dtype=np.float64, copy=True) for x in x0s]
    dot = lambda a, b: float(sum(float(a[r] @ b[r]) for r in R))   # rank-wise, then over the ranks in order

    def A_of(vecs):      # exchange, then every rank's rows
        solve_ref_dist.exchange(ranks, vecs, nv)
        return [ranks[r].A @ vecs[r] for r in R]

    def operator(owned):
        ax = A_of([np.concatenate([owned[r], np.zeros(ranks[r].A.shape[1] - no[r])]) for r in R])
        return [M[r] @ ax[r] for r in R]

    info = dict(reason=CONVERGED, iterations=0, restarts=0)
    mb = [M[r] @ ranks[r].b for r in R]
    bn = float(np.sqrt(dot(mb, mb)))
    info["rhs_norm"] = bn

    def restart():
        ax = A_of(xs)
        r_ = [M[r] @ (ranks[r].b - ax[r]) for r in R]
        z = [np.zeros_like(v) for v in r_]
        return r_, [v.copy() for v in r_], z, [v.copy() for v in z], dot(r_, r_), 1.0, 1.0, 0.0

    def done(reason, rn2):
        info["reason"], info["residual_norm"] = reason, float(np.sqrt(rn2))
        return xs, info

    r_, rh, p, v, rn2, alpha, omega, beta = restart()
    rho = rn2
    if not (np.isfinite(bn) and np.isfinite(rn2)):
        return done(NOT_FINITE, rn2)
    if bn == 0.0:
        for x in xs:
            x[:] = 0.0
        return done(CONVERGED, 0.0)
    tol = max(rel_tol * bn, abs_tol)
    if np.sqrt(rn2) <= tol:
        return done(CONVERGED, rn2)
    breakdowns = 0
    while True:
        if info["iterations"] >= max_its:
            _, _, _, _, rn2, _, _, _ = restart()
            return done(CONVERGED if np.sqrt(rn2) <= tol else MAX_ITS, rn2)
        info["iterations"] += 1
        flag = 0
        with np.errstate(all="ignore"):
            p = [r_[r] + beta * (p[r] - omega * v[r]) for r in R]
            px = [right[r](p[r]) for r in R]
            v = operator(px)
            r0v = dot(rh, v)
            alpha = rho / r0v if r0v != 0.0 else np.inf
            if r0v == 0.0 or not np.isfinite(alpha):
                flag = 1
            if not flag:
                s = [r_[r] - alpha * v[r] for r in R]
                sx = [right[r](s[r]) for r in R]
                t = operator(sx)
                ts, tt = dot(t, s), dot(t, t)
                omega = ts / tt if tt > 0.0 else 0.0
                if omega == 0.0 or not np.isfinite(omega):
                    flag = 1
            if not flag:
                for r in R:
                    xs[r][:no[r]] += alpha * px[r] + omega * sx[r]
                r_ = [s[r] - omega * t[r] for r in R]
                rho1, rn2 = dot(rh, r_), dot(r_, r_)
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
        r_, rh, p, v, rn2, alpha, omega, beta = restart()
        rho = rn2
        if not claims and breakdowns > MAX_BREAKDOWNS:
            return done(BREAKDOWN if np.isfinite(rn2) else NOT_FINITE, rn2)
        if not np.isfinite(rn2):
            return done(NOT_FINITE, rn2)
        if np.sqrt(rn2) <= tol:
            return done(CONVERGED, rn2)
        info["restarts"] += 1


def yardstick(name, world, O, rel_tol):
    """(gathered x, info) of bicgstab_dist on solve_ref_dist.ranks_of(name, world) from x0 = 0; computed once.  World 1 is one rank
    that owns every node: the oracle's global assembly."""
    key = (name, world, rel_tol)
    if key not in _YARD:
        s = solve_ref_dist.case(name)
        ranks = solve_ref_dist.ranks_of(name, world, O)
        fk = (name, world, "factors")
        if fk not in _YARD:
            _YARD[fk] = [f.apply for f in factors(ranks, s.nv)]
        xs, info = bicgstab_dist(ranks, [np.zeros(rk.A.shape[1]) for rk in ranks], rel_tol, nv=s.nv, max_its=2000, right=_YARD[fk])
        _YARD[key] = (solve_ref_dist.gather(ranks, xs, s.nv, s.xyz.shape[0]), info)
    return _YARD[key]
