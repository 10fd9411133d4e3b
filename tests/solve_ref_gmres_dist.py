"""numpy yardstick of GMRES across ranks (rdc_solve_dist_gmres, rdc_solve_dist_gmres_arnoldi): right-preconditioned GMRES(m) of
tests/solve_ref_gmres.py on the GLOBAL system, with the right preconditioners of the partitioned solves built from what the ranks hold.

Block Jacobi couples nothing across ranks, so for precond 0, 1 and 2 the partitioned GMRES is mathematically the GMRES of the global
system: the yardstick is plain solve_ref_gmres.gmres on it.  For precond 5 `right` is the rank-block-diagonal ILU(0) apply on the
owned squares (solve_ref_ilu_dist.factors), for precond 3 the cycle of solve_ref_mg_dist.HierarchyDist, both wrapped to act on
global vectors: the owned rows of rank r are the global dofs dofs[r].

operators() gives the Arnoldi tests the operator v -> D^-1 A (M v) of a global matrix in FP64 and in extended precision, in the
RANK ORDER of solve_ref_mg_dist.rank_order (the ranks' owned rows one behind the other), where M is block diagonal by ranges and the
rank-local hierarchy is solve_ref_mg_dist.EmulatedHierarchy, which tests/solve_ref_mg_ld.py can run in extended precision."""
import numpy as np
import scipy.sparse as sps

import solve_ref
import solve_ref_dist
import solve_ref_gmres
import solve_ref_ilu
import solve_ref_ilu_dist
import solve_ref_mg
import solve_ref_mg_dist
import solve_ref_mg_ld as ld

LD = np.longdouble
_RIGHT, _YARD = {}, {}
TOLS = (1e-8, 1e-10)
# (system, world, precond, restart, refine) of the partitioned solves the GPU test runs; the last gives many restarts and, with the
# second Gram-Schmidt pass, three all-reduces per step.  (The hydrogel mesh with block Jacobi stagnates and is not among them.)
CASES = [(name, world, precond, 30, False) for name, world in (("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("pihna_kuhn3", 3))
         for precond in (2, 5, 3)] + [("pihna_kuhn", 2, 2, 7, True)]


def rank_dofs(ranks, nv):
    """per rank the global dofs of its owned rows, in its local order"""
    return [(rk.lp.node_global[:rk.lp.n_owned].astype(np.int64)[:, None] * nv + np.arange(nv)).reshape(-1) for rk in ranks]


def on_global(apply_owned, dofs):
    """apply_owned([owned vector per rank]) -> [owned vector per rank], as a map of global vectors"""
    def right(y):
        parts = apply_owned([y[d] for d in dofs])
        out = np.zeros(y.size, dtype=np.result_type(*[p.dtype for p in parts]))
        for d, p in zip(dofs, parts):
            out[d] = p
        return out
    return right


def right_of(ranks, nv, precond):
    """the right preconditioner of `precond` across `ranks` on global vectors (None for 0, 1, 2)"""
    dofs = rank_dofs(ranks, nv)
    if precond == 5:
        fs = solve_ref_ilu_dist.factors(ranks, nv)
        assert all(f.singular == 0 for f in fs)
        return on_global(lambda parts: [f.apply(p) for f, p in zip(fs, parts)], dofs)
    if precond == 3:
        return on_global(solve_ref_mg_dist.HierarchyDist(ranks, nv).cycle, dofs)
    assert precond in (0, 1, 2), precond
    return None


def gmres_dist(name, world, oracle, rel_tol, precond, restart=30, refine=False):
    """(x in the global numbering, info of solve_ref_gmres.gmres) from x0 = 0 on solve_ref_dist.global_system(name) with the right
    preconditioner of `precond` over solve_ref_dist.ranks_of(name, world); computed once"""
    key = (name, world, rel_tol, precond, restart, refine)
    if key not in _YARD:
        s, A, b = solve_ref_dist.global_system(name, oracle)
        rk = (name, world, precond)
        if rk not in _RIGHT:
            _RIGHT[rk] = right_of(solve_ref_dist.ranks_of(name, world, oracle), s.nv, precond)
        _YARD[key] = solve_ref_gmres.gmres(A, b, np.zeros(b.size), rel_tol, max_its=2000, precond=min(precond, 2), nv=s.nv, right=_RIGHT[rk],
                                           restart=restart, refine=refine)
    return _YARD[key]


def operators(Ap, counts, nv, precond):
    """Ap: a global matrix with its nodes in rank order, counts[r] owned nodes of rank r.  -> (op, op_ld): v -> D^-1 Ap (M v) as numpy's
    FP64 applies it and in extended precision, M = the right preconditioner of `precond` (2: none; 5: the ILU(0) of every rank's
    diagonal range; 3: the cycle of the hierarchy whose aggregates stay inside a rank)"""
    Ap = sps.csr_matrix(Ap)
    M = solve_ref.precond_inverse(Ap, nv, 2)[0]
    bptr, bcol, a = solve_ref_mg.block_pattern(Ap, nv)
    rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
    A_ld = ld.Op.of_blocks(bptr, bcol, ld.newton_inverse(ld.diag_of(bptr, bcol, a))[rows] @ a.astype(LD))
    if precond == 5:
        off = np.concatenate([[0], np.cumsum(counts)]) * nv
        sq = [Ap[off[r]:off[r + 1], off[r]:off[r + 1]].tocsr() for r in range(len(counts))]
        f64, fld = [solve_ref_ilu.Factor(q, nv) for q in sq], [solve_ref_ilu.Factor(q, nv, dtype=LD) for q in sq]
        assert all(f.singular == 0 for f in f64 + fld)
        right = lambda v: np.concatenate([f.apply(v[off[r]:off[r + 1]]) for r, f in enumerate(f64)])
        right_ld = lambda v: np.concatenate([f.apply(np.asarray(v, dtype=LD)[off[r]:off[r + 1]]) for r, f in enumerate(fld)])
    elif precond == 3:
        H = solve_ref_mg_dist.EmulatedHierarchy(Ap, nv, counts)
        right, right_ld = H.cycle, ld.Cycle(H, Ap).cycle
    else:
        assert precond == 2, precond
        right = right_ld = None
    op = lambda v: M @ (Ap @ (right(v) if right else v))
    op_ld = lambda v: A_ld @ (right_ld(v) if right_ld else np.asarray(v, dtype=LD))
    return op, op_ld
