"""numpy / scipy restatement of the aggregation-multigrid preconditioner of rdc_solve (precond = 3; rdc_solve.h, rdc_solve.hip):
the yardstick for its iteration counts and its hierarchy, as solve_ref.py is for the Jacobi-class preconditioners.

System: A^ = D^-1 A, b^ = D^-1 b, D the node-block diagonal (what precond = 2 iterates on).  The cycle M ~ A^^-1 is applied from
the RIGHT (p^ = M p, v = A^ p^; s^ = M s, t = A^ s^; x += alpha p^ + omega s^), so the recurrence residual stays D^-1 (b - A x)
and the stopping test, the confirmation / restart and solve_ref.check_solution(..., precond=2, ...) mean what they mean there.

Aggregation (per level, on the node-block graph bptr / bcol, ascending node order, deterministic):
  pass 1  a free node with at least MIN_FREE free neighbours becomes a root and takes the first AGG_CAP - 1 of them (ascending);
  pass 2  a node still free joins the aggregate of its first neighbour (ascending) that has one by then -- joined in pass 2
          included --, or becomes a singleton.
Levels are added until one has at most COARSEST_NODES nodes, MAX_LEVELS exist, or a coarsening merges nothing.
P is piecewise constant per unknown; level l + 1 = P^T A_l P with A_0 = A^: coarse block (I, J) is the sum of the fine blocks
(n, m), agg[n] = I, agg[m] = J, in ascending (n, k) order.  The level-0 summand D^-1_n A_nm is formed as scaled_block does.

Cycle: V(1,1), damped block Jacobi (omega = 0.6): x = w D_l^-1 r; r_c = P^T (r - A_l x); x += P cycle(r_c); x += w D_l^-1 (r - A_l x);
COARSEST_SWEEPS sweeps of the same smoother on the last level.  D_0 = I: the diagonal blocks of A^ are the identity."""
import numpy as np
import scipy.sparse as sps

import solve_ref
from solve_ref import CONVERGED  # noqa: F401 (the tests name the outcome through this module)

AGG_CAP, MIN_FREE, COARSEST_NODES, MAX_LEVELS, COARSEST_SWEEPS, OMEGA = 8, 3, 40, 10, 8, 0.6


def block_pattern(A, nv):
    """(bptr int64, bcol int32, blocks [nblk][nv][nv]) of a scalar CSR matrix with dof = node * nv + var; bcol ascends per node"""
    B = sps.bsr_matrix(A, blocksize=(nv, nv))
    B.sort_indices()
    return B.indptr.astype(np.int64), B.indices.astype(np.int32), np.array(B.data, dtype=np.float64)


def aggregate(bptr, bcol):
    """-> (agg int32 [n], number of aggregates, number of aggregates built in pass 1, their sizes at the end of pass 1)"""
    n = bptr.size - 1
    agg = np.full(n, -1, dtype=np.int32)
    na = 0
    for i in range(n):
        if agg[i] >= 0:
            continue
        nb = [j for j in bcol[bptr[i]:bptr[i + 1]] if j != i and agg[j] < 0]
        if len(nb) >= MIN_FREE:
            agg[i] = na
            agg[nb[:AGG_CAP - 1]] = na
            na += 1
    n_pass1, sizes1 = na, np.bincount(agg[agg >= 0], minlength=na)
    for i in range(n):
        if agg[i] >= 0:
            continue
        for j in bcol[bptr[i]:bptr[i + 1]]:
            if j != i and agg[j] >= 0:
                agg[i] = agg[j]
                break
        else:
            agg[i] = na
            na += 1
    return agg, na, n_pass1, sizes1


def coarse_pattern(bptr, bcol, agg, na):
    """-> (coarse bptr, coarse bcol, cptr, cidx): the fine blocks cidx[cptr[c]:cptr[c + 1]] (ascending) sum into coarse block c"""
    rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
    key = agg[rows].astype(np.int64) * na + agg[bcol]
    uniq, inv = np.unique(key, return_inverse=True)
    cb = np.zeros(na + 1, dtype=np.int64)
    np.add.at(cb, uniq // na + 1, 1)
    cptr = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=uniq.size))]).astype(np.int64)
    return np.cumsum(cb), (uniq % na).astype(np.int32), cptr, np.argsort(inv, kind="stable").astype(np.int32)


def pattern_hierarchy(bptr, bcol):
    """the coarsening steps below a pattern: [dict(agg, n, n_pass1, pass1_sizes, bptr, bcol, cptr, cidx)], step l takes level l to l + 1"""
    steps, n = [], bptr.size - 1
    while n > COARSEST_NODES and len(steps) + 1 < MAX_LEVELS:
        agg, na, n1, sizes1 = aggregate(bptr, bcol)
        if na >= n:
            break
        cb, cc, cptr, cidx = coarse_pattern(bptr, bcol, agg, na)
        steps.append(dict(agg=agg, n=na, n_pass1=n1, pass1_sizes=sizes1, bptr=cb, bcol=cc, cptr=cptr, cidx=cidx))
        n, bptr, bcol = na, cb, cc
    return steps


def scaled_blocks(dinv, blocks):
    """dinv[i] @ blocks[i] with every sum in ascending index order from 0.0, separate multiply and add"""
    out = np.zeros_like(blocks)
    for q in range(blocks.shape[1]):
        out = out + dinv[:, :, q, None] * blocks[:, q, None, :]
    return out


def galerkin(blocks, cptr, cidx):
    """coarse blocks: the fine ones summed in list order, from 0.0"""
    out = np.zeros((cptr.size - 1,) + blocks.shape[1:])
    np.add.at(out, np.repeat(np.arange(cptr.size - 1), np.diff(cptr)), blocks[cidx])
    return out


class Hierarchy:
    """levels[l] = dict(n, bptr, bcol, blocks, A (scipy CSR), Dinv (scipy CSR), agg (to level l + 1, absent on the last))"""

    def __init__(self, A, nv, omega=OMEGA):
        self.nv, self.omega = nv, omega
        bptr, bcol, blocks = block_pattern(A, nv)
        n = bptr.size - 1
        rows = np.repeat(np.arange(n), np.diff(bptr))
        _, Di, _ = solve_ref.precond_inverse(A, nv, 2)
        lv = dict(n=n, bptr=bptr, bcol=bcol, blocks=scaled_blocks(Di[rows], blocks))
        self.M0 = solve_ref.precond_inverse(A, nv, 2)[0]
        self.A0 = A
        self.levels = [lv]
        for st in pattern_hierarchy(bptr, bcol):
            agg, na, cb, cc, cptr, cidx = st["agg"], st["n"], st["bptr"], st["bcol"], st["cptr"], st["cidx"]
            lv["agg"] = agg
            lv["P"] = sps.kron(sps.csr_matrix((np.ones(agg.size), agg, np.arange(agg.size + 1)), shape=(agg.size, na)), sps.eye(nv)).tocsr()
            lv = dict(n=na, bptr=cb, bcol=cc, blocks=galerkin(lv["blocks"], cptr, cidx), cptr=cptr, cidx=cidx)
            self.levels.append(lv)
        for l, lv in enumerate(self.levels):
            if l == 0:
                continue
            N = lv["n"] * nv
            lv["A"] = sps.bsr_matrix((lv["blocks"], lv["bcol"], lv["bptr"]), shape=(N, N)).tocsr()
            lv["Dinv"] = solve_ref.precond_inverse(lv["A"], nv, 2)[0]

    def level_sizes(self):
        """[(nodes, blocks)] per level, level 0 first"""
        return [(int(lv["n"]), int(lv["bcol"].size)) for lv in self.levels]

    def operator_complexity(self):
        s = self.level_sizes()
        return sum(b for _, b in s) / s[0][1]

    def _op(self, l, x):
        return self.M0 @ (self.A0 @ x) if l == 0 else self.levels[l]["A"] @ x

    def _smooth(self, l, r):
        return self.omega * r if l == 0 else self.omega * (self.levels[l]["Dinv"] @ r)

    def cycle(self, r, l=0):
        x = self._smooth(l, r)
        if l == len(self.levels) - 1:
            for _ in range(COARSEST_SWEEPS - 1):
                x = x + self._smooth(l, r - self._op(l, x))
            return x
        P = self.levels[l]["P"]
        x = x + P @ self.cycle(P.T @ (r - self._op(l, x)), l + 1)
        return x + self._smooth(l, r - self._op(l, x))


def bicgstab(A, b, x0, rel_tol, abs_tol=0.0, max_its=10000, nv=1, omega=OMEGA, hierarchy=None):
    """solve_ref.bicgstab(precond=2) with the cycle as its `right` hook -> (x, info); info also has levels, complexity"""
    H = hierarchy or Hierarchy(A, nv, omega)
    x, info = solve_ref.bicgstab(A, b, x0, rel_tol, abs_tol, max_its, 2, nv, right=H.cycle)
    info.update(levels=H.level_sizes(), complexity=H.operator_complexity())
    return x, info
