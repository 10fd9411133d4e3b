"""numpy / scipy restatement of the multigrid cycle of rdc_solve with the multicolour Gauss-Seidel smoother (option "mg_smoother" = 1;
rdc_solve.h: mg_colour, rdc_solve.hip: k_gs, gs_sweeps): the yardstick for its iteration counts and its colours, on the hierarchy of
solve_ref_mg.py unchanged.

Colours (per level, on the node-block graph): greedy, nodes in ascending order, each takes the smallest colour that no row neighbour
with a colour already holds; no cap on their number.

Cycle: the first sweep from zero on every level stays x = w D_l^-1 r (w = 0.6); every other sweep -- the post-smoothing of every
level and the COARSEST_SWEEPS - 1 further sweeps of the last -- is one forward Gauss-Seidel sweep, colour after colour:
x_n += D_l^-1 (r_n - (A_l x)_n) for the nodes n of the colour, from the x the colours before it left.  D_0 = I.  Written as loops
over the colours, as the device runs them; the two differ in the order of the sums of a row only."""
import numpy as np

import solve_ref
import solve_ref_mg
from solve_ref import CONVERGED  # noqa: F401 (the tests name the outcome through this module)
from solve_ref_mg import COARSEST_SWEEPS, OMEGA


def colour(bptr, bcol):
    """-> (colour int32 [n], cptr int64 [colours + 1], nodes int32 [n]): nodes[cptr[c]:cptr[c + 1]] are those of colour c, ascending"""
    n = bptr.size - 1
    col = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        nb = bcol[bptr[i]:bptr[i + 1]]
        held = set(col[nb[(nb != i) & (nb < n)]].tolist())
        c = 0
        while c in held:
            c += 1
        col[i] = c
    cptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=1))]).astype(np.int64)
    return col, cptr, np.argsort(col, kind="stable").astype(np.int32)


def is_proper(bptr, bcol, col):
    """no block (i, j), i != j, joins two nodes of one colour"""
    rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
    off = (rows != bcol) & (bcol < col.size)
    return not np.any(col[rows[off]] == col[bcol[off]])


class Hierarchy(solve_ref_mg.Hierarchy):
    """solve_ref_mg.Hierarchy with the colour lists of every level (colour, cptr, cnodes) and the Gauss-Seidel cycle"""

    def __init__(self, A, nv, omega=OMEGA, base=None):
        """base: a solve_ref_mg.Hierarchy of the same A, nv and omega, whose levels are then shared, not built again"""
        if base is None:
            super().__init__(A, nv, omega)
        else:
            self.__dict__.update(base.__dict__)
        self.colour()

    def colour(self):
        nv = self.nv
        for l, lv in enumerate(self.levels):
            lv["colour"], lv["cptr"], lv["cnodes"] = colour(lv["bptr"], lv["bcol"])
            A, D = (self.A0, self.M0) if l == 0 else (lv["A"], lv["Dinv"])
            lv["sweep"] = []   # per colour: its unknowns, their rows of A_l, and the D^-1 blocks that go with them
            for c in range(lv["cptr"].size - 1):
                nodes = lv["cnodes"][lv["cptr"][c]:lv["cptr"][c + 1]].astype(np.int64)
                dofs = (nodes[:, None] * nv + np.arange(nv)[None]).reshape(-1)
                lv["sweep"].append((dofs, A[dofs], D[dofs][:, dofs]))

    def colours(self):
        """[colours] per level, level 0 first"""
        return [int(lv["cptr"].size - 1) for lv in self.levels]

    def _gs(self, l, r, x):
        """one forward sweep on level l, in place"""
        for dofs, rows, dinv in self.levels[l]["sweep"]:
            if l == 0:     # the operator is D^-1 A, the smoother's D is the identity
                x[dofs] += r[dofs] - dinv @ (rows @ x)
            else:
                x[dofs] += dinv @ (r[dofs] - rows @ x)
        return x

    def cycle(self, r, l=0):
        x = self._smooth(l, r)
        if l == len(self.levels) - 1:
            for _ in range(COARSEST_SWEEPS - 1):
                x = self._gs(l, r, x)
            return x
        P = self.levels[l]["P"]
        x = x + P @ self.cycle(P.T @ (r - self._op(l, x)), l + 1)
        return self._gs(l, r, x)


def bicgstab(A, b, x0, rel_tol, abs_tol=0.0, max_its=10000, nv=1, omega=OMEGA, hierarchy=None):
    """solve_ref_mg.bicgstab with the Gauss-Seidel cycle -> (x, info); info also has levels, complexity, colours"""
    H = hierarchy or Hierarchy(A, nv, omega)
    x, info = solve_ref.bicgstab(A, b, x0, rel_tol, abs_tol, max_its, 2, nv, right=H.cycle)
    info.update(levels=H.level_sizes(), complexity=H.operator_complexity(), colours=H.colours())
    return x, info
