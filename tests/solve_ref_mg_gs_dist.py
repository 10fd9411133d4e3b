"""numpy yardstick of the multigrid solve across ranks with the rank-local multicolour Gauss-Seidel smoother
(RDC_PRECOND_MULTIGRID_GS_LOCAL, precond 6; rdc_solve.hip: gs_sweeps_dist): solve_ref_mg_dist.HierarchyDist with the colours of
solve_ref_mg_gs.colour per rank and level, and the cycle of solve_ref_mg_gs.Hierarchy restated on what the ranks hold.

Rule: Gauss-Seidel inside each rank, Jacobi between the ranks.  The first sweep from zero on every level stays x = w D_l^-1 r;
every other sweep is one undamped forward sweep x_n += D_l^-1 (r_n - (A_l x)_n) over the rank's own colour lists, preceded by the
exchange of x on that level: a ghost column reads the value that exchange received and is never written.  The colours of a rank
on a level are the greedy colours of its owned square (columns in the ghost layer ignored); a rank that owns no node of a level
has no colour there.  A sweep costs the one exchange the damped-Jacobi sweep makes for its operator, so the exchange counts are
those of HierarchyDist, count for count.

BiCGStab goes through solve_ref_mg_dist.bicgstab_dist, GMRES through solve_ref_gmres_dist.on_global and solve_ref_gmres.gmres.

EmulatedGs / CycleLocal: the same cycle on ONE global hierarchy whose nodes are ordered rank by rank (solve_ref_mg_dist.
EmulatedHierarchy), in FP64 and, on the operators of solve_ref_mg_ld, in np.longdouble: what ONE application of the device
cycle across ranks is held to."""
import copy

import numpy as np
import scipy.sparse as sps

import solve_ref_dist
import solve_ref_gmres
import solve_ref_gmres_dist
import solve_ref_mg
import solve_ref_mg_dist
import solve_ref_mg_gs
import solve_ref_mg_ld as ld
from solve_ref_mg import COARSEST_SWEEPS, OMEGA

LD = np.longdouble
PRECOND = 6
TOLS = (1e-8, 1e-10)
# (case, world) -> iterations at 1e-8 | 1e-10 from x0 = 0: BiCGStab with the Jacobi smoother, BiCGStab and GMRES(30) with this one
# (None: not run), levels, colours per rank (level 0 first).  tests/test_solve_ref_mg_gs_dist.py pins this table to the code below.
TABLE = {
    ("pihna_kuhn", 1): dict(jacobi=(10, 11), bicgstab=(6, 9), gmres=None, levels=3, colours=[[10, 9, 6]]),
    ("pihna_kuhn", 2): dict(jacobi=(9, 10), bicgstab=(6, 8), gmres=(12, 15), levels=3, colours=[[9, 9, 5], [9, 7, 4]]),
    ("pihna_kuhn", 3): dict(jacobi=(8, 10), bicgstab=(6, 9), gmres=(12, 15), levels=3, colours=[[8, 7, 4], [8, 7, 3], [8, 6, 2]]),
    ("hcc_hex", 2): dict(jacobi=(12, 14), bicgstab=(10, 11), gmres=(16, 20), levels=3, colours=[[13, 8, 4], [12, 7, 3]]),
    ("hcc_hex", 3): dict(jacobi=(13, 16), bicgstab=(9, 12), gmres=None, levels=3, colours=[[12, 7, 3], [11, 7, 2], [11, 7, 1]]),
    ("pihna_kuhn3", 3): dict(jacobi=(5, 6), bicgstab=(4, 5), gmres=(7, 9), levels=2, colours=[[7, 3], [8, 3], [4, 2]]),
}
_H, _YARD = {}, {}


def colour(bptr, bcol):
    """solve_ref_mg_gs.colour of the owned square of one rank's level; no node, no colour"""
    if bptr.size == 1:
        return np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    return solve_ref_mg_gs.colour(np.asarray(bptr, dtype=np.int64), np.asarray(bcol))


def interior_split(nodes, cptr, n_int):
    """how many leading nodes of colour 0 lie below n_int: the part of the level-0 sweep that runs inside the exchange"""
    return int(np.searchsorted(nodes[cptr[0]:cptr[1]], n_int)) if cptr.size > 1 else 0


class HierarchyGsDist(solve_ref_mg_dist.HierarchyDist):
    """HierarchyDist with cols[r][l] = (colour, cptr, nodes) of rank r on level l and the Gauss-Seidel cycle"""

    def __init__(self, ranks, nv, omega=OMEGA, base=None):
        """base: a HierarchyDist of the same ranks, nv and omega, whose levels are then shared, not built again"""
        if base is None:
            super().__init__(ranks, nv, omega)
        else:
            self.__dict__.update(base.__dict__)
            self.exchanges = [0] * self.n_levels
        self.cols, self.sweep = [], []
        for r, rk in enumerate(ranks):
            self.cols.append([])
            self.sweep.append([])
            for l in range(self.n_levels):
                bptr, bcol = self.pattern(r, l)
                col = colour(bptr, bcol)
                A, D = (sps.csr_matrix(rk.A), self.M0[r]) if l == 0 else (self.lv[r][l]["A"], self.lv[r][l]["Dinv"])
                per = []    # per colour: its unknowns, their rows of A_l over owned and ghost columns, the D^-1 blocks that go with them
                for c in range(col[1].size - 1):
                    nodes = col[2][col[1][c]:col[1][c + 1]].astype(np.int64)
                    dofs = (nodes[:, None] * nv + np.arange(nv)[None]).reshape(-1)
                    per.append((dofs, A[dofs], D[dofs][:, dofs]))
                self.cols[r].append(col)
                self.sweep[r].append(per)

    def pattern(self, r, l):
        """(bptr, bcol) of rank r's rows on level l, ghost columns included"""
        if l == 0:
            bptr, bcol, _ = solve_ref_mg.block_pattern(sps.csr_matrix(self.ranks[r].A), self.nv)
            return bptr, bcol
        return self.steps[r][l - 1]["bptr"], self.steps[r][l - 1]["bcol"]

    def colours(self, r):
        """[colours] of rank r per level, level 0 first"""
        return [int(c[1].size - 1) for c in self.cols[r]]

    def _gs(self, l, rs, xs):
        """one sweep on level l: the exchange of x, then every rank's colours in order on its own copy"""
        R = range(len(xs))
        full = [np.concatenate([xs[r], np.zeros(self.lv[r][l]["n_ghost"] * self.nv, dtype=xs[r].dtype)]) for r in R]
        self._exchange(l, full)
        for r in R:
            x = full[r]
            for dofs, rows, dinv in self.sweep[r][l]:
                if l == 0:     # the operator is D^-1 A, the smoother's D is the identity
                    x[dofs] += rs[r][dofs] - dinv @ (rows @ x)
                else:
                    x[dofs] += dinv @ (rs[r][dofs] - rows @ x)
        return [full[r][:xs[r].size] for r in R]

    def cycle(self, rs, l=0):
        R = range(len(rs))
        x = self._smooth(l, rs)
        if l == self.n_levels - 1:
            for _ in range(COARSEST_SWEEPS - 1):
                x = self._gs(l, rs, x)
            return x
        P = [self.lv[r][l]["P"] for r in R]
        ax = self.op(l, x)
        xc = self.cycle([P[r].T @ (rs[r] - ax[r]) for r in R], l + 1)
        return self._gs(l, rs, [x[r] + P[r] @ xc[r] for r in R])


def hierarchy(name, world, oracle):
    """(HierarchyDist, HierarchyGsDist on the same levels) of a case; once per (name, world)"""
    if (name, world) not in _H:
        s = solve_ref_dist.case(name)
        ranks = solve_ref_dist.ranks_of(name, world, oracle)
        base = solve_ref_mg_dist.HierarchyDist(ranks, s.nv)
        _H[(name, world)] = (base, HierarchyGsDist(ranks, s.nv, base=copy.copy(base)))
    return _H[(name, world)]


def bicgstab(name, world, oracle, rel_tol, smoother=1):
    """(xs per rank, info) of solve_ref_mg_dist.bicgstab_dist from x0 = 0 with this smoother (0: damped Jacobi); computed once"""
    key = ("bicgstab", name, world, rel_tol, smoother)
    if key not in _YARD:
        s = solve_ref_dist.case(name)
        ranks = solve_ref_dist.ranks_of(name, world, oracle)
        H = hierarchy(name, world, oracle)[smoother]
        H.exchanges = [0] * H.n_levels
        _YARD[key] = solve_ref_mg_dist.bicgstab_dist(ranks, [np.zeros(rk.A.shape[1]) for rk in ranks], rel_tol, nv=s.nv, hierarchy=H)
    return _YARD[key]


def gmres(name, world, oracle, rel_tol, smoother=1, restart=30):
    """(x in the global numbering, info) of solve_ref_gmres.gmres from x0 = 0 on the global system, the cycle from the right; once"""
    key = ("gmres", name, world, rel_tol, smoother, restart)
    if key not in _YARD:
        s, A, b = solve_ref_dist.global_system(name, oracle)
        ranks = solve_ref_dist.ranks_of(name, world, oracle)
        right = solve_ref_gmres_dist.on_global(hierarchy(name, world, oracle)[smoother].cycle, solve_ref_gmres_dist.rank_dofs(ranks, s.nv))
        _YARD[key] = solve_ref_gmres.gmres(A, b, np.zeros(b.size), rel_tol, max_its=2000, precond=2, nv=s.nv, right=right, restart=restart)
    return _YARD[key]


# ---- the same cycle on one global hierarchy in rank order, in FP64 and in extended precision ----

class EmulatedGs(solve_ref_mg_dist.EmulatedHierarchy):
    """EmulatedHierarchy with every rank's colours of its diagonal range on every level (rank_nodes[l][r] = [global nodes per
    colour]) and the rank-local sweep: the columns outside a rank's range read the x from before the sweep"""

    def __init__(self, A, nv, counts, omega=OMEGA):
        super().__init__(A, nv, counts, omega)
        for l, lv in enumerate(self.levels):
            bptr, bcol = lv["bptr"], lv["bcol"]
            rows = np.repeat(np.arange(lv["n"]), np.diff(bptr))
            lv["rank_nodes"], lv["colour"], o = [], np.zeros(lv["n"], dtype=np.int32), 0
            for c in self.counts[l]:
                keep = (rows >= o) & (rows < o + c)
                sp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep] - o, minlength=c))]).astype(np.int64)
                cols = bcol[keep].astype(np.int64) - o
                cols[(cols < 0) | (cols >= c)] = c     # another rank's node: a ghost column
                col, cptr, nodes = colour(sp, cols)
                lv["colour"][o:o + c] = col
                lv["rank_nodes"].append([o + nodes[cptr[k]:cptr[k + 1]].astype(np.int64) for k in range(cptr.size - 1)])
                o += c
        self.build_sweeps(range(len(self.levels)))

    def build_sweeps(self, which):
        nv = self.nv
        for l in which:
            lv = self.levels[l]
            A, D = (sps.csr_matrix(self.A0), sps.csr_matrix(self.M0)) if l == 0 else (lv["A"], lv["Dinv"])
            lv["sweep"], o = [], 0
            for c, per in zip(self.counts[l], lv["rank_nodes"]):
                inside = np.zeros(A.shape[1])
                inside[o * nv:(o + c) * nv] = 1.0
                own, other = sps.diags(inside), sps.diags(1.0 - inside)
                for nodes in per:
                    dofs = (nodes[:, None] * nv + np.arange(nv)[None]).reshape(-1)
                    lv["sweep"].append((dofs, (A[dofs] @ own).tocsr(), (A[dofs] @ other).tocsr(), D[dofs][:, dofs]))
                o += c

    def mixed(self, A32):
        """this hierarchy with the level-0 operator inside the cycle replaced by A32 = fl32(D^-1 A); the coarse levels are shared"""
        G = copy.copy(self)
        G.A0, G.M0 = sps.csr_matrix(A32), sps.identity(A32.shape[0], format="csr")
        G.levels = [dict(self.levels[0])] + self.levels[1:]
        G.build_sweeps([0])
        return G

    def _gs(self, l, r, x):
        old = x.copy()
        for dofs, own, other, dinv in self.levels[l]["sweep"]:
            ax = own @ x + other @ old
            if l == 0:
                x[dofs] += r[dofs] - dinv @ ax
            else:
                x[dofs] += dinv @ (r[dofs] - ax)
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


def _split_columns(op, lo, hi):
    """the entries of an ld.Op whose column lies in [lo, hi), and the others: two Ops over the same rows and columns"""
    inside = (op.indices >= lo) & (op.indices < hi)
    rows = np.repeat(np.arange(op.indptr.size - 1), np.diff(op.indptr))
    part = lambda k: ld.Op(np.concatenate([[0], np.cumsum(np.bincount(rows[k], minlength=op.indptr.size - 1))]), op.indices[k], op.data[k], op.n_cols)
    return part(inside), part(~inside)


class CycleLocal(ld.Cycle):
    """ld.Cycle of an EmulatedGs hierarchy H on the matrix A it was built from, with the rank-local sweep: every value in extended
    precision, nothing taken from H but its index lists and its damping.  op0: the level-0 operator of the mixed form."""

    def __init__(self, H, A, op0=None):
        super().__init__(H, A, op0)
        nv = self.nv
        for mine, lv, counts in zip(self.levels, H.levels, H.counts):
            mine["sweep"], o = [], 0
            for c, per in zip(counts, lv["rank_nodes"]):
                for nodes in per:
                    dofs = (nodes[:, None] * nv + np.arange(nv)[None]).reshape(-1)
                    mine["sweep"].append((nodes, dofs) + _split_columns(mine["op"].rows(dofs), o * nv, (o + c) * nv))
                o += c

    def _sweep(self, l, r, x):
        lv, old = self.levels[l], x.copy()
        for nodes, dofs, own, other in lv["sweep"]:
            res = r[dofs] - (own @ x + other @ old)
            x[dofs] += res if l == 0 else (lv["dinv"][nodes] @ res.reshape(-1, self.nv, 1)).reshape(-1)
        return x
