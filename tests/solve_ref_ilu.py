"""numpy restatement of the multicolour block ILU(0) preconditioner of rdc_solve (RDC_PRECOND_ILU0 = 4; rdc_solve.h:
ilu_build, ilu_factor_node; rdc_solve.hip: k_ilu_factor, k_ilu_fwd, k_ilu_bwd): the yardstick for the factor, for one apply
and for the iteration counts.

The system is that of block Jacobi, A^ = D^-1 A, and M = (LU)^-1 is applied from the right.  LU is the block ILU(0) of A^ on the
node-block pattern: nodes are eliminated by (colour, node id), the colours being the greedy ones of solve_ref_mg_gs.colour
(order="natural": by node id alone, for comparison).  L has identity diagonal blocks, which are not stored; U carries the
diagonal blocks, so the backward sweep divides by a BLOCK: z_i = U_ii^-1 (z_i - sum U_ij z_j) -- a scalar triangular solve with
U would be another preconditioner.

The factor of node i: for its row neighbours k that are eliminated earlier, in elimination order, L_ik = F_ik U_kk^-1, then
F_ij -= L_ik F_kj for every block j of row k that is eliminated later than k and is also in row i.

dtype: np.float64, or np.longdouble -- the reference the device factor and apply are held to (its D^-1 and U_ii^-1 come from
solve_ref_mg_ld.newton_inverse).  The blocks are kept in the order of the CSR pattern (bcol ascending per node): values() is
the factor in the layout of the CSR values, what rdc_solve_ilu_download returns."""
import numpy as np
import scipy.sparse as sps

import solve_ref
import solve_ref_mg
import solve_ref_mg_gs
import solve_ref_mg_ld as ld
from solve_ref import CONVERGED, MAX_ITS  # noqa: F401 (the tests name the outcome through this module)

LD = np.longdouble


def _inverse(D, dtype):
    return ld.newton_inverse(D) if dtype == LD else np.linalg.inv(D)


def csr_layout(bptr, blocks):
    """blocks [nblk][nv][nv] (bcol order) in the layout of the CSR values: per node [var a][block k][var b]"""
    nv = blocks.shape[1]
    out = np.empty(blocks.size, dtype=blocks.dtype)
    for i in range(bptr.size - 1):
        b0, b1 = bptr[i], bptr[i + 1]
        out[nv * nv * b0:nv * nv * b1] = blocks[b0:b1].transpose(1, 0, 2).reshape(-1)
    return out


def scaled_values(A, nv, dtype=np.float64):
    """A^ = D^-1 A in the layout of the CSR values: what the factorisation starts from"""
    bptr, bcol, blocks = solve_ref_mg.block_pattern(A, nv)
    rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
    return csr_layout(bptr, _inverse(blocks[bcol == rows], dtype)[rows] @ blocks.astype(dtype))


class Factor:
    def __init__(self, A, nv, order="colour", dtype=np.float64):
        self.nv, self.dtype = nv, dtype
        bptr, bcol, blocks = solve_ref_mg.block_pattern(A, nv)
        self.bptr, self.bcol = bptr, bcol
        n = self.n = bptr.size - 1
        rows = np.repeat(np.arange(n), np.diff(bptr))
        on = bcol == rows
        assert np.count_nonzero(on) == n, "a node has no diagonal block"
        self.diag = np.flatnonzero(on)
        if order == "colour":
            self.colour, self.cptr, _ = solve_ref_mg_gs.colour(bptr, bcol)
            assert solve_ref_mg_gs.is_proper(bptr, bcol, self.colour)
        else:
            assert order == "natural"
            self.colour, self.cptr = np.zeros(n, dtype=np.int32), None
        self.order = np.lexsort((np.arange(n), self.colour))          # elimination order: (colour, node id)
        rank = self.rank = np.empty(n, dtype=np.int64)
        rank[self.order] = np.arange(n)
        # A^ = D^-1 A in the working precision
        F = self.F = _inverse(blocks[self.diag], dtype)[rows] @ blocks.astype(dtype)
        self.Uinv = np.zeros((n, nv, nv), dtype=dtype)
        self.lower, self.upper = [None] * n, [None] * n                # block indices of a node, each in elimination order
        for i in range(n):
            ks = np.arange(bptr[i], bptr[i + 1])
            ks = ks[np.argsort(rank[bcol[ks]], kind="stable")]
            r = rank[bcol[ks]]
            self.lower[i], self.upper[i] = ks[r < rank[i]], ks[r > rank[i]]
        self.singular = 0
        for i in self.order:
            b0, row = bptr[i], bcol[bptr[i]:bptr[i + 1]]
            for kb in self.lower[i]:
                k = bcol[kb]
                L = F[kb] = F[kb] @ self.Uinv[k]
                up = self.upper[k]
                at = np.searchsorted(row, bcol[up])
                hit = row[np.minimum(at, row.size - 1)] == bcol[up]
                F[b0 + at[hit]] -= L @ F[up[hit]]
            U = F[self.diag[i]]
            try:                                   # an exactly zero pivot (LinAlgError) or a non-finite entry: a bad block
                with np.errstate(all="ignore"):
                    Ui = _inverse(U[None], dtype)[0]
                bad = not np.all(np.isfinite(Ui.astype(np.float64)))
            except np.linalg.LinAlgError:
                bad = True
            self.singular += bad
            self.Uinv[i] = np.eye(nv) if bad else Ui
        self._sweeps = None

    def values(self):
        """the factor in the layout of the CSR values: per node [var a][block k][var b]; L and U blocks where the blocks they replace
        were, the diagonal blocks of U included"""
        return csr_layout(self.bptr, self.F)

    def apply(self, y):
        """z = (LU)^-1 y, node after node in the working precision: forward with L (identity diagonal), backward with U by blocks"""
        nv = self.nv
        z = np.array(y, dtype=self.dtype).reshape(self.n, nv)
        if self.dtype == np.float64 and self.cptr is not None:
            return self._apply_by_colour(z.reshape(-1))
        for i in self.order:
            lo = self.lower[i]
            if lo.size:
                z[i] -= np.einsum("kab,kb->a", self.F[lo], z[self.bcol[lo]])
        for i in self.order[::-1]:
            up = self.upper[i]
            t = z[i] - np.einsum("kab,kb->a", self.F[up], z[self.bcol[up]]) if up.size else z[i]
            z[i] = self.Uinv[i] @ t
        return z.reshape(-1)

    def _apply_by_colour(self, z):
        """the same in FP64, colour after colour as the device runs it (the nodes of a colour are independent): sparse rows of L and
        of the strict upper part of U per colour, U_ii^-1 as a block-diagonal matrix"""
        if self._sweeps is None:
            nv, n = self.nv, self.n
            strict_l = np.concatenate(self.lower)
            strict_u = np.concatenate(self.upper)
            rows = np.repeat(np.arange(n), np.diff(self.bptr))

            def part(idx):   # the blocks idx of the factor as a scalar CSR matrix (ascending block index = row-major)
                idx = np.sort(idx)
                indptr = np.concatenate([[0], np.cumsum(np.bincount(rows[idx], minlength=n))])
                return sps.bsr_matrix((self.F[idx], self.bcol[idx], indptr), shape=(n * nv, n * nv)).tocsr()
            Lm, Um = part(strict_l), part(strict_u)
            Ui = sps.bsr_matrix((self.Uinv, np.arange(n), np.arange(n + 1)), shape=(n * nv, n * nv)).tocsr()
            self._sweeps = []
            nodes = self.order
            for c in range(self.cptr.size - 1):
                mine = nodes[self.cptr[c]:self.cptr[c + 1]].astype(np.int64)
                dofs = (mine[:, None] * nv + np.arange(nv)[None]).reshape(-1)
                self._sweeps.append((dofs, Lm[dofs], Um[dofs], Ui[dofs][:, dofs]))
        z = z.copy()
        for dofs, Lr, _, _ in self._sweeps[1:]:
            z[dofs] -= Lr @ z
        for dofs, _, Ur, Ui in self._sweeps[::-1]:
            z[dofs] = Ui @ (z[dofs] - Ur @ z)
        return z


def bicgstab(A, b, x0, rel_tol, abs_tol=0.0, max_its=10000, nv=1, order="colour", factor=None):
    """solve_ref.bicgstab on block Jacobi's system with the ILU(0) sweeps from the right -> (x, info); info also has colours"""
    f = factor or Factor(A, nv, order)
    x, info = solve_ref.bicgstab(A, b, x0, rel_tol, abs_tol, max_its, 2, nv, right=f.apply)
    info.update(colours=int(f.colour.max()) + 1)
    return x, info
