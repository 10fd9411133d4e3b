"""Extended-precision (np.longdouble, 64-bit mantissa) evaluation of the multigrid cycle of solve_ref_mg.Hierarchy and
solve_ref_mg_gs.Hierarchy: the reference that ONE application of the device cycle (rdc_solve_mg_apply) and the coarse matrices
(rdc_solve_mg_level_download) are held to, where the iteration counts of a converged solve have no room to show a fault
(tests/test_solve_ref_mg_ld.py has the record; tests/test_gpu_mg_cycle.py the device side).

Nothing here is taken from the numpy hierarchy but its index lists (aggregates, patterns, Galerkin lists, colours) and its damping:
every value is formed again from A in extended precision -- D^-1 by Newton refinement of np.linalg.inv, D^-1 A, the Galerkin sums,
every D_l^-1 -- so that the difference between the numpy cycle and this one measures the rounding of an FP64 evaluation of the
cycle (`noise`), the yardstick for what the device may differ by.  Matrix products are scalar-CSR products with np.add.reduceat,
restriction is np.add.at, prolongation an index.

Mixed form (rdc_solve_mixed): the level-0 operator inside the cycle is fl32(D^-1 A), passed in as a matrix (`op0`); the coarse
levels stay the Galerkin products of the unrounded D^-1 A, as on the device."""
import copy

import numpy as np
import scipy.sparse as sps

import solve_ref
import solve_ref_mg
from solve_ref_mg import COARSEST_SWEEPS

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
EPS_LD = float(np.finfo(LD).eps)

# What the device cycle may differ from the extended-precision one by: MARGIN x max(noise, 16 eps), noise = what the numpy FP64
# cycle differs by on the same system and inputs (mixed: also what one-ulp differences of the fp32 copy do, noise32).  The
# margins are the next power of two at or above 8 x the largest error / noise ratio measured on an MI355X (DESIGN.md 7.2 has the
# table, tests/test_gpu_mg_cycle.py repeats it); MARGIN_INV is the same for the D_l^-1 of a level against np.linalg.inv of the same block.  BOUND_CAP is a condition, not
# a measurement: a case whose bound exceeds it is ill-conditioned in a way the reference is not, and fails.
MARGIN, MARGIN_MIXED, MARGIN_INV = 128.0, 64.0, 1024.0   # largest ratios measured: 13.71, 5.65, 67.98
MARGIN_INV_CAP = 1024.0
BOUND_CAP = 1e-6


def bound(margin, *noises):
    return margin * max(max(noises), 16.0 * EPS)


def newton_inverse(D, steps=6):
    """[n][nv][nv] inverses in extended precision: X <- X + X (I - D X) from X = np.linalg.inv(D), which converges quadratically
    from any start with ||I - D X|| < 1 (cond(D) * 2^-53 < 1)"""
    D = np.asarray(D, dtype=LD)
    X = np.linalg.inv(D.astype(np.float64)).astype(LD)
    eye = np.eye(D.shape[-1], dtype=LD)
    for _ in range(steps):
        X = X + X @ (eye - D @ X)
    return X


class Op:
    """scalar CSR matrix with extended-precision values"""

    def __init__(self, indptr, indices, data, n_cols):
        self.indptr, self.indices, self.data, self.n_cols = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(data, dtype=LD), n_cols
        self._index = None

    @classmethod
    def of_matrix(cls, A):
        A = sps.csr_matrix(A)
        return cls(A.indptr, A.indices, A.data, A.shape[1])

    @classmethod
    def of_blocks(cls, bptr, bcol, blocks):
        """node-block pattern with [nblk][nv][nv] values: dof = node * nv + var"""
        nv, n = blocks.shape[1], bptr.size - 1
        where = sps.bsr_matrix((np.arange(1, blocks.size + 1, dtype=np.float64).reshape(blocks.shape), bcol, bptr), shape=(n * nv, n * nv)).tocsr()
        return cls(where.indptr, where.indices, np.asarray(blocks, dtype=LD).reshape(-1)[where.data.astype(np.int64) - 1], n * nv)

    def __matmul__(self, x):
        prod = self.data * np.asarray(x, dtype=LD)[self.indices]
        y = np.zeros(self.indptr.size - 1, dtype=LD)
        full = np.diff(self.indptr) > 0
        y[full] = np.add.reduceat(prod, self.indptr[:-1][full])   # the starts of the rows that have entries ascend strictly
        return y

    def rows(self, dofs):
        """the rows `dofs`, as an Op over the same columns"""
        if self._index is None:
            self._index = sps.csr_matrix((np.arange(1, self.data.size + 1, dtype=np.float64), self.indices, self.indptr), shape=(self.indptr.size - 1, self.n_cols))
        sub = self._index[dofs]
        return Op(sub.indptr, sub.indices, self.data[sub.data.astype(np.int64) - 1], self.n_cols)


def galerkin(blocks, cptr, cidx):
    """extended-precision sum of the summands blocks[cidx[cptr[c]:cptr[c + 1]]] per coarse block c (no list is empty)"""
    assert np.diff(cptr).min() >= 1
    return np.add.reduceat(np.asarray(blocks, dtype=LD)[cidx], cptr[:-1], axis=0)


def galerkin_lists(H, l):
    """(cptr, cidx) of the Galerkin sum that builds level l >= 1 of the numpy hierarchy H from level l - 1, from the patterns and
    aggregates (a Gauss-Seidel hierarchy keeps its colour lists under the key the Jacobi hierarchy keeps these under)"""
    fine = H.levels[l - 1]
    cb, cc, cptr, cidx = solve_ref_mg.coarse_pattern(fine["bptr"], fine["bcol"], fine["agg"], H.levels[l]["n"])
    assert np.array_equal(cb, H.levels[l]["bptr"]) and np.array_equal(cc, H.levels[l]["bcol"])
    return cptr, cidx


def diag_of(bptr, bcol, blocks):
    """the diagonal blocks [n][nv][nv] of a node-block matrix (every node has one)"""
    rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
    on = bcol == rows
    assert np.count_nonzero(on) == bptr.size - 1
    return blocks[on]


def scaled_f32_ld(A, nv):
    """fl32(D^-1 A) as solve_ref_mixed.scaled_f32 gives it, but rounded from the extended-precision D^-1 A: the same pattern"""
    bptr, bcol, blocks = solve_ref_mg.block_pattern(A, nv)
    rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
    S = newton_inverse(solve_ref.diag_blocks(A, nv))[rows] @ blocks.astype(LD)
    with np.errstate(over="ignore"):
        S32 = S.astype(np.float32).astype(np.float64)
    N = (bptr.size - 1) * nv
    return sps.bsr_matrix((S32, bcol, bptr), shape=(N, N)).tocsr()


def mixed_hierarchy(H, A32):
    """the numpy hierarchy H with the level-0 operator INSIDE the cycle replaced by A32 = fl32(D^-1 A) (a float64 matrix); the
    coarse levels are shared.  What rdc_solve_mixed applies."""
    G = copy.copy(H)
    G.A0, G.M0 = sps.csr_matrix(A32), sps.identity(A32.shape[0], format="csr")
    if hasattr(H, "_gs"):
        G.levels = [dict(H.levels[0])] + H.levels[1:]
        G.levels[0]["sweep"] = [(dofs, G.A0[dofs], G.M0[dofs][:, dofs]) for dofs, _, _ in H.levels[0]["sweep"]]
    return G


class Cycle:
    """the cycle of the numpy hierarchy H (solve_ref_mg.Hierarchy: damped Jacobi; solve_ref_mg_gs.Hierarchy: Gauss-Seidel) on the
    matrix A it was built from, every value in extended precision.  op0: the level-0 operator of the mixed form."""

    def __init__(self, H, A, op0=None):
        nv = self.nv = H.nv
        self.omega = LD(H.omega)
        self.gs = hasattr(H, "_gs")   # (the level dicts of a Jacobi hierarchy may be shared with a Gauss-Seidel one: no test on their keys)
        self.levels = []
        blocks = None
        for l, lv in enumerate(H.levels):
            bptr, bcol = lv["bptr"], lv["bcol"]
            if l == 0:
                _, _, a = solve_ref_mg.block_pattern(A, nv)
                rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
                blocks = newton_inverse(diag_of(bptr, bcol, a))[rows] @ a.astype(LD)
                mine = dict(op=Op.of_matrix(op0) if op0 is not None else Op.of_blocks(bptr, bcol, blocks), dinv=None)
            else:
                blocks = galerkin(blocks, *galerkin_lists(H, l))
                mine = dict(op=Op.of_blocks(bptr, bcol, blocks), dinv=newton_inverse(diag_of(bptr, bcol, blocks)))
            mine.update(n=lv["n"], blocks=blocks, agg=lv.get("agg"))
            if self.gs:
                mine["sweep"] = []
                for c in range(lv["colour"].max() + 1):
                    nodes = np.flatnonzero(lv["colour"] == c)   # ascending, as the colour lists are
                    dofs = (nodes[:, None] * nv + np.arange(nv)[None]).reshape(-1)
                    mine["sweep"].append((nodes, dofs, mine["op"].rows(dofs)))
            self.levels.append(mine)

    def _smooth(self, l, r):
        if l == 0:
            return self.omega * r
        return self.omega * (self.levels[l]["dinv"] @ r.reshape(-1, self.nv, 1)).reshape(-1)

    def _sweep(self, l, r, x):
        lv = self.levels[l]
        if not self.gs:
            return x + self._smooth(l, r - lv["op"] @ x)
        for nodes, dofs, rows in lv["sweep"]:
            res = r[dofs] - rows @ x
            x[dofs] += res if l == 0 else (lv["dinv"][nodes] @ res.reshape(-1, self.nv, 1)).reshape(-1)
        return x

    def cycle(self, r, l=0):
        r = np.asarray(r, dtype=LD)
        lv = self.levels[l]
        x = self._smooth(l, r)
        if l == len(self.levels) - 1:
            for _ in range(COARSEST_SWEEPS - 1):
                x = self._sweep(l, r, x)
            return x
        rc = np.zeros((self.levels[l + 1]["n"], self.nv), dtype=LD)
        np.add.at(rc, lv["agg"], (r - lv["op"] @ x).reshape(-1, self.nv))
        x = x + self.cycle(rc.reshape(-1), l + 1).reshape(-1, self.nv)[lv["agg"]].reshape(-1)
        return self._sweep(l, r, x)


def rel_diff(z, z_ld):
    """(2-norm, max-norm) of z - z_ld relative to z_ld, formed in extended precision"""
    d = np.asarray(z, dtype=LD) - z_ld
    return float(np.sqrt(d @ d) / np.sqrt(z_ld @ z_ld)), float(np.abs(d).max() / np.abs(z_ld).max())


def probe_vectors(n, b):
    """the inputs the cycle is compared on: two Gaussian vectors (fixed seeds) and the scaled rhs b"""
    return [np.random.default_rng(seed).standard_normal(n) for seed in (11, 12)] + [np.asarray(b, dtype=np.float64)]


def noise(H, C, inputs):
    """largest relative 2-norm and max-norm difference between the numpy cycle H and the extended-precision cycle C over `inputs`"""
    d = [rel_diff(H.cycle(v), C.cycle(v)) for v in inputs]
    return max(a for a, _ in d), max(b for _, b in d)
