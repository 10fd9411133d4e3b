"""numpy yardstick of the block ILU(0) with an fp32 copy of the factor (option "ilu_factor_bits" = 32; rdc_solve.hip:
k_ilu_round_f32, k_ilu_fwd_f32, k_ilu_bwd_f32): built on tests/solve_ref_ilu.py, which stays as it is.

The factorisation is the FP64 one.  Its lower and upper blocks are then rounded to fp32 (astype(np.float32): round to nearest
even, what the device's conversion does) and the sweeps run on the rounded blocks with everything else -- z, the sums, U_ii^-1 --
in the working precision: np.float64, or np.longdouble, the reference one device apply is held to.  The diagonal blocks of U are
not rounded: the sweeps never read them, they read U_ii^-1.

rounded(f) takes a solve_ref_ilu.Factor; with val / uinv it takes a DOWNLOADED factor instead (rdc_solve_ilu_download, or
rdc_solve_ilu_local_download with f built on the owned square: both are the layout of f's pattern) and f only lends its lists.  A
test of the device rounds the device's own FP64 factor: a last-bit difference between two FP64 factors can flip an fp32 rounding,
6e-8 on an entry, which has nothing to do with the sweeps under test."""
import numpy as np

import solve_ref
import solve_ref_dist
import solve_ref_ilu
import solve_ref_ilu_dist
import solve_ref_mixed
from solve_ref import CONVERGED, MAX_ITS  # noqa: F401

LD = np.longdouble
_YARD = {}


def blocks_of(bptr, val, nv):
    """the inverse of solve_ref_ilu.csr_layout: values per node [var a][block k][var b] -> blocks [nblk][nv][nv] in bcol order"""
    val = np.asarray(val)
    out = np.empty((int(bptr[-1]), nv, nv), dtype=val.dtype)
    for i in range(bptr.size - 1):
        b0, b1 = bptr[i], bptr[i + 1]
        out[b0:b1] = val[nv * nv * b0:nv * nv * b1].reshape(nv, b1 - b0, nv).transpose(1, 0, 2)
    return out


def round_blocks(F, diag, dtype=np.float64):
    """the off-diagonal blocks through fp32, the diagonal ones as they are"""
    F = np.asarray(F, dtype=np.float64)
    with np.errstate(over="ignore"):
        R = F.astype(np.float32).astype(dtype)
    R[diag] = F[diag]
    return R


def rounded(f, dtype=np.float64, val=None, uinv=None):
    """a solve_ref_ilu.Factor whose apply() runs the sweeps of f's factor -- or of the downloaded one, val / uinv -- with the
    off-diagonal blocks rounded to fp32, in `dtype`"""
    g = solve_ref_ilu.Factor.__new__(solve_ref_ilu.Factor)
    g.__dict__.update(f.__dict__)
    F = f.F if val is None else blocks_of(f.bptr, val, f.nv)
    g.F = round_blocks(F, f.diag, dtype)
    g.Uinv = np.asarray(f.Uinv if uinv is None else uinv, dtype=np.float64).reshape(f.n, f.nv, f.nv).astype(dtype)
    g.dtype = dtype
    g._sweeps = None
    return g


def unrounded(f, dtype, val, uinv):
    """the same from a downloaded factor without the rounding: the FP64 apply of the device's factor"""
    g = rounded(f, dtype, val, uinv)
    g.F = blocks_of(f.bptr, val, f.nv).astype(dtype)
    return g


def overflows(F, diag):
    """entries of the off-diagonal blocks that are finite in FP64 and not in fp32: what sends a solve back to the FP64 sweeps"""
    F = np.asarray(F, dtype=np.float64)
    with np.errstate(over="ignore"):
        bad = np.isfinite(F) & ~np.isfinite(F.astype(np.float32))
    bad[diag] = False
    return int(np.count_nonzero(bad))


def bicgstab(A, b, x0, rel_tol, abs_tol=0.0, max_its=10000, nv=1, factor=None, mixed=False):
    """solve_ref.bicgstab on block Jacobi's system with the sweeps of the rounded factor from the right; mixed: the operator inside
    an iteration is solve_ref_mixed.scaled_f32, the fp32 copy of D^-1 A.  factor: a rounded() one (default: of Factor(A, nv))"""
    g = factor or rounded(solve_ref_ilu.Factor(A, nv))
    op = None
    if mixed:
        A32 = solve_ref_mixed.scaled_f32(A, nv, 2)
        op = lambda y: A32 @ y   # noqa: E731
    x, info = solve_ref.bicgstab(A, b, x0, rel_tol, abs_tol, max_its, 2, nv, operator=op, right=g.apply)
    info.update(colours=int(g.colour.max()) + 1)
    return x, info


def yardstick_dist(name, world, O, rel_tol):
    """(gathered x, info) of solve_ref_ilu_dist.bicgstab_dist with every rank's factor rounded, from x0 = 0; computed once"""
    key = (name, world, rel_tol)
    if key not in _YARD:
        s = solve_ref_dist.case(name)
        ranks = solve_ref_dist.ranks_of(name, world, O)
        fk = (name, world, "factors")
        if fk not in _YARD:
            _YARD[fk] = [rounded(f).apply for f in solve_ref_ilu_dist.factors(ranks, s.nv)]
        xs, info = solve_ref_ilu_dist.bicgstab_dist(ranks, [np.zeros(rk.A.shape[1]) for rk in ranks], rel_tol, nv=s.nv, max_its=2000,
                                                    right=_YARD[fk])
        _YARD[key] = (solve_ref_dist.gather(ranks, xs, s.nv, s.xyz.shape[0]), info)
    return _YARD[key]
