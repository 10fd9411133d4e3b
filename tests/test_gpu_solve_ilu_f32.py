"""The fp32 copy of the block ILU(0) factor through the C-ABI (option "ilu_factor_bits" = 32; rdc_solve and rdc_solve_mixed with
precond = 4 or 5, rdc_solve_ilu_apply, rdc_solve_ilu_factor_bits): every case assembles on the GPU, downloads values, rhs and
pattern once and is judged on the host against tests/solve_ref_ilu_f32.py built from the DOWNLOADED system.

Apply: the reference is the extended-precision sweeps of the FP64 factor the DEVICE built (rdc_solve_ilu_download), rounded to
fp32 by numpy, with the downloaded U_ii^-1 -- a last-bit difference between two FP64 factors can flip an fp32 rounding, 6e-8 on an
entry, so a reference with a factor of its own would measure that and not the rounding kernel and the sweeps.  Bound =
ld.bound(64, noise), noise = numpy's FP64 evaluation of the same sweeps against the extended-precision one: the bound of
tests/test_gpu_solve_ilu.py, FP64 noise.  An fp32 subnormal the device flushes differs by less than 2^-126 on an entry.

Solve: reason, the residual inequality of the block-Jacobi solve, iterations <= yardstick + 2 with the FP64 operator (the
yardstick: the rounded factor of numpy's own factorisation), <= 2 x yardstick + 2 with the fp32 operator (the criterion of
tests/test_gpu_solve_mixed.py: the count of a mixed solve moves with the place of its restart).

Shapes: K(8) nvar 5, 15-block rows; HEX8 nvar 3, 27-block rows, 15 colours; the solid cube with rhs_scale -1; the hydrogel mesh,
irregular rows of 30 - 60 blocks whose runs are no multiples of 4 floats; the hub mesh with one row of 740 blocks."""
import numpy as np
import pytest

import solve_ref
import solve_ref_ilu
import solve_ref_ilu_f32
import solve_ref_mg_ld as ld
from solve_systems import _dev, _open, _unchanged
from test_gpu_solve_ilu import _raises, _same, _solve, _values_tensor
from rdcfes_amd.context import (ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED, PRECOND_BLOCK_JACOBI, PRECOND_ILU0, PRECOND_ILU0_LOCAL,
                                PRECOND_MULTIGRID, SOLVE_BAD_DIAGONAL, SOLVE_CONVERGED)

pytestmark = pytest.mark.gpu
FOUR = ["pihna_kuhn", "hcc_hex", "pihna_hydrogel", "pihna_hub"]
FIVE = FOUR + ["solid_cube"]
MARGIN, SLACK = 64.0, 2
EPS = ld.EPS
_REF = {}


class _Ref:
    """the lists of the yardstick factor of one downloaded system, its rounded factor, and the yardstick solves, each built once"""

    def __init__(self, A, b, nv):
        self.A, self.b, self.nv = A, b, nv
        self.f = solve_ref_ilu.Factor(A, nv)
        assert self.f.singular == 0
        self.g = solve_ref_ilu_f32.rounded(self.f)
        self._solves = {}

    def solve(self, rel_tol, mixed):
        if (rel_tol, mixed) not in self._solves:
            self._solves[(rel_tol, mixed)] = solve_ref_ilu_f32.bicgstab(self.A, self.b, np.zeros(self.b.size), rel_tol, nv=self.nv, max_its=2000,
                                                                        factor=self.g, mixed=mixed)[1]
        return self._solves[(rel_tol, mixed)]


def _ref(name, A, b, nv, val):
    if name not in _REF or _REF[name][0] != val.tobytes():
        _REF[name] = (val.tobytes(), _Ref(A, b, nv))
    return _REF[name][1]


@pytest.mark.parametrize("name", FOUR)
def test_apply_against_the_rounded_downloaded_factor(name):
    ctx, s, A, rhs, val = _open(name)
    nv = s.nv
    R = _ref(name, A, s.rhs_scale * rhs, nv, val)
    inputs = ld.probe_vectors(rhs.size, s.rhs_scale * rhs)
    if name == "pihna_hub":                          # the node that owns the row of 740 blocks
        hub = int(np.argmax(np.diff(R.f.bptr)))
        assert R.f.bptr[hub + 1] - R.f.bptr[hub] >= 740
        unit = np.zeros(rhs.size)
        unit[hub * nv] = 1.0
        inputs.append(unit)
    with ctx:
        _raises(ERR_STATE, ctx.ilu_factor_bits)
        plain = [ctx.ilu_apply(v) for v in inputs]   # the option at its default
        assert ctx.ilu_factor_bits() == 64
        bytes64 = ctx.ilu_stats()[1]
        ctx.set_option("ilu_factor_bits", 32)
        assert ctx.ilu_stats()[1] == bytes64, "the fp32 copy is counted before a call has made it"
        got = [ctx.ilu_apply(v) for v in inputs]
        again = ctx.ilu_apply(inputs[0])
        assert ctx.ilu_factor_bits() == 32
        fval, fuinv = ctx.ilu_factor()               # the FP64 factor the copy was rounded from
        bytes32 = ctx.ilu_stats()[1]
        _unchanged(ctx, val, rhs)
    gl = solve_ref_ilu_f32.rounded(R.f, dtype=np.longdouble, val=fval, uinv=fuinv.reshape(-1))
    g = solve_ref_ilu_f32.rounded(R.f, val=fval, uinv=fuinv.reshape(-1))
    zs = [gl.apply(v) for v in inputs]
    noise = max(max(ld.rel_diff(g.apply(v), z)) for v, z in zip(inputs, zs))
    err = max(max(ld.rel_diff(z32, z)) for z32, z in zip(got, zs))
    diff = [float(np.linalg.norm(a - b) / np.linalg.norm(b)) for a, b in zip(got, plain)]
    n, nblk = rhs.size // nv, val.size // nv ** 2
    off_diag = (nblk - n) * nv * nv
    print(f"{name}: fp32-factor apply error {err:.2e} = {err / max(noise, 16 * EPS):.2f} x max(noise {noise:.2e}, 16 eps); against the FP64-factor "
          f"apply {min(diff):.2e} .. {max(diff):.2e}; factor bytes {bytes64} -> {bytes32} (+{bytes32 - bytes64}, 4 x off-diagonal non-zeros = {4 * off_diag})")
    assert err <= ld.bound(MARGIN, noise), (err, noise)
    assert again.tobytes() == got[0].tobytes()
    assert all(a.tobytes() != b.tobytes() for a, b in zip(got, plain)) and 1e-9 <= min(diff) and max(diff) <= 1e-6, diff
    # 4 bytes per off-diagonal non-zero; at most 3 padding floats in each of the nvar rows of a node's two runs, 8 bytes of offset per
    # node and one more, and the alignment of the allocation's two parts
    assert 4 * off_diag <= bytes32 - bytes64 <= 4 * (off_diag + 2 * 3 * nv * n) + 8 * (n + 1) + 2 * 256


@pytest.mark.parametrize("name", FIVE)
def test_solve(name):
    ctx, s, A, rhs, val = _open(name)
    b = s.rhs_scale * rhs
    R = _ref(name, A, b, s.nv, val)
    with ctx:
        ctx.set_option("ilu_factor_bits", 32)
        for rel_tol in (1e-8, 1e-10):
            kw = dict(rel_tol=rel_tol, rhs_scale=s.rhs_scale)
            info, x = _solve(ctx, rhs.size, precond=PRECOND_ILU0, **kw)
            assert ctx.ilu_factor_bits() == 32
            ref = R.solve(rel_tol, False)
            ms = ctx.ilu_stats()[0]
            print(f"{name} tol {rel_tol:g}: fp32 factor, FP64 operator: iterations GPU {info.iterations} (restarts {info.restarts}), yardstick "
                  f"{ref['iterations']}; {info.device_ms:.2f} ms, of which set-up {ms:.2f}")
            assert info.reason == SOLVE_CONVERGED and ref["reason"] == solve_ref_ilu_f32.CONVERGED, (info, ref)
            f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
            assert abs(info.residual_norm - f["residual_norm"]) <= f["rho"], (info, f)
            assert info.iterations <= ref["iterations"] + SLACK, (info.iterations, ref)
            assert info.matrix_bits == 64 and info.bad_blocks == 0
            again, y = _solve(ctx, rhs.size, precond=PRECOND_ILU0, **kw)
            assert _same(info, again) and x.tobytes() == y.tobytes(), "two solves differ"
            local, y = _solve(ctx, rhs.size, precond=PRECOND_ILU0_LOCAL, **kw)
            assert _same(info, local) and x.tobytes() == y.tobytes(), "precond 5 without ghosts is not precond 4"
            # the fp32 operator with the fp32 factor
            mixed, xm = _solve(ctx, rhs.size, precond=PRECOND_ILU0, mixed=True, **kw)
            assert ctx.ilu_factor_bits() == 32
            ref = R.solve(rel_tol, True)
            print(f"{name} tol {rel_tol:g}: fp32 factor, fp32 operator: iterations GPU {mixed.iterations} (restarts {mixed.restarts}), yardstick "
                  f"{ref['iterations']} (restarts {ref['restarts']}); {mixed.device_ms:.2f} ms")
            assert mixed.reason == SOLVE_CONVERGED and ref["reason"] == solve_ref_ilu_f32.CONVERGED, (mixed, ref)
            f = solve_ref.check_solution(A, b, xm, s.nv, 2, rel_tol)
            assert abs(mixed.residual_norm - f["residual_norm"]) <= f["rho"], (mixed, f)
            assert mixed.iterations <= 2 * ref["iterations"] + 2, (mixed.iterations, ref)
            assert mixed.matrix_bits == 32 and mixed.bad_blocks == 0
            again, y = _solve(ctx, rhs.size, precond=PRECOND_ILU0, mixed=True, **kw)
            assert _same(mixed, again) and xm.tobytes() == y.tobytes(), "two mixed solves differ"
            local, y = _solve(ctx, rhs.size, precond=PRECOND_ILU0_LOCAL, mixed=True, **kw)
            assert _same(mixed, local) and xm.tobytes() == y.tobytes(), "precond 5 without ghosts is not precond 4 (mixed)"
        _unchanged(ctx, val, rhs)


def test_the_default_is_undisturbed():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size

    def four():
        return [_solve(ctx, n, rel_tol=1e-10, precond=PRECOND_ILU0), _solve(ctx, n, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI),
                _solve(ctx, n, rel_tol=1e-10, precond=PRECOND_MULTIGRID), _solve(ctx, n, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI, mixed=True)]
    with ctx:
        before = four()
        stats = ctx.ilu_stats()[1:]
        assert ctx.ilu_factor_bits() == 64
        x0 = np.random.default_rng(5).uniform(size=n)
        xd = _dev(x0)
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_ILU0, mixed=True), match="rdc_solve_mixed")
        e = _raises(ERR_INVALID, lambda: ctx.set_option("ilu_factor_bits", 16))
        assert "64 or 32" in str(e)
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_ILU0, mixed=True), match="rdc_solve_mixed")   # still 64
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        ctx.set_option("ilu_factor_bits", 32)
        i32, x32 = _solve(ctx, n, rel_tol=1e-10, precond=PRECOND_ILU0)
        assert i32.reason == SOLVE_CONVERGED and ctx.ilu_factor_bits() == 32 and x32.tobytes() != before[0][1].tobytes()
        _raises(ERR_INVALID, lambda: ctx.set_option("ilu_factor_bits", 16))
        assert _same(_solve(ctx, n, rel_tol=1e-10, precond=PRECOND_ILU0)[0], i32)                                                 # still 32
        ctx.set_option("ilu_factor_bits", 64)
        after = four()
        assert ctx.ilu_factor_bits() == 64
        for (ia, xa), (ib, xb), what in zip(before, after, ("ILU(0)", "block Jacobi", "multigrid", "mixed block Jacobi")):
            assert ia.reason == SOLVE_CONVERGED
            assert _same(ia, ib) and ia.matrix_bits == ib.matrix_bits and xa.tobytes() == xb.tobytes(), f"the fp32 factor changed the {what} solve"
        assert ctx.ilu_stats()[2] == stats[1] and ctx.ilu_stats()[1] > stats[0]       # the copy is kept with the mesh, and counted
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_ILU0, mixed=True), match="rdc_solve_mixed")
        _unchanged(ctx, val, rhs)


def _scalar_entries(rp, col, nv, node, other):
    """indices into the scalar CSR values of node block (node, other)"""
    return np.concatenate([np.arange(rp[node * nv + a], rp[node * nv + a + 1])[col[rp[node * nv + a]:rp[node * nv + a + 1]] // nv == other]
                           for a in range(nv)])


def test_a_factor_that_does_not_fit_fp32_falls_back_to_the_fp64_sweeps():
    import torch
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n, nv = rhs.size, s.nv
    with ctx:
        val_d = _values_tensor(ctx, val.size)
        rp, col = ctx.csr_pattern()
        node = 11
        other = int(next(j for j in col[rp[node * nv]:rp[node * nv + 1]] // nv if j != node))
        idx = _scalar_entries(rp, col, nv, node, other)
        assert idx.size == nv * nv
        val_d[torch.from_numpy(idx).to("cuda:0")] *= 1e45   # finite in FP64, above FLT_MAX behind D^-1
        torch.cuda.synchronize()
        big = val_d.cpu().numpy()
        assert np.all(np.isfinite(big)) and np.abs(big[idx]).max() > 1e40
        kw = dict(rel_tol=1e-8, precond=PRECOND_ILU0)
        xd = _dev(np.zeros(n))
        i64 = ctx.solve(xd.data_ptr(), max_its=50, **kw)
        x64 = xd.cpu().numpy()
        ctx.set_option("ilu_factor_bits", 32)
        xd = _dev(np.zeros(n))
        i32 = ctx.solve(xd.data_ptr(), max_its=50, **kw)
        x32 = xd.cpu().numpy()
        print(f"fall-back: reason {i32.reason}, {i32.iterations} iterations, factor bits {ctx.ilu_factor_bits()}")
        assert ctx.ilu_factor_bits() == 64
        assert _same(i64, i32) and i64.matrix_bits == i32.matrix_bits and x64.tobytes() == x32.tobytes()
        z64 = None
        if i64.bad_blocks == 0:                              # the hook falls back as well
            y = np.random.default_rng(3).standard_normal(n)
            z32 = ctx.ilu_apply(y)
            assert ctx.ilu_factor_bits() == 64
            ctx.set_option("ilu_factor_bits", 64)
            z64 = ctx.ilu_apply(y)
            assert z32.tobytes() == z64.tobytes()
    assert z64 is not None or i64.bad_blocks > 0


def test_zeroed_diagonal_block_is_reported_with_the_fp32_factor():
    import torch
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n, nv = rhs.size, s.nv
    with ctx:
        ctx.set_option("ilu_factor_bits", 32)
        val_d = _values_tensor(ctx, val.size)
        rp, col = ctx.csr_pattern()
        idx = _scalar_entries(rp, col, nv, 11, 11)
        assert idx.size == 25
        keep = val_d.clone()
        val_d[torch.from_numpy(idx).to("cuda:0")] = 0.0
        x0 = np.random.default_rng(2).uniform(size=n)
        for mixed in (False, True):
            xd = _dev(x0)
            info = ctx.solve(xd.data_ptr(), rel_tol=1e-10, max_its=2000, precond=PRECOND_ILU0, mixed=mixed)
            assert info.reason == SOLVE_BAD_DIAGONAL and info.bad_blocks >= 1 and info.iterations == 0
            assert xd.cpu().numpy().tobytes() == x0.tobytes()
        val_d.copy_(keep)
        torch.cuda.synchronize()
        info, x = _solve(ctx, n, rel_tol=1e-10, precond=PRECOND_ILU0)
        assert info.reason == SOLVE_CONVERGED and info.bad_blocks == 0 and ctx.ilu_factor_bits() == 32
        solve_ref.check_solution(A, rhs, x, 5, 2, 1e-10)
