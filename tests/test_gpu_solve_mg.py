"""RDC_PRECOND_MULTIGRID through the C-ABI (rdc_solve, rdc_solve_mixed with precond = 3; rdc_solve_mg_levels): every case
assembles on the GPU, downloads values, rhs and pattern once and is judged on the host -- the residual inequality of the
block-Jacobi solve (solve_ref.check_solution with precond = 2: the cycle is applied from the right, the norm is the same),
iteration counts and level sizes against tests/solve_ref_mg.py (the same algorithm in numpy) on the same downloaded system.

Shapes: K(8) has three levels, the last below one workgroup; the hub has a row of 740 blocks and one giant aggregate; the
hydrogel mesh gives irregular aggregates; HEX8 / solid have 3 unknowns per node and 27-block rows.
Iteration slack: the device inverts the diagonal blocks and adds its sums in an order of its own, so a count may differ from the
yardstick's by an iteration or two at the stopping threshold: at most yardstick + 2."""
import numpy as np
import pytest

import solve_ref
import solve_ref_mg
from solve_systems import _dev, _open
from rdcfes_amd import RdcError
from rdcfes_amd.context import PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, SOLVE_BAD_DIAGONAL, SOLVE_CONVERGED

pytestmark = pytest.mark.gpu
SLACK = 2


def _solve(ctx, n, **kw):
    xd = _dev(np.zeros(n))
    info = ctx.solve(xd.data_ptr(), max_its=2000, **kw)
    return info, xd.cpu().numpy()


@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex", "solid_cube", "pihna_hub", "pihna_hydrogel"])
def test_multigrid_solve(name):
    ctx, s, A, rhs, val = _open(name)
    b = s.rhs_scale * rhs
    H = solve_ref_mg.Hierarchy(A, s.nv)
    with ctx:
        with pytest.raises(RdcError) as ei:                  # no hierarchy before the first multigrid solve
            ctx.mg_levels()
        assert ei.value.code == 3
        for rel_tol in (1e-8, 1e-10):
            info, x = _solve(ctx, rhs.size, rel_tol=rel_tol, precond=PRECOND_MULTIGRID, rhs_scale=s.rhs_scale)
            _, ref = solve_ref_mg.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=s.nv, max_its=2000, hierarchy=H)
            _, bj = solve_ref.bicgstab(A, b, np.zeros(b.size), rel_tol, precond=2, nv=s.nv, max_its=2000)
            levels, (setup_ms, nbytes) = ctx.mg_levels(), ctx.mg_stats()
            print(f"{name} tol {rel_tol:g}: iterations GPU {info.iterations} (restarts {info.restarts}), yardstick {ref['iterations']}, "
                  f"block Jacobi yardstick {bj['iterations']}; levels {levels}; {info.device_ms:.2f} ms, hierarchy set-up {setup_ms:.3f} ms, "
                  f"{nbytes} bytes")
            assert info.reason == SOLVE_CONVERGED and ref["reason"] == solve_ref_mg.CONVERGED, (info, ref)
            f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
            assert abs(info.residual_norm - f["residual_norm"]) <= f["rho"], (info, f)
            assert abs(info.rhs_norm - f["rhs_norm"]) <= 1e-13 * f["rhs_norm"], (info, f)
            assert info.iterations <= ref["iterations"] + SLACK, (info.iterations, ref)
            assert info.matrix_bits == 64 and info.bad_blocks == 0
            assert levels == H.level_sizes() and len(levels) >= 3
            assert 0.0 <= setup_ms <= info.device_ms and nbytes > 8 * sum(blk * s.nv * s.nv for _, blk in levels[1:])
        v, r = ctx.csr_download()
        assert v.tobytes() == val.tobytes() and r.tobytes() == rhs.tobytes(), "CSR values / rhs were modified"


def test_two_solves_are_bitwise_equal():
    ctx, s, A, rhs, val = _open("pihna_hydrogel")
    with ctx:
        ia, xa = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        ib, xb = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
    assert ia.reason == ib.reason == SOLVE_CONVERGED
    assert (ia.iterations, ia.restarts) == (ib.iterations, ib.restarts) and xa.tobytes() == xb.tobytes()
    assert ia.residual_norm == ib.residual_norm


def test_mixed_multigrid_on_pihna():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    H = solve_ref_mg.Hierarchy(A, s.nv)
    with ctx:
        for rel_tol in (1e-8, 1e-10):
            info, x = _solve(ctx, rhs.size, rel_tol=rel_tol, precond=PRECOND_MULTIGRID, mixed=True)
            _, ref = solve_ref_mg.bicgstab(A, rhs, np.zeros(rhs.size), rel_tol, nv=s.nv, hierarchy=H)
            print(f"mixed multigrid tol {rel_tol:g}: {info.iterations} iterations, {info.restarts} restarts (FP64 yardstick {ref['iterations']})")
            assert info.reason == SOLVE_CONVERGED and info.matrix_bits == 32
            solve_ref.check_solution(A, rhs, x, s.nv, 2, rel_tol)
        assert ctx.mg_levels() == H.level_sizes()


def test_block_jacobi_is_undisturbed_and_the_damping_is_an_option():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        i0, x0 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)
        m0, y0 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        i1, x1 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)
        assert i0.reason == i1.reason == m0.reason == SOLVE_CONVERGED
        assert (i0.iterations, i0.restarts, i0.residual_norm) == (i1.iterations, i1.restarts, i1.residual_norm)
        assert x0.tobytes() == x1.tobytes(), "a multigrid solve changed what the block-Jacobi solve returns"
        _, ref = solve_ref.bicgstab(A, rhs, np.zeros(rhs.size), 1e-10, precond=2, nv=s.nv)
        assert i0.iterations <= 2 * ref["iterations"] + 2 and m0.iterations < i0.iterations
        # "mg_omega", in thousandths: the default is 600; a value out of (0, 2) is refused and changes nothing
        ctx.set_option("mg_omega", 600)
        m1, y1 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        assert m1.iterations == m0.iterations and y1.tobytes() == y0.tobytes()
        for bad in (0, 2000, -600):
            with pytest.raises(RdcError) as ei:
                ctx.set_option("mg_omega", bad)
            assert ei.value.code == 1
        ctx.set_option("mg_omega", 500)
        m2, y2 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        _, ref2 = solve_ref_mg.bicgstab(A, rhs, np.zeros(rhs.size), 1e-10, nv=s.nv, omega=0.5)
        assert m2.reason == SOLVE_CONVERGED and y2.tobytes() != y0.tobytes() and m2.iterations <= ref2["iterations"] + SLACK
        solve_ref.check_solution(A, rhs, y2, s.nv, 2, 1e-10)


def test_zeroed_diagonal_block_is_reported():
    import torch
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    with ctx:
        vptr, _ = ctx.csr_values_device_ptr()

        class _V:
            pass
        v = _V()
        v.__cuda_array_interface__ = {"shape": (val.size,), "typestr": "<f8", "data": (vptr, False), "version": 2, "strides": None}
        val_d = torch.as_tensor(v, device="cuda:0")
        rp, col = ctx.csr_pattern()
        node = 11
        idx = np.concatenate([np.arange(rp[node * 5 + a], rp[node * 5 + a + 1])[col[rp[node * 5 + a]:rp[node * 5 + a + 1]] // 5 == node]
                              for a in range(5)])
        assert idx.size == 25
        keep = val_d.clone()
        val_d[torch.from_numpy(idx).to("cuda:0")] = 0.0
        for mixed in (False, True):
            x0 = np.random.default_rng(2).uniform(size=n)
            xd = _dev(x0)
            info = ctx.solve(xd.data_ptr(), rel_tol=1e-10, max_its=2000, precond=PRECOND_MULTIGRID, mixed=mixed)
            assert info.reason == SOLVE_BAD_DIAGONAL and info.bad_blocks >= 1 and info.iterations == 0
            assert xd.cpu().numpy().tobytes() == x0.tobytes()
        val_d.copy_(keep)
        torch.cuda.synchronize()
        info, x = _solve(ctx, n, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        assert info.reason == SOLVE_CONVERGED
        solve_ref.check_solution(A, rhs, x, 5, 2, 1e-10)


def test_ghosted_context_is_refused():
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        xd = _dev(np.zeros(rhs.size))
        for mixed in (False, True):
            with pytest.raises(RdcError, match="ghost") as ei:
                ctx.solve(xd.data_ptr(), precond=PRECOND_MULTIGRID, mixed=mixed)
            assert ei.value.code == 4
