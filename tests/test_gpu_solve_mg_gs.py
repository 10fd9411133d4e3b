"""The multicolour Gauss-Seidel smoother of RDC_PRECOND_MULTIGRID through the C-ABI (rdc_set_option "mg_smoother" = 1 and
"mg_gs_fuse", rdc_solve, rdc_solve_mixed, rdc_solve_mg_colours): every case assembles on the GPU, downloads values, rhs and
pattern once and is judged on the host -- the residual inequality of the block-Jacobi solve (solve_ref.check_solution with
precond = 2), iteration counts and colours against tests/solve_ref_mg_gs.py (the same algorithm in numpy) on the same system.

Shapes: K(8) has coarse levels of 95 and 14 nodes -- colours of fewer nodes than the 16 of a workgroup, and levels that sweep in
one launch; the hub has a row of 740 blocks; the hydrogel mesh has irregular rows and a level 0 above the fused size; HEX8 / solid
have 3 unknowns per node and 27-block rows.
Iteration slack: the device inverts the diagonal blocks and adds its sums in an order of its own, so a count may differ from the
yardstick's by an iteration or two at the stopping threshold: at most yardstick + 2 (tests/test_gpu_solve_mg.py)."""
import numpy as np
import pytest

import solve_ref
import solve_ref_mg
import solve_ref_mg_gs
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import RdcError, partition
from rdcfes_amd.context import (ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED, PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, SOLVE_BAD_DIAGONAL,
                                SOLVE_CONVERGED)

pytestmark = pytest.mark.gpu
SLACK = 2
_YARD = {}


def _solve(ctx, n, **kw):
    xd = _dev(np.zeros(n))
    info = ctx.solve(xd.data_ptr(), max_its=2000, **kw)
    return info, xd.cpu().numpy()


def _yardstick(name, A, b, nv, rel_tol):
    """(Gauss-Seidel hierarchy, yardstick info) of the downloaded system; the hierarchy once per system, a solve once per tolerance"""
    if name not in _YARD:
        _YARD[name] = solve_ref_mg_gs.Hierarchy(A, nv)
    if (name, rel_tol) not in _YARD:
        _YARD[(name, rel_tol)] = solve_ref_mg_gs.bicgstab(A, b, np.zeros(b.size), rel_tol, nv=nv, max_its=2000, hierarchy=_YARD[name])[1]
    return _YARD[name], _YARD[(name, rel_tol)]


def _same(a, b):
    return (a.reason, a.iterations, a.restarts, a.residual_norm) == (b.reason, b.iterations, b.restarts, b.residual_norm)


@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex", "solid_cube", "pihna_hub", "pihna_hydrogel"])
def test_gauss_seidel_solve(name):
    ctx, s, A, rhs, val = _open(name)
    b = s.rhs_scale * rhs
    with ctx:
        ctx.set_option("mg_smoother", 1)
        with pytest.raises(RdcError) as ei:                  # no colours before the first solve with the smoother
            ctx.mg_colours()
        assert ei.value.code == ERR_STATE
        for rel_tol in (1e-8, 1e-10):
            info, x = _solve(ctx, rhs.size, rel_tol=rel_tol, precond=PRECOND_MULTIGRID, rhs_scale=s.rhs_scale)
            H, ref = _yardstick(name, A, b, s.nv, rel_tol)
            levels, colours = ctx.mg_levels(), ctx.mg_colours()
            print(f"{name} tol {rel_tol:g}: iterations GPU {info.iterations} (restarts {info.restarts}), yardstick {ref['iterations']}; "
                  f"levels {levels}, colours {colours}; {info.device_ms:.2f} ms")
            assert info.reason == SOLVE_CONVERGED and ref["reason"] == solve_ref_mg_gs.CONVERGED, (info, ref)
            f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
            assert abs(info.residual_norm - f["residual_norm"]) <= f["rho"], (info, f)
            assert info.iterations <= ref["iterations"] + SLACK, (info.iterations, ref)
            assert info.matrix_bits == 64 and info.bad_blocks == 0
            assert colours == H.colours()
            assert levels == H.level_sizes() and len(levels) >= 3
        _unchanged(ctx, val, rhs)


@pytest.mark.parametrize("name", ["pihna_hydrogel", "hcc_hex"])
def test_two_solves_and_both_launch_shapes_are_bitwise_equal(name):
    ctx, s, A, rhs, val = _open(name)
    kw = dict(rel_tol=1e-10, precond=PRECOND_MULTIGRID, rhs_scale=s.rhs_scale)
    with ctx:
        ctx.set_option("mg_smoother", 1)
        ia, xa = _solve(ctx, rhs.size, **kw)
        ib, xb = _solve(ctx, rhs.size, **kw)
        ctx.set_option("mg_gs_fuse", 0)                      # one launch per colour on the small levels too
        ic, xc = _solve(ctx, rhs.size, **kw)
        ctx.set_option("mg_gs_fuse", 1)
        id_, xd = _solve(ctx, rhs.size, **kw)
        for bad in (2, -1):
            with pytest.raises(RdcError) as ei:
                ctx.set_option("mg_gs_fuse", bad)
            assert ei.value.code == ERR_INVALID
    assert ia.reason == SOLVE_CONVERGED
    assert _same(ia, ib) and xa.tobytes() == xb.tobytes(), "two solves differ"
    assert _same(ia, ic) and xa.tobytes() == xc.tobytes(), "one launch per colour differs from one launch per sweep"
    assert _same(ia, id_) and xa.tobytes() == xd.tobytes()


def test_mixed_precision_on_pihna():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        ctx.set_option("mg_smoother", 1)
        for fuse in (1, 0):      # level 0 of K(8) has 729 nodes: k_gs_f32 per colour either way; the levels below change shape
            ctx.set_option("mg_gs_fuse", fuse)
            for rel_tol in (1e-8, 1e-10):
                info, x = _solve(ctx, rhs.size, rel_tol=rel_tol, precond=PRECOND_MULTIGRID, mixed=True)
                H, ref = _yardstick("pihna_kuhn", A, rhs, s.nv, rel_tol)
                print(f"mixed Gauss-Seidel tol {rel_tol:g} fuse {fuse}: {info.iterations} iterations, {info.restarts} restarts "
                      f"(FP64 yardstick {ref['iterations']})")
                assert info.reason == SOLVE_CONVERGED and info.matrix_bits == 32
                assert info.iterations <= 1.5 * ref["iterations"] + 2
                solve_ref.check_solution(A, rhs, x, s.nv, 2, rel_tol)
        assert ctx.mg_levels() == H.level_sizes() and ctx.mg_colours() == H.colours()


def test_mixed_precision_sweeps_level_0_in_one_launch_on_a_small_mesh():
    """ripf_tet has 343 nodes: level 0 itself is below the fused size, so the fp32 sweep of level 0 runs in one workgroup"""
    ctx, s, A, rhs, val = _open("ripf_tet")
    out = []
    with ctx:
        ctx.set_option("mg_smoother", 1)
        for fuse in (1, 0):
            ctx.set_option("mg_gs_fuse", fuse)
            out.append(_solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID, mixed=True))
        f64, x64 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
    (ia, xa), (ib, xb) = out
    H, ref = _yardstick("ripf_tet", A, rhs, s.nv, 1e-10)
    assert ia.reason == f64.reason == SOLVE_CONVERGED and ia.matrix_bits == 32 and f64.matrix_bits == 64
    assert _same(ia, ib) and xa.tobytes() == xb.tobytes()
    print(f"ripf_tet: mixed {ia.iterations} iterations, FP64 {f64.iterations}, yardstick {ref['iterations']}")
    assert f64.iterations <= ref["iterations"] + SLACK
    solve_ref.check_solution(A, rhs, xa, s.nv, 2, 1e-10)
    solve_ref.check_solution(A, rhs, x64, s.nv, 2, 1e-10)


def test_the_default_is_undisturbed():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        for bad in (2, -1, 600):                             # refused, and changes nothing
            with pytest.raises(RdcError) as ei:
                ctx.set_option("mg_smoother", bad)
            assert ei.value.code == ERR_INVALID
        m0, y0 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        j0, x0 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)
        levels, nbytes = ctx.mg_levels(), ctx.mg_stats()[1]
        with pytest.raises(RdcError) as ei:
            ctx.mg_colours()
        assert ei.value.code == ERR_STATE
        ctx.set_option("mg_smoother", 1)
        g, z = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        assert g.reason == SOLVE_CONVERGED and z.tobytes() != y0.tobytes()
        j1, x1 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)   # the option touches the multigrid cycle only
        ctx.set_option("mg_smoother", 0)
        m2, y2 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        j2, x2 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)
        assert m0.reason == j0.reason == SOLVE_CONVERGED
        assert _same(m0, m2) and y0.tobytes() == y2.tobytes(), "a Gauss-Seidel solve changed what the default multigrid solve returns"
        assert _same(j0, j1) and _same(j0, j2) and x0.tobytes() == x1.tobytes() == x2.tobytes()
        assert ctx.mg_levels() == levels and ctx.mg_stats()[1] == nbytes
        _, ref = solve_ref_mg.bicgstab(A, rhs, np.zeros(rhs.size), 1e-10, nv=s.nv)
        assert m0.iterations <= ref["iterations"] + SLACK
        _unchanged(ctx, val, rhs)


def test_ghosted_context_is_refused():
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        ctx.set_option("mg_smoother", 1)
        xd = _dev(np.zeros(rhs.size))
        for mixed in (False, True):
            with pytest.raises(RdcError, match="ghost") as ei:
                ctx.solve(xd.data_ptr(), precond=PRECOND_MULTIGRID, mixed=mixed)
            assert ei.value.code == ERR_UNSUPPORTED


def test_the_partitioned_multigrid_solve_refuses_the_smoother():
    from rdcfes_amd import SolveComm
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        lp = partition.build_local(s.conn, s.xyz, np.zeros(s.conn.shape[0], dtype=np.int32), 0, 1)
        comm = SolveComm(lp, s.nv, "cuda:0", sized=True)
        x0 = np.random.default_rng(5).uniform(size=rhs.size)
        xd = _dev(x0)
        ctx.set_option("mg_smoother", 1)
        with pytest.raises(RdcError, match="mg_smoother") as ei:
            ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-8, precond=PRECOND_MULTIGRID)
        assert ei.value.code == ERR_UNSUPPORTED
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        assert (comm.exchanges, comm.sized_exchanges, comm.allreduces) == (0, 0, 0)
        ctx.set_option("mg_smoother", 0)                     # with the default the partitioned solve is what it was
        ia = ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-8, precond=PRECOND_MULTIGRID)
        ib, xb = _solve(ctx, rhs.size, rel_tol=1e-8, precond=PRECOND_MULTIGRID)
        assert ia.reason == ib.reason == SOLVE_CONVERGED


def test_zeroed_diagonal_block_is_reported():
    import torch
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    with ctx:
        ctx.set_option("mg_smoother", 1)
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
