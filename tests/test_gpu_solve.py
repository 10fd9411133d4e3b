"""Device-resident linear solve through the C-ABI (rdc_csr_matvec, rdc_solve): every case assembles on the GPU, downloads
values, rhs and pattern once, and is judged on the host with scipy -- never against the library's own output.  The
residual inequality, its rounding term and the per-unknown form are written down once in solve_ref.check_solution;
iteration counts are held against tests/solve_ref.py (the same algorithm in numpy) on the same downloaded system.

RIPF: the solver case takes its time step from the state (cell Courant number 1, solve_systems.ripf_tet); at the
shipped time_step 0.1 the synthetic system is indefinite and no Jacobi-class Krylov method converges on it
(tests/test_solve_ref.py): test_ripf_at_courant_900_reports_non_convergence holds the library to saying so truthfully."""
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref
import solve_systems
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import AssemblyContext, RdcError
from rdcfes_amd.context import (FIELD_OLD_SOLUTION, PRECOND_BLOCK_JACOBI, SOLVE_BAD_DIAGONAL, SOLVE_CONVERGED, SOLVE_MAX_ITS,
                                SOLVE_NOT_FINITE)

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("name", list(solve_systems.MATVEC_SYSTEMS))
def test_matvec(name):
    ctx, s, A, rhs, val = _open(name)
    with ctx:
        x = np.random.default_rng(5).uniform(-1.0, 1.0, A.shape[1])
        y = ctx.csr_matvec(x)
        y2 = ctx.csr_matvec(x)
        _unchanged(ctx, val, rhs)
    L = solve_ref.longest_row(A)
    bound = 4.0 * L * EPS * (abs(A) @ np.abs(x))
    err = np.abs(y - A @ x)
    print(f"{name}: rows {A.shape[0]}, longest row {L}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3e}")
    assert y.shape == (A.shape[0],)
    assert np.all(err <= bound)
    assert y.tobytes() == y2.tobytes()
    if name == "pihna_ghosted":
        assert A.shape[0] < A.shape[1]
    if name == "pihna_hub":
        assert L > 3 * 5 * 245


def _check(ctx, s, A, rhs, x0, rel_tol, precond, info, x, max_ref_its=5000):
    b = s.rhs_scale * rhs
    assert info.reason == SOLVE_CONVERGED, info
    f = solve_ref.check_solution(A, b, x, s.nv, precond, rel_tol)
    assert abs(info.residual_norm - f["residual_norm"]) <= f["rho"], (info, f)
    assert abs(info.plain_residual_norm - f["plain_residual_norm"]) <= f["plain_rho"], (info, f)
    print(f"{s.name}: rhs norm rel. difference {abs(info.rhs_norm - f['rhs_norm']) / f['rhs_norm']:.2e} (preconditioned), "
          f"{abs(info.plain_rhs_norm - f['plain_rhs_norm']) / f['plain_rhs_norm']:.2e} (plain); max cond_inf(D_block) {f['cond']:.2e}")
    assert abs(info.rhs_norm - f["rhs_norm"]) <= 1e-13 * f["rhs_norm"], (info, f)
    assert abs(info.plain_rhs_norm - f["plain_rhs_norm"]) <= 1e-13 * f["plain_rhs_norm"], (info, f)
    _, ref = solve_ref.bicgstab(A, b, x0, rel_tol, precond=precond, nv=s.nv, max_its=max_ref_its)
    print(f"{s.name} tol {rel_tol:g} precond {precond}: iterations GPU {info.iterations} (restarts {info.restarts}), yardstick "
          f"{ref['iterations']}; residual {f['residual_norm']:.3e} <= {f['bound']:.3e}, {info.device_ms:.2f} ms")
    assert info.iterations <= 2 * ref["iterations"] + 2, (info.iterations, ref)


def _solve_cases():
    for name in solve_systems.SOLVE_SYSTEMS:
        tols = (1e-3, 1e-8, 1e-10) if name == "solid_cube" else (1e-8, 1e-10)
        for tol in tols:
            yield name, tol


@pytest.mark.parametrize("name,rel_tol", list(_solve_cases()))
def test_solve(name, rel_tol):
    """x0 = 0 and x0 = the old solution (the solid system solves for a Newton update, whose old value is 0: one start)"""
    ctx, s, A, rhs, val = _open(name)
    with ctx:
        starts = [np.zeros(rhs.size)]
        if FIELD_OLD_SOLUTION in s.fields:
            starts.append(np.ascontiguousarray(s.fields[FIELD_OLD_SOLUTION], dtype=np.float64).reshape(-1))
        for x0 in starts:
            xd = _dev(x0)
            info = ctx.solve(xd.data_ptr(), rel_tol=rel_tol, max_its=2000, rhs_scale=s.rhs_scale)
            _check(ctx, s, A, rhs, x0, rel_tol, PRECOND_BLOCK_JACOBI, info, xd.cpu().numpy())
        _unchanged(ctx, val, rhs)


@pytest.mark.parametrize("precond", [0, 1, 2])
def test_three_preconditioners_on_pihna(precond):
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        for rel_tol in (1e-8, 1e-10):
            xd = _dev(np.zeros(rhs.size))
            info = ctx.solve(xd.data_ptr(), rel_tol=rel_tol, max_its=5000, precond=precond)
            _check(ctx, s, A, rhs, np.zeros(rhs.size), rel_tol, precond, info, xd.cpu().numpy())


def test_ripf_at_courant_900_reports_non_convergence():
    ctx, s, A, rhs, val = _open("ripf_tet_dt01")
    with ctx:
        xd = _dev(np.zeros(rhs.size))
        info = ctx.solve(xd.data_ptr(), rel_tol=1e-8, max_its=300)
        x = xd.cpu().numpy()
    M, _, cond = solve_ref.precond_inverse(A, 3, 2)
    true = float(np.linalg.norm(M @ (rhs - A @ x)))
    rho = 4.0 * solve_ref.longest_row(A) * EPS * np.linalg.norm(abs(M) @ (abs(A) @ np.abs(x) + np.abs(rhs)))
    print(info, true)
    assert info.reason == SOLVE_MAX_ITS and info.iterations == 300 and np.all(np.isfinite(x))
    assert abs(info.residual_norm - true) <= rho + 64.0 * EPS * cond * true
    assert true > 1e-8 * info.rhs_norm


def test_time_loop(oracle):
    """Three steps of assemble -> solve(1e-10, in place in FIELD_OLD_SOLUTION) -> clamp on K(8), every step judged on its own
    inputs: the oracle assembles from the downloaded state before the step, and the unclamped solution must satisfy the
    solve inequality with THAT A, b (rounding term enlarged by the 1e-10 per-block assembly tolerance of tests/parity.py)."""
    import time_loop
    s = solve_systems.get("pihna_kuhn")
    seen = {}

    def on_step(k, phase, ctx):
        if phase == "assembled":
            seen["before"] = ctx.field_download(FIELD_OLD_SOLUTION, ctx.n_node * 5)
            xd = _dev(seen["before"])                       # scratch vector that starts as a copy of the state
            seen["scratch_info"] = ctx.solve(xd.data_ptr(), rel_tol=1e-10, max_its=2000)
            seen["scratch"] = xd.cpu().numpy()
        else:
            seen["solved"] = ctx.field_download(FIELD_OLD_SOLUTION, ctx.n_node * 5)

    with AssemblyContext(0) as ctx:
        s.upload(ctx)
        for k in range(3):
            rec = time_loop.run(ctx, s.conn, s.params, 1, rel_tol=1e-10, max_its=2000, on_step=on_step)[0]
            assert rec["reason"] == SOLVE_CONVERGED and seen["scratch_info"].reason == SOLVE_CONVERGED
            assert seen["scratch"].tobytes() == seen["solved"].tobytes(), "in-place solve differs from the solve into a scratch vector"
            rp, col, val0, rhs0 = s.oracle_assemble(oracle, u_old=seen["before"].reshape(-1, 5))
            A0 = sps.csr_matrix((val0, col, rp), shape=(rhs0.size, rhs0.size))
            f = solve_ref.check_solution(A0, rhs0, seen["solved"], 5, 2, 1e-10, extra_rel=1e-10)
            after = ctx.field_download(FIELD_OLD_SOLUTION, ctx.n_node * 5)
            assert after.tobytes() == np.maximum(seen["solved"], 0.0).tobytes()
            u = after.reshape(-1, 5)
            bg = (u[:, 0] == 0) & (u[:, 1] == 0) & (u[:, 2] == 0) & (u[:, 4] == 0)
            assert rec["background_nodes"] == float(bg.astype(np.float64).mean())
            assert rec["background_elems"] == float(bg[s.conn.astype(np.int64)].all(axis=1).astype(np.float64).mean())
            print(f"step {k + 1}: {rec['iterations']} iterations, residual {f['residual_norm']:.3e} <= {f['bound']:.3e}, background "
                  f"nodes {rec['background_nodes']:.4f} elements {rec['background_elems']:.4f}")


def test_outcomes_and_refusals():
    import torch
    with AssemblyContext(0) as ctx:
        xd = _dev(np.zeros(16))
        with pytest.raises(RdcError) as ei:                                    # before a mesh upload
            ctx._ck(ctx._lib.rdc_solve(ctx._h, None, None, None))
        assert ei.value.code == 3
        with pytest.raises(RdcError) as ei:
            ctx.csr_matvec_device(xd.data_ptr(), xd.data_ptr())
        assert ei.value.code == 3
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:                                                                  # ghosts: matvec fine (test_matvec), solve refused
        xd = _dev(np.zeros(rhs.size))
        with pytest.raises(RdcError, match="ghost") as ei:
            ctx.solve(xd.data_ptr())
        assert ei.value.code == 4
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    with ctx:
        good = dict(rel_tol=1e-10, max_its=2000)
        for bad in (dict(max_its=0), dict(rel_tol=-1.0), dict(rel_tol=float("nan")), dict(abs_tol=float("inf")), dict(precond=7)):
            xd = _dev(np.zeros(n))
            with pytest.raises(RdcError) as ei:
                ctx.solve(xd.data_ptr(), **dict(good, **bad))
            assert ei.value.code == 1, bad
            with pytest.raises(RdcError) as ei:
                ctx._ck(ctx._lib.rdc_solve(ctx._h, None, xd.data_ptr(), None))
            assert ei.value.code == 1
            info = ctx.solve(xd.data_ptr(), **good)                            # the context is still usable
            assert info.reason == SOLVE_CONVERGED
            solve_ref.check_solution(A, rhs, xd.cpu().numpy(), 5, 2, 1e-10)
        # max_its = 1: the last iterate, finite, residual reported truthfully
        xd = _dev(np.zeros(n))
        info = ctx.solve(xd.data_ptr(), rel_tol=1e-10, max_its=1)
        x = xd.cpu().numpy()
        assert info.reason == SOLVE_MAX_ITS and info.iterations == 1 and np.all(np.isfinite(x))
        M, _, cond = solve_ref.precond_inverse(A, 5, 2)
        res = M @ (rhs - A @ x)
        rho = 4.0 * solve_ref.longest_row(A) * EPS * np.linalg.norm(abs(M) @ (abs(A) @ np.abs(x) + np.abs(rhs)))
        assert abs(info.residual_norm - np.linalg.norm(res)) <= rho + 64.0 * EPS * cond * np.linalg.norm(res)
        assert info.residual_norm > 1e-10 * info.rhs_norm
        # b = 0: x = 0 whatever the start
        vptr, rptr = ctx.csr_values_device_ptr()

        class _V:
            pass
        def view(ptr, count):
            v = _V()
            v.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False), "version": 2, "strides": None}
            return torch.as_tensor(v, device="cuda:0")
        rhs_d, val_d = view(rptr, n), view(vptr, val.size)
        keep_rhs = rhs_d.clone()
        rhs_d.zero_()
        xd = _dev(np.ones(n))
        info = ctx.solve(xd.data_ptr(), **good)
        assert info.reason == SOLVE_CONVERGED and info.iterations == 0 and not xd.cpu().numpy().any()
        # NaN in the rhs: ordinary data, reported
        rhs_d.copy_(keep_rhs)
        rhs_d[7] = float("nan")
        xd = _dev(np.zeros(n))
        info = ctx.solve(xd.data_ptr(), **good)
        assert info.reason == SOLVE_NOT_FINITE and not xd.cpu().numpy().any()
        rhs_d.copy_(keep_rhs)
        # a rhs whose norm overflows: reported before x is touched
        rhs_d.mul_(1e200)
        x0 = np.random.default_rng(3).uniform(size=n)
        xd = _dev(x0)
        info = ctx.solve(xd.data_ptr(), **good)
        assert info.reason == SOLVE_NOT_FINITE and xd.cpu().numpy().tobytes() == x0.tobytes()
        rhs_d.copy_(keep_rhs)
        # one diagonal block zeroed: reported, x untouched
        rp, col = ctx.csr_pattern()
        node = 11
        idx = np.concatenate([np.arange(rp[node * 5 + a], rp[node * 5 + a + 1])[col[rp[node * 5 + a]:rp[node * 5 + a + 1]] // 5 == node]
                              for a in range(5)])
        assert idx.size == 25
        keep_val = val_d.clone()
        val_d[torch.from_numpy(idx).to("cuda:0")] = 0.0
        x0 = np.random.default_rng(2).uniform(size=n)
        xd = _dev(x0)
        info = ctx.solve(xd.data_ptr(), **good)
        assert info.reason == SOLVE_BAD_DIAGONAL and info.bad_blocks == 1
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        val_d.copy_(keep_val)
        torch.cuda.synchronize()
        xd = _dev(np.zeros(n))
        assert ctx.solve(xd.data_ptr(), **good).reason == SOLVE_CONVERGED


def test_field_keyword_and_exclusive_arguments():
    ctx, s, A, rhs, val = _open("hcc_tet")
    with ctx:
        with pytest.raises(ValueError):
            ctx.solve()
        with pytest.raises(ValueError):
            ctx.solve(1234, field=FIELD_OLD_SOLUTION)
        x0 = ctx.field_download(FIELD_OLD_SOLUTION, rhs.size)
        info = ctx.solve(field=FIELD_OLD_SOLUTION, rel_tol=1e-10, max_its=2000)
        x = ctx.field_download(FIELD_OLD_SOLUTION, rhs.size)
        _check(ctx, s, A, rhs, x0, 1e-10, PRECOND_BLOCK_JACOBI, info, x)


def test_solve_on_a_non_default_stream():
    import torch
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        xa = _dev(np.zeros(rhs.size))
        ia = ctx.solve(xa.data_ptr(), rel_tol=1e-10, max_its=2000)
        stream = torch.cuda.Stream()
        xb = _dev(np.zeros(rhs.size))
        torch.cuda.synchronize()
        ctx.set_stream(stream.cuda_stream)
        ib = ctx.solve(xb.data_ptr(), rel_tol=1e-10, max_its=2000)
        yb = torch.empty(rhs.size, dtype=torch.float64, device="cuda:0")
        ctx.csr_matvec_device(xb.data_ptr(), yb.data_ptr())
        ctx.synchronize()
        ctx.set_stream(0)
        assert ia.reason == ib.reason == SOLVE_CONVERGED and ia.iterations == ib.iterations
        assert xa.cpu().numpy().tobytes() == xb.cpu().numpy().tobytes()
        assert np.all(np.abs(yb.cpu().numpy() - A @ xb.cpu().numpy()) <= 4.0 * solve_ref.longest_row(A) * EPS * (abs(A) @ np.abs(xb.cpu().numpy())))
