"""Mixed-precision linear solve through the C-ABI (rdc_csr_scale_f32, rdc_csr_matvec_f32, rdc_solve_mixed): BiCGStab
whose iteration streams an fp32 copy of D^-1 A while everything that decides stays on the fp64 values.  As in
test_gpu_solve.py every case assembles on the GPU, downloads values, rhs and pattern once and is judged on the host with
scipy; the returned x is held to the UNCHANGED fp64 inequality solve_ref.check_solution, and iteration counts to
tests/solve_ref_mixed.py (the same algorithm in numpy) on the same downloaded system."""
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sps

import solve_ref
import solve_ref_mixed
import solve_systems
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import AssemblyContext, RdcError, pihna_params_from_dict, synth
from rdcfes_amd.context import FIELD_OLD_SOLUTION, PRECOND_BLOCK_JACOBI, PRECOND_NONE, SOLVE_CONVERGED, SOLVE_MAX_ITS

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tools"))
pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _owned_square(A):
    return A[:, :A.shape[0]].tocsr()


@pytest.mark.parametrize("name", list(solve_systems.MATVEC_SYSTEMS))
def test_matvec_f32(name):
    """per row: |y - M(Ax)|_i <= (2^-24 + 4 L eps + 64 eps cond) (|M||A||x|)_i + 2^-126 ||x||_1 -- fp32 rounding of each
    entry, fp64 accumulation over the longest row, the device's Gauss-Jordan against numpy's inverse, flushed subnormals"""
    ctx, s, A, rhs, val = _open(name)
    with ctx:
        x = np.random.default_rng(5).uniform(-1.0, 1.0, A.shape[1])
        with pytest.raises(RdcError) as ei:                # fresh mesh: no copy yet
            ctx.csr_matvec_f32(x)
        assert ei.value.code == 1
        ctx.csr_scale_f32(2)
        y = ctx.csr_matvec_f32(x)
        y2 = ctx.csr_matvec_f32(x)
        _unchanged(ctx, val, rhs)
    M, _, cond = solve_ref.precond_inverse(_owned_square(A), s.nv, 2)
    L = solve_ref.longest_row(A)
    scale = abs(M) @ (abs(A) @ np.abs(x))
    bound = (2.0 ** -24 + 4.0 * L * EPS + 64.0 * EPS * cond) * scale + 2.0 ** -126 * np.abs(x).sum()
    err = np.abs(y - M @ (A @ x))
    over64 = err > 4.0 * L * EPS * scale
    print(f"{name}: rows {A.shape[0]}, longest row {L}, cond {cond:.2e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3e}, "
          f"rows above the fp64 bound {int(over64.sum())}")
    assert y.shape == (A.shape[0],)
    assert np.all(err <= bound)
    assert y.tobytes() == y2.tobytes()
    if name in ("ripf_tet", "hcc_hex"):
        assert over64.any(), "no row shows an fp32 rounding: were the values rounded at all?"
    if name == "pihna_ghosted":
        assert A.shape[0] < A.shape[1]
    if name == "pihna_hub":
        assert L > 3 * 5 * 245


def _check(s, A, rhs, x0, rel_tol, precond, info, x, max_ref_its=5000, bits=(32,)):
    b = s.rhs_scale * rhs
    assert info.reason == SOLVE_CONVERGED, info
    assert info.matrix_bits in bits, info
    f = solve_ref.check_solution(A, b, x, s.nv, precond, rel_tol)
    assert abs(info.residual_norm - f["residual_norm"]) <= f["rho"], (info, f)
    assert abs(info.plain_residual_norm - f["plain_residual_norm"]) <= f["plain_rho"], (info, f)
    assert abs(info.rhs_norm - f["rhs_norm"]) <= 1e-13 * f["rhs_norm"], (info, f)
    assert abs(info.plain_rhs_norm - f["plain_rhs_norm"]) <= 1e-13 * f["plain_rhs_norm"], (info, f)
    ref_fn = solve_ref_mixed.bicgstab if info.matrix_bits == 32 else solve_ref.bicgstab
    _, ref = ref_fn(A, b, x0, rel_tol, precond=precond, nv=s.nv, max_its=max_ref_its)
    print(f"{s.name} tol {rel_tol:g} precond {precond} bits {info.matrix_bits}: iterations GPU {info.iterations} (restarts {info.restarts}), "
          f"yardstick {ref['iterations']} (restarts {ref['restarts']}); residual {f['residual_norm']:.3e} <= {f['bound']:.3e}, "
          f"{info.device_ms:.2f} ms")
    assert info.iterations <= 2 * ref["iterations"] + 2, (info.iterations, ref)


@pytest.mark.parametrize("rel_tol", [1e-8, 1e-10])
@pytest.mark.parametrize("name", list(solve_systems.SOLVE_SYSTEMS))
def test_solve_mixed(name, rel_tol):
    """x0 = 0 and x0 = the old solution (the solid system solves for a Newton update, whose old value is 0: one start)"""
    ctx, s, A, rhs, val = _open(name)
    with ctx:
        starts = [np.zeros(rhs.size)]
        if FIELD_OLD_SOLUTION in s.fields:
            starts.append(np.ascontiguousarray(s.fields[FIELD_OLD_SOLUTION], dtype=np.float64).reshape(-1))
        for x0 in starts:
            xd = _dev(x0)
            info = ctx.solve(xd.data_ptr(), rel_tol=rel_tol, max_its=2000, rhs_scale=s.rhs_scale, mixed=True)
            _check(s, A, rhs, x0, rel_tol, PRECOND_BLOCK_JACOBI, info, xd.cpu().numpy())
        _unchanged(ctx, val, rhs)


@pytest.mark.parametrize("precond", [0, 1, 2])
def test_three_preconditioners_on_pihna(precond):
    """whichever operator runs must be truthful: if the unscaled matrix overflowed fp32, matrix_bits says 64"""
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        xd = _dev(np.zeros(rhs.size))
        info = ctx.solve(xd.data_ptr(), rel_tol=1e-8, max_its=5000, precond=precond, mixed=True)
        overflows = bool(np.any(np.abs(val) > np.finfo(np.float32).max)) if precond == 0 else False
        _check(s, A, rhs, np.zeros(rhs.size), 1e-8, precond, info, xd.cpu().numpy(), bits=(64,) if overflows else (32,))


def test_fallback_when_an_entry_overflows_fp32():
    """The PIHNA assembly multiplies the spatial operator by the time step, so a LARGE time step (1e40) is what lifts
    assembled values above 3.4e38 while they stay finite in fp64.  Without a preconditioner the copy cannot hold them:
    the mixed solve must say so (matrix_bits 64) and be the fp64 solve, bit for bit."""
    d = synth.pihna_param_dict("shipped")
    d["time_step"] = 1e40
    ctx, s, A, rhs, val = _open("pihna_kuhn", pihna_params_from_dict(d))
    assert np.all(np.isfinite(val)) and np.abs(val).max() > 3.4e38
    with ctx:
        xa, xb = _dev(np.zeros(rhs.size)), _dev(np.zeros(rhs.size))
        ia = ctx.solve(xa.data_ptr(), rel_tol=1e-8, max_its=40, precond=PRECOND_NONE, mixed=False)
        ib = ctx.solve(xb.data_ptr(), rel_tol=1e-8, max_its=40, precond=PRECOND_NONE, mixed=True)
        print(ia, ib)
        assert ia.matrix_bits == 64 and ib.matrix_bits == 64
        assert (ia.reason, ia.iterations, ia.restarts) == (ib.reason, ib.iterations, ib.restarts) and ia.iterations > 0
        assert xa.cpu().numpy().tobytes() == xb.cpu().numpy().tobytes()
        assert ia.residual_norm == ib.residual_norm
        with pytest.raises(RdcError, match="fp32") as ei:
            ctx.csr_scale_f32(PRECOND_NONE)
        assert ei.value.code == 1
        with pytest.raises(RdcError) as ei:               # a refused copy is no copy
            ctx.csr_matvec_f32(np.zeros(A.shape[1]))
        assert ei.value.code == 1
        _unchanged(ctx, val, rhs)


def test_outcomes():
    import torch
    ctx, s, A, rhs, val = _open("ripf_tet_dt01")
    with ctx:                                              # no convergence: said so, x finite
        xd = _dev(np.zeros(rhs.size))
        info = ctx.solve(xd.data_ptr(), rel_tol=1e-8, max_its=300, mixed=True)
        x = xd.cpu().numpy()
    M, _, cond = solve_ref.precond_inverse(A, 3, 2)
    true = float(np.linalg.norm(M @ (rhs - A @ x)))
    rho = 4.0 * solve_ref.longest_row(A) * EPS * np.linalg.norm(abs(M) @ (abs(A) @ np.abs(x) + np.abs(rhs)))
    print(info, true)
    assert info.reason == SOLVE_MAX_ITS and info.iterations == 300 and np.all(np.isfinite(x)) and info.matrix_bits == 32
    assert abs(info.residual_norm - true) <= rho + 64.0 * EPS * cond * true
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:                                              # ghosts: scale + matvec fine (test_matvec_f32), solve refused
        xd = _dev(np.zeros(rhs.size))
        with pytest.raises(RdcError, match="ghost") as ei:
            ctx.solve(xd.data_ptr(), mixed=True)
        assert ei.value.code == 4
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    with ctx:
        # the fp64 solve reports 64
        xd = _dev(np.zeros(n))
        assert ctx.solve(xd.data_ptr(), rel_tol=1e-8, max_its=2000).matrix_bits == 64
        # a non-default stream gives the same iteration count and the same x
        xa = _dev(np.zeros(n))
        ia = ctx.solve(xa.data_ptr(), rel_tol=1e-8, max_its=2000, mixed=True)
        stream = torch.cuda.Stream()
        xb = _dev(np.zeros(n))
        torch.cuda.synchronize()
        ctx.set_stream(stream.cuda_stream)
        ib = ctx.solve(xb.data_ptr(), rel_tol=1e-8, max_its=2000, mixed=True)
        ctx.synchronize()
        ctx.set_stream(0)
        assert ia.reason == ib.reason == SOLVE_CONVERGED and ia.iterations == ib.iterations
        assert xa.cpu().numpy().tobytes() == xb.cpu().numpy().tobytes()
        # b = 0: x = 0 in 0 iterations whatever the start
        _, rptr = ctx.csr_values_device_ptr()

        class _V:
            pass
        v = _V()
        v.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (rptr, False), "version": 2, "strides": None}
        rhs_d = torch.as_tensor(v, device="cuda:0")
        keep = rhs_d.clone()
        rhs_d.zero_()
        xd = _dev(np.ones(n))
        info = ctx.solve(xd.data_ptr(), rel_tol=1e-8, max_its=2000, mixed=True)
        assert info.reason == SOLVE_CONVERGED and info.iterations == 0 and not xd.cpu().numpy().any()
        rhs_d.copy_(keep)
        torch.cuda.synchronize()
        _unchanged(ctx, val, rhs)


def test_time_loop_mixed(oracle):
    """Three steps of assemble -> solve(mixed, 1e-10, in place in FIELD_OLD_SOLUTION) -> clamp on K(8); every step is judged
    on its own inputs, as test_gpu_solve.test_time_loop does for the fp64 solve."""
    import time_loop
    s = solve_systems.get("pihna_kuhn")
    seen = {}

    def on_step(k, phase, ctx):
        if phase == "assembled":
            seen["before"] = ctx.field_download(FIELD_OLD_SOLUTION, ctx.n_node * 5)
        else:
            seen["solved"] = ctx.field_download(FIELD_OLD_SOLUTION, ctx.n_node * 5)

    with AssemblyContext(0) as ctx:
        s.upload(ctx)
        for k in range(3):
            rec = time_loop.run(ctx, s.conn, s.params, 1, rel_tol=1e-10, max_its=2000, on_step=on_step, mixed=True)[0]
            assert rec["reason"] == SOLVE_CONVERGED and rec["matrix_bits"] == 32
            rp, col, val0, rhs0 = s.oracle_assemble(oracle, u_old=seen["before"].reshape(-1, 5))
            A0 = sps.csr_matrix((val0, col, rp), shape=(rhs0.size, rhs0.size))
            f = solve_ref.check_solution(A0, rhs0, seen["solved"], 5, 2, 1e-10, extra_rel=1e-10)
            after = ctx.field_download(FIELD_OLD_SOLUTION, ctx.n_node * 5)
            assert after.tobytes() == np.maximum(seen["solved"], 0.0).tobytes()
            print(f"step {k + 1}: {rec['iterations']} iterations, {rec['restarts']} restarts, residual {f['residual_norm']:.3e} <= {f['bound']:.3e}")
