"""Restarted GMRES(m) through the C-ABI (rdc_solve / rdc_solve_mixed with the option "solve_method" = 1; rdc_solve_gmres_arnoldi,
rdc_solve_gmres_stats): every case assembles on the GPU, downloads values, rhs and pattern once and is judged on the host against
tests/solve_ref_gmres.py (the same algorithm in numpy) built from the DOWNLOADED system.

Arnoldi (the hook): 12 steps from the rhs and from a random vector, one and two Gram-Schmidt passes, precond 2, 3 and 4, judged in
extended precision -- the relation ||Op v_j - V H[:, j]|| / ||Op v_j|| for every j, max |V^T V - I|, and H itself against the
extended-precision Arnoldi process.  Bound = MARGIN x max(noise, 16 eps), MARGIN = 64 (that of tests/test_gpu_mg_cycle.py and
tests/test_gpu_solve_ilu.py); noise = the same figure of numpy's FP64 run of the same algorithm (for the orthogonality: numpy's own
loss of orthogonality), measured on the reference, never on the device result.

Solve: reason, the residual inequality of the block-Jacobi solve (solve_ref.check_solution with precond = 2: M comes from the
right), iterations <= yardstick + 2 (the slack of the ILU and Gauss-Seidel tests: a count may move by a step at the threshold),
restarts <= yardstick + 1.

Shapes: ripf_tet, 1029 entries = one full 1024-entry workgroup of the vector kernels and a 5-entry tail, nvar 3; K(8), nvar 5, 3645
entries; HEX8, rows of 27 blocks; the hub mesh with its row of 740 blocks; the solid cube with rhs_scale -1; the hydrogel mesh for
the restarts."""
import ctypes as C

import numpy as np
import pytest

import solve_ref
import solve_ref_gmres
import solve_ref_ilu
import solve_ref_ilu_f32
import solve_ref_mg
import solve_ref_mg_ld as ld
import solve_ref_mixed
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import RdcError, SolveComm, SolveInfo, SolveParams, partition
from rdcfes_amd.context import (ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED, PRECOND_BLOCK_JACOBI, PRECOND_ILU0, PRECOND_MULTIGRID,
                                SOLVE_BAD_DIAGONAL, SOLVE_CONVERGED, SOLVE_MAX_ITS, SOLVE_NOT_FINITE)

pytestmark = pytest.mark.gpu
FOUR = ["ripf_tet", "pihna_kuhn", "hcc_hex", "pihna_hub"]
MARGIN, SLACK = 64.0, 2
EPS, LD = ld.EPS, np.longdouble
STEPS = 12
_REF = {}


class _Ref:
    """the yardsticks of one downloaded system, each built once: numpy's right preconditioners and their extended-precision forms"""

    def __init__(self, A, b, nv):
        self.A, self.b, self.nv = A, b, nv
        self.M = solve_ref.precond_inverse(A, nv, 2)[0]
        self._right, self._right_ld, self._op_ld, self._solves, self._a32 = {}, {}, None, {}, None

    def hierarchy(self):
        if "H" not in self._right:
            self._right["H"] = solve_ref_mg.Hierarchy(self.A, self.nv)
        return self._right["H"]

    def factor(self):
        if "F" not in self._right:
            self._right["F"] = solve_ref_ilu.Factor(self.A, self.nv)
            assert self._right["F"].singular == 0
        return self._right["F"]

    def right(self, precond):
        return {PRECOND_MULTIGRID: lambda: self.hierarchy().cycle, PRECOND_ILU0: lambda: self.factor().apply}.get(precond, lambda: None)()

    def op(self, precond):
        """v -> D^-1 A (M v) as numpy's FP64 solve applies it"""
        right = self.right(precond)
        return lambda v: self.M @ (self.A @ (right(v) if right else v))

    def op_ld(self, precond):
        """the same in extended precision"""
        if self._op_ld is None:
            bptr, bcol, a = solve_ref_mg.block_pattern(self.A, self.nv)
            rows = np.repeat(np.arange(bptr.size - 1), np.diff(bptr))
            self._op_ld = ld.Op.of_blocks(bptr, bcol, ld.newton_inverse(ld.diag_of(bptr, bcol, a))[rows] @ a.astype(LD))
        if precond not in self._right_ld:
            self._right_ld[precond] = {PRECOND_MULTIGRID: lambda: ld.Cycle(self.hierarchy(), self.A).cycle,
                                       PRECOND_ILU0: lambda: solve_ref_ilu.Factor(self.A, self.nv, dtype=LD).apply}.get(precond, lambda: None)()
        right = self._right_ld[precond]
        return lambda v: self._op_ld @ (right(v) if right else np.asarray(v, dtype=LD))

    def a32(self):
        if self._a32 is None:
            self._a32 = solve_ref_mixed.scaled_f32(self.A, self.nv, 2)
        return self._a32

    def solve(self, precond, rel_tol, restart=30, max_its=2000, refine=False):
        key = (precond, rel_tol, restart, max_its, refine)
        if key not in self._solves:
            self._solves[key] = solve_ref_gmres.gmres(self.A, self.b, np.zeros(self.b.size), rel_tol, max_its=max_its, precond=2, nv=self.nv,
                                                      right=self.right(precond), restart=restart, refine=refine)[1]
        return self._solves[key]


def _ref(name, A, b, nv, val):
    """the reference of the values THIS context assembled (two contexts differ in the last bits: the assembly adds with atomics)"""
    if name not in _REF or _REF[name][0] != val.tobytes():
        _REF[name] = (val.tobytes(), _Ref(A, b, nv))
    return _REF[name][1]


def _gmres(ctx, restart=30, refine=0):
    ctx.set_option("solve_method", 1)
    ctx.set_option("gmres_restart", restart)
    ctx.set_option("gmres_refine", refine)


def _solve(ctx, n, x0=None, max_its=2000, **kw):
    xd = _dev(np.zeros(n) if x0 is None else x0)
    info = ctx.solve(xd.data_ptr(), max_its=max_its, **kw)
    return info, xd.cpu().numpy()


def _same(a, b):
    return (a.reason, a.iterations, a.restarts, a.residual_norm, a.bad_blocks) == (b.reason, b.iterations, b.restarts, b.residual_norm, b.bad_blocks)


def _raises(code, fn, match=None):
    with pytest.raises(RdcError, match=match) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return ei.value


def _values_tensor(ctx, size):
    """the CSR values of a context as a device tensor (no copy)"""
    import torch
    vptr, _ = ctx.csr_values_device_ptr()

    class _V:
        pass
    view = _V()
    view.__cuda_array_interface__ = {"shape": (size,), "typestr": "<f8", "data": (vptr, False), "version": 2, "strides": None}
    return torch.as_tensor(view, device="cuda:0")


def _rhs_tensor(ctx, size):
    import torch
    _, rptr = ctx.csr_values_device_ptr()

    class _V:
        pass
    view = _V()
    view.__cuda_array_interface__ = {"shape": (size,), "typestr": "<f8", "data": (rptr, False), "version": 2, "strides": None}
    return torch.as_tensor(view, device="cuda:0")


def _true_residual(A, b, x, nv):
    M, _, _ = solve_ref.precond_inverse(A, nv, 2)
    rn = float(np.linalg.norm(M @ (b - A @ x)))
    rho = 4.0 * solve_ref.longest_row(A) * solve_ref.EPS * float(np.linalg.norm(abs(M) @ (abs(A) @ np.abs(x) + np.abs(b))))
    return rn, rho


# ---- the Arnoldi process held to a reference ----

def _figures(op_ld, V, H):
    """(largest relative defect of the Arnoldi relation over the columns, max |V^T V - I|) of a basis V [k + 1][n] and a raw
    Hessenberg matrix H [>= k + 1][>= k], evaluated in extended precision"""
    k = V.shape[0] - 1
    Vl = np.asarray(V, dtype=LD)
    rel = 0.0
    for j in range(k):
        w = op_ld(Vl[j])
        d = w - np.asarray(H[:k + 1, j], dtype=LD) @ Vl
        rel = max(rel, float(np.sqrt(d @ d) / np.sqrt(w @ w)))
    return rel, float(np.abs(Vl @ Vl.T - np.eye(k + 1, dtype=LD)).max())


@pytest.mark.parametrize("precond", [PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, PRECOND_ILU0])
@pytest.mark.parametrize("name", FOUR)
def test_arnoldi_against_reference(name, precond):
    ctx, s, A, rhs, val = _open(name)
    b = s.rhs_scale * rhs
    R = _ref(name, A, b, s.nv, val)
    op, op_ld = R.op(precond), R.op_ld(precond)
    starts = {"rhs": b, "random": np.random.default_rng(21).standard_normal(b.size)}
    with ctx:
        ctx.set_option("gmres_restart", STEPS)
        for refine in (0, 1):
            ctx.set_option("gmres_refine", refine)
            for label, v0 in starts.items():
                Vl, Hl, done_l = solve_ref_gmres.arnoldi(op_ld, v0, STEPS, refine=bool(refine), dtype=LD)
                Vn, Hn, done_n = solve_ref_gmres.arnoldi(op, v0, STEPS, refine=bool(refine))
                assert done_l == done_n == STEPS
                noise_rel, noise_orth = _figures(op_ld, Vn, Hn)
                scale = float(np.abs(Hl).max())
                noise_h = float(np.abs(Hn.astype(LD) - Hl).max()) / scale
                V, H = ctx.gmres_arnoldi(v0, STEPS, precond)
                V2, H2 = ctx.gmres_arnoldi(v0, STEPS, precond)
                assert V.shape == (STEPS + 1, b.size) and H.shape == (STEPS + 1, STEPS)
                assert np.all(np.isfinite(V)) and np.all(np.isfinite(H))
                assert np.all(np.tril(H, -2) == 0.0), "entries below the subdiagonal were written"
                rel, orth = _figures(op_ld, V, H)
                err_h = float(np.abs(H.astype(LD) - Hl).max()) / scale
                print(f"{name} precond {precond} refine {refine} v0 {label}: relation {rel:.2e} = {rel / max(noise_rel, 16 * EPS):.2f} x max(noise "
                      f"{noise_rel:.2e}, 16 eps); orthogonality {orth:.2e} = {orth / max(noise_orth, 16 * EPS):.2f} x max(noise {noise_orth:.2e}, 16 eps); "
                      f"H {err_h:.2e} = {err_h / max(noise_h, 16 * EPS):.2f} x max(noise {noise_h:.2e}, 16 eps)")
                assert rel <= ld.bound(MARGIN, noise_rel), (rel, noise_rel)
                assert orth <= ld.bound(MARGIN, noise_orth), (orth, noise_orth)
                assert err_h <= ld.bound(MARGIN, noise_h), (err_h, noise_h)
                assert V2.tobytes() == V.tobytes() and H2.tobytes() == H.tobytes(), "a second call returns other bytes"
        _unchanged(ctx, val, rhs)


# ---- the solve ----

CASES = [(n, p, 30) for n in ("pihna_kuhn", "hcc_hex", "ripf_tet", "pihna_hub") for p in (PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, PRECOND_ILU0)] + \
        [("solid_cube", PRECOND_BLOCK_JACOBI, 30), ("pihna_hydrogel", PRECOND_MULTIGRID, 30), ("pihna_hydrogel", PRECOND_ILU0, 60)]


@pytest.mark.parametrize("name,precond,restart", CASES)
def test_solve(name, precond, restart):
    ctx, s, A, rhs, val = _open(name)
    b = s.rhs_scale * rhs
    R = _ref(name, A, b, s.nv, val)
    with ctx:
        _gmres(ctx, restart)
        for rel_tol in (1e-8, 1e-10):
            info, x = _solve(ctx, rhs.size, rel_tol=rel_tol, precond=precond, rhs_scale=s.rhs_scale)
            ref = R.solve(precond, rel_tol, restart)
            m, nbytes, cycles = ctx.gmres_stats()
            print(f"{name} precond {precond} restart {restart} tol {rel_tol:g}: steps GPU {info.iterations} (restarts {info.restarts}), yardstick "
                  f"{ref['iterations']} (restarts {ref['restarts']}); {info.device_ms:.2f} ms")
            assert info.reason == SOLVE_CONVERGED and ref["reason"] == solve_ref_gmres.CONVERGED, (info, ref)
            f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
            assert abs(info.residual_norm - f["residual_norm"]) <= f["rho"], (info, f)
            assert info.iterations <= ref["iterations"] + SLACK, (info.iterations, ref)
            assert info.restarts <= ref["restarts"] + 1, (info.restarts, ref)
            assert info.matrix_bits == 64 and info.bad_blocks == 0
            assert (m, nbytes, cycles) == (restart, (restart + 1) * rhs.size * 8, info.restarts + 1)
            assert info.restarts >= (info.iterations - 1) // restart
        _unchanged(ctx, val, rhs)


def test_cycle_bookkeeping():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    R = _ref("pihna_kuhn", A, rhs, s.nv, val)
    n = rhs.size
    with ctx:
        _gmres(ctx, 1)                                   # GMRES(1): every step is a cycle
        info, x = _solve(ctx, n, rel_tol=1e-8, precond=PRECOND_ILU0)
        ref = R.solve(PRECOND_ILU0, 1e-8, 1)
        print(f"restart 1: {info.iterations} steps, {info.restarts} restarts; yardstick {ref['iterations']}, {ref['restarts']}")
        assert info.reason == SOLVE_CONVERGED and ref["reason"] == solve_ref_gmres.CONVERGED
        assert info.restarts == info.iterations - 1 and info.iterations <= ref["iterations"] + SLACK
        assert ctx.gmres_stats() == (1, 2 * n * 8, info.iterations)
        solve_ref.check_solution(A, rhs, x, s.nv, 2, 1e-8)
        _gmres(ctx, 128)                                 # a restart longer than the solve: one cycle
        info, x = _solve(ctx, n, rel_tol=1e-8, precond=PRECOND_BLOCK_JACOBI)
        ref = R.solve(PRECOND_BLOCK_JACOBI, 1e-8, 128)
        print(f"restart 128: {info.iterations} steps, {info.restarts} restarts; yardstick {ref['iterations']}")
        assert info.reason == SOLVE_CONVERGED and info.restarts == 0 and ref["restarts"] == 0
        assert info.iterations <= ref["iterations"] + SLACK
        assert ctx.gmres_stats() == (128, 129 * n * 8, 1)
        solve_ref.check_solution(A, rhs, x, s.nv, 2, 1e-8)
        _gmres(ctx, 5)                                   # max_its inside the second cycle
        info, x = _solve(ctx, n, max_its=7, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)
        rn, rho = _true_residual(A, rhs, x, s.nv)
        assert info.reason == SOLVE_MAX_ITS and info.iterations == 7 and info.restarts == 1 and np.all(np.isfinite(x))
        assert abs(info.residual_norm - rn) <= rho, (info.residual_norm, rn, rho)
        assert info.residual_norm > 1e-10 * info.rhs_norm
        _unchanged(ctx, val, rhs)


def test_hydrogel_block_jacobi_does_not_converge_and_says_so():
    """GMRES(30) stagnates on block Jacobi's system of the hydrogel mesh (tests/test_solve_ref_gmres.py has the CPU record)"""
    ctx, s, A, rhs, val = _open("pihna_hydrogel")
    with ctx:
        _gmres(ctx, 30)
        info, x = _solve(ctx, rhs.size, max_its=300, rel_tol=1e-8, precond=PRECOND_BLOCK_JACOBI)
    rn, rho = _true_residual(A, rhs, x, s.nv)
    print(f"hydrogel precond 2 restart 30: reason {info.reason}, {info.iterations} steps, {info.restarts} restarts, residual "
          f"{info.residual_norm / info.rhs_norm:.2e} relative")
    assert info.reason == SOLVE_MAX_ITS and info.iterations == 300 and info.restarts == 9 and np.all(np.isfinite(x))
    assert abs(info.residual_norm - rn) <= rho, (info.residual_norm, rn, rho)
    assert info.residual_norm > 1e-8 * info.rhs_norm


def test_krylov_space_exhausted_in_one_step():
    """every off-diagonal block zeroed: D^-1 A = I, the first Arnoldi step leaves (next to) nothing, and x = D^-1 b"""
    import torch
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    with ctx:
        _gmres(ctx, 30)
        val_d = _values_tensor(ctx, val.size)
        rp, col = ctx.csr_pattern()
        rows = np.repeat(np.arange(n), np.diff(rp))
        off = np.flatnonzero(col // 5 != rows // 5)
        keep = val_d.clone()
        val_d[torch.from_numpy(off).to("cuda:0")] = 0.0
        torch.cuda.synchronize()
        info, x = _solve(ctx, n, rel_tol=1e-8, precond=PRECOND_BLOCK_JACOBI)
        val_d.copy_(keep)
        torch.cuda.synchronize()
        _unchanged(ctx, val, rhs)
    M, _, cond = solve_ref.precond_inverse(A, 5, 2)     # the diagonal blocks are those of A
    want = M @ rhs
    assert info.reason == SOLVE_CONVERGED and info.iterations == 1 and info.restarts == 0, info
    assert np.all(np.isfinite(x))
    assert np.linalg.norm(x - want) <= 64.0 * EPS * cond * np.linalg.norm(want), (np.linalg.norm(x - want), cond)


def test_outcomes_carried_over():
    import torch
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    with ctx:
        _gmres(ctx, 30)
        good = dict(rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)
        val_d, rhs_d = _values_tensor(ctx, val.size), _rhs_tensor(ctx, n)
        keep_val, keep_rhs = val_d.clone(), rhs_d.clone()
        rp, col = ctx.csr_pattern()
        node = 11
        idx = np.concatenate([np.arange(rp[node * 5 + a], rp[node * 5 + a + 1])[col[rp[node * 5 + a]:rp[node * 5 + a + 1]] // 5 == node]
                              for a in range(5)])
        val_d[torch.from_numpy(idx).to("cuda:0")] = 0.0
        x0 = np.random.default_rng(2).uniform(size=n)
        for precond in (PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, PRECOND_ILU0):
            info, x = _solve(ctx, n, x0=x0, rel_tol=1e-10, precond=precond)
            assert info.reason == SOLVE_BAD_DIAGONAL and info.bad_blocks >= 1 and info.iterations == 0, (precond, info)
            assert x.tobytes() == x0.tobytes()
        val_d.copy_(keep_val)
        rhs_d.zero_()                                     # b = 0: x = 0 whatever the start
        info, x = _solve(ctx, n, x0=np.ones(n), **good)
        assert info.reason == SOLVE_CONVERGED and info.iterations == 0 and not x.any()
        rhs_d.copy_(keep_rhs)
        rhs_d[7] = float("nan")                           # a non-finite rhs entry: reported, x untouched
        info, x = _solve(ctx, n, x0=x0, **good)
        assert info.reason == SOLVE_NOT_FINITE and info.iterations == 0 and x.tobytes() == x0.tobytes()
        rhs_d.copy_(keep_rhs)
        torch.cuda.synchronize()
        info, x = _solve(ctx, n, **good)
        assert info.reason == SOLVE_CONVERGED
        solve_ref.check_solution(A, rhs, x, 5, 2, 1e-10)
        _unchanged(ctx, val, rhs)


# ---- determinism and isolation ----

@pytest.mark.parametrize("name,precond", [("pihna_hydrogel", PRECOND_MULTIGRID), ("hcc_hex", PRECOND_BLOCK_JACOBI)])
def test_two_solves_are_bitwise_equal(name, precond):
    ctx, s, A, rhs, val = _open(name)
    kw = dict(rel_tol=1e-10, precond=precond, rhs_scale=s.rhs_scale)
    with ctx:
        _gmres(ctx, 30)
        ia, xa = _solve(ctx, rhs.size, **kw)
        ib, xb = _solve(ctx, rhs.size, **kw)
    assert ia.reason == SOLVE_CONVERGED and ia.restarts >= 1
    assert _same(ia, ib) and xa.tobytes() == xb.tobytes(), "two solves differ"


def test_bicgstab_is_undisturbed():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    three = (PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, PRECOND_ILU0)
    with ctx:
        before = [_solve(ctx, n, rel_tol=1e-10, precond=p) for p in three]
        levels, mg_bytes, ilu = ctx.mg_levels(), ctx.mg_stats()[1], ctx.ilu_stats()[1:]
        _raises(ERR_STATE, ctx.gmres_stats)               # no GMRES solve yet
        _gmres(ctx, 30)
        g = [_solve(ctx, n, rel_tol=1e-10, precond=p) for p in three]
        assert ctx.gmres_stats()[0] == 30
        assert ctx.mg_levels() == levels and ctx.mg_stats()[1] == mg_bytes and ctx.ilu_stats()[1:] == ilu
        ctx.set_option("solve_method", 0)
        after = [_solve(ctx, n, rel_tol=1e-10, precond=p) for p in three]
        for (i0, x0), (i1, x1), (ig, xg), p in zip(before, after, g, three):
            assert i0.reason == ig.reason == SOLVE_CONVERGED
            assert _same(i0, i1) and x0.tobytes() == x1.tobytes(), f"a GMRES solve changed what BiCGStab returns with precond {p}"
            assert xg.tobytes() != x0.tobytes() and ig.iterations < 2 * i0.iterations
        assert ctx.gmres_stats()[0] == 30                 # the record of the last GMRES solve stays
        _unchanged(ctx, val, rhs)


# ---- mixed precision ----

@pytest.mark.parametrize("precond", [PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, PRECOND_ILU0])
def test_mixed(precond):
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    R = _ref("pihna_kuhn", A, rhs, s.nv, val)
    A32 = R.a32()
    right = {PRECOND_BLOCK_JACOBI: lambda: None, PRECOND_MULTIGRID: lambda: ld.mixed_hierarchy(R.hierarchy(), A32).cycle,
             PRECOND_ILU0: lambda: solve_ref_ilu_f32.rounded(R.factor()).apply}[precond]()
    with ctx:
        _gmres(ctx, 30)
        if precond == PRECOND_ILU0:
            ctx.set_option("ilu_factor_bits", 32)
        for rel_tol in (1e-8, 1e-10):
            info, x = _solve(ctx, rhs.size, rel_tol=rel_tol, precond=precond, mixed=True)
            ref = solve_ref_gmres.gmres(A, rhs, np.zeros(rhs.size), rel_tol, max_its=2000, precond=2, nv=s.nv, operator=lambda y: A32 @ y,
                                        right=right, restart=30)[1]
            print(f"mixed precond {precond} tol {rel_tol:g}: steps GPU {info.iterations} (restarts {info.restarts}), yardstick {ref['iterations']} "
                  f"(restarts {ref['restarts']})")
            assert info.reason == SOLVE_CONVERGED and ref["reason"] == solve_ref_gmres.CONVERGED and info.matrix_bits == 32
            solve_ref.check_solution(A, rhs, x, s.nv, 2, rel_tol)
            assert info.iterations <= ref["iterations"] + SLACK, (info.iterations, ref)
        if precond == PRECOND_ILU0:
            assert ctx.ilu_factor_bits() == 32
        _unchanged(ctx, val, rhs)


# ---- refusals ----

def test_ghosted_context_is_refused():
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        _gmres(ctx, 30)
        x0 = np.random.default_rng(3).uniform(size=ctx.n_node * s.nv)
        xd = _dev(x0)
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_BLOCK_JACOBI), match="ghost")
        vd = _dev(x0[:rhs.size])
        H = np.zeros((30, 31))
        _raises(ERR_UNSUPPORTED, lambda: ctx.gmres_arnoldi_device(vd.data_ptr(), 3, PRECOND_BLOCK_JACOBI, xd.data_ptr(), H), match="ghost")
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        _raises(ERR_STATE, ctx.gmres_stats)


def test_partitioned_entries_refuse_the_method():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        x0 = np.random.default_rng(5).uniform(size=rhs.size)
        xd = _dev(x0)
        lp = partition.build_local(s.conn, s.xyz, np.zeros(s.conn.shape[0], dtype=np.int32), 0, 1)
        _gmres(ctx, 30)
        for sized in (False, True):
            comm = SolveComm(lp, s.nv, "cuda:0", sized=sized)
            for mixed in (False, True):
                for precond in (PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID) if sized else (PRECOND_BLOCK_JACOBI,):
                    _raises(ERR_UNSUPPORTED, lambda: ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-8, precond=precond, mixed=mixed), match="solve_method")
            if sized:
                p, info = SolveParams(1e-8, 0.0, 1.0, 100, PRECOND_MULTIGRID), SolveInfo()
                rc = ctx._lib.rdc_solve_dist_mg(ctx._h, C.byref(p), C.byref(comm.sized_struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info))
                assert rc == ERR_UNSUPPORTED
            assert (comm.exchanges, comm.allreduces) == (0, 0)
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        _raises(ERR_STATE, ctx.gmres_stats)                # nothing was built
        ctx.set_option("solve_method", 0)                  # and BiCGStab across ranks works as before
        comm = SolveComm(lp, s.nv, "cuda:0")
        info = ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-8, precond=PRECOND_BLOCK_JACOBI)
        assert info.reason == SOLVE_CONVERGED and comm.allreduces > 0
        solve_ref.check_solution(A, rhs, xd.cpu().numpy(), s.nv, 2, 1e-8)


def test_option_values_out_of_range():
    ctx, s, A, rhs, val = _open("ripf_tet")
    R = _ref("ripf_tet", A, rhs, s.nv, val)
    with ctx:
        _gmres(ctx, 7, 1)
        for key, bad in (("solve_method", 2), ("solve_method", -1), ("gmres_restart", 0), ("gmres_restart", 129), ("gmres_refine", 2),
                         ("gmres_refine", -1)):
            _raises(ERR_INVALID, lambda: ctx.set_option(key, bad), match=key)
        v0 = np.ones(rhs.size)
        _raises(ERR_INVALID, lambda: ctx.gmres_arnoldi(v0, 8, PRECOND_BLOCK_JACOBI), match="steps")    # more steps than the restart
        _raises(ERR_INVALID, lambda: ctx.gmres_arnoldi(v0, 0, PRECOND_BLOCK_JACOBI), match="steps")
        _raises(ERR_INVALID, lambda: ctx.gmres_arnoldi(v0, 3, 9), match="preconditioner")
        info, x = _solve(ctx, rhs.size, rel_tol=1e-8, precond=PRECOND_BLOCK_JACOBI)    # the settings are what they were: GMRES(7), two passes
        ref = R.solve(PRECOND_BLOCK_JACOBI, 1e-8, 7, refine=True)
        assert info.reason == SOLVE_CONVERGED and ctx.gmres_stats()[0] == 7
        assert info.iterations <= ref["iterations"] + SLACK and info.restarts <= ref["restarts"] + 1
        solve_ref.check_solution(A, rhs, x, s.nv, 2, 1e-8)
