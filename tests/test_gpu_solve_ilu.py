"""RDC_PRECOND_ILU0 through the C-ABI (rdc_solve with precond = 4; rdc_solve_ilu_apply, rdc_solve_ilu_download, rdc_solve_ilu_stats):
every case assembles on the GPU, downloads values, rhs and pattern once and is judged on the host against tests/solve_ref_ilu.py
(the same algorithm in numpy) built from the DOWNLOADED system.

Factor and apply: against the extended-precision factor / apply; bound = MARGIN x max(noise, 16 eps) relative to the reference in
the 2-norm and in the max norm, noise = what numpy's FP64 evaluation of the same thing differs from the reference by on the same
system (and inputs) -- measured on the reference, never on the device result.  MARGIN = 64, the margin tests/test_gpu_mg_cycle.py
allows a cycle: the device adds a row in another order (16 lanes, then a butterfly), contracts to fma and inverts blocks by
Gauss-Jordan.  The numpy noise per system is in DESIGN.md 7.4 (1e-16 .. 6e-10: the hydrogel blocks have condition numbers up to 2e13).

Solve: reason, the residual inequality of the block-Jacobi solve (solve_ref.check_solution with precond = 2: M comes from the right),
iterations <= yardstick + 2 (the slack of tests/test_gpu_solve_mg_gs.py: a count may move by an iteration or two at the threshold).

Shapes: K(8) nvar 5, 15-block rows; HEX8 nvar 3, 27-block rows, 15 colours; the solid cube with rhs_scale -1; the hydrogel mesh with
irregular rows of 30 - 60 blocks; the hub mesh with one row of 740 blocks (about 148 KB: the factorisation works on it in global
memory)."""
import ctypes as C

import numpy as np
import pytest

import solve_ref
import solve_ref_ilu
import solve_ref_mg_ld as ld
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import RdcError, SolveInfo, SolveParams, partition
from rdcfes_amd.context import (ERR_STATE, ERR_UNSUPPORTED, PRECOND_BLOCK_JACOBI, PRECOND_ILU0, PRECOND_MULTIGRID, SOLVE_BAD_DIAGONAL,
                                SOLVE_CONVERGED, SOLVE_MAX_ITS)

pytestmark = pytest.mark.gpu
FIVE = ["pihna_kuhn", "hcc_hex", "solid_cube", "pihna_hydrogel", "pihna_hub"]
MARGIN, SLACK = 64.0, 2
EPS = ld.EPS
_REF = {}


class _Ref:
    """the FP64 and the extended-precision yardstick factor of one downloaded system, and the yardstick solves, each built once"""

    def __init__(self, A, b, nv):
        self.A, self.b, self.nv = A, b, nv
        self.f = solve_ref_ilu.Factor(A, nv)
        self.fl = solve_ref_ilu.Factor(A, nv, dtype=np.longdouble)
        assert self.f.singular == 0 and self.fl.singular == 0
        self._solves = {}

    def solve(self, rel_tol):
        if rel_tol not in self._solves:
            self._solves[rel_tol] = solve_ref_ilu.bicgstab(self.A, self.b, np.zeros(self.b.size), rel_tol, nv=self.nv, max_its=2000, factor=self.f)[1]
        return self._solves[rel_tol]


def _ref(name, A, b, nv, val):
    """the reference of the values THIS context assembled (two contexts differ in the last bits: the assembly adds with atomics)"""
    if name not in _REF or _REF[name][0] != val.tobytes():
        _REF[name] = (val.tobytes(), _Ref(A, b, nv))
    return _REF[name][1]


def _solve(ctx, n, **kw):
    xd = _dev(np.zeros(n))
    info = ctx.solve(xd.data_ptr(), max_its=2000, **kw)
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


@pytest.mark.parametrize("name", FIVE)
def test_factor_against_reference(name):
    ctx, s, A, rhs, val = _open(name)
    R = _ref(name, A, s.rhs_scale * rhs, s.nv, val)
    want, want_u = R.fl.values(), R.fl.Uinv.reshape(-1)
    noise = max(ld.rel_diff(R.f.values(), want))
    noise_u = max(ld.rel_diff(R.f.Uinv.reshape(-1), want_u))
    with ctx:
        _raises(ERR_STATE, ctx.ilu_stats)
        _raises(ERR_STATE, ctx.ilu_factor)
        ctx.ilu_apply(np.ones(rhs.size))
        got, got_u = ctx.ilu_factor()
        ms, nbytes, colours = ctx.ilu_stats()
        _unchanged(ctx, val, rhs)
    err, err_u = max(ld.rel_diff(got, want)), max(ld.rel_diff(got_u.reshape(-1), want_u))
    print(f"{name}: factor error {err:.2e} = {err / max(noise, 16 * EPS):.2f} x max(noise {noise:.2e}, 16 eps); U_ii^-1 error {err_u:.2e} = "
          f"{err_u / max(noise_u, 16 * EPS):.2f} x max(noise {noise_u:.2e}, 16 eps); {colours} colours, {nbytes} bytes, set-up {ms:.3f} ms")
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(got_u))
    assert err <= ld.bound(MARGIN, noise), (err, noise)
    assert err_u <= ld.bound(MARGIN, noise_u), (err_u, noise_u)
    assert colours == int(R.f.colour.max()) + 1
    nnz, nblk, n = val.size, val.size // s.nv ** 2, rhs.size // s.nv
    assert 8 * nnz + 4 * nblk <= nbytes <= 8 * (nnz + n * s.nv ** 2 + 2 * rhs.size) + 4 * (nblk + 3 * n) + 8 * 256


@pytest.mark.parametrize("name", FIVE)
def test_apply_against_reference(name):
    ctx, s, A, rhs, val = _open(name)
    R = _ref(name, A, s.rhs_scale * rhs, s.nv, val)
    inputs = ld.probe_vectors(rhs.size, s.rhs_scale * rhs)
    if name == "pihna_hub":                          # the node that owns the row of 740 blocks
        hub = int(np.argmax(np.diff(R.f.bptr)))
        assert R.f.bptr[hub + 1] - R.f.bptr[hub] >= 740
        unit = np.zeros(rhs.size)
        unit[hub * s.nv] = 1.0
        inputs.append(unit)
    zs = [R.fl.apply(v) for v in inputs]
    noise = max(max(ld.rel_diff(R.f.apply(v), z)) for v, z in zip(inputs, zs))
    with ctx:
        got = [ctx.ilu_apply(v) for v in inputs]
        again = ctx.ilu_apply(inputs[0])
        _unchanged(ctx, val, rhs)
    err = max(max(ld.rel_diff(g, z)) for g, z in zip(got, zs))
    print(f"{name}: apply error {err:.2e} = {err / max(noise, 16 * EPS):.2f} x max(noise {noise:.2e}, 16 eps)")
    assert err <= ld.bound(MARGIN, noise), (err, noise)
    assert again.tobytes() == got[0].tobytes()


@pytest.mark.parametrize("name", FIVE)
def test_solve(name):
    ctx, s, A, rhs, val = _open(name)
    b = s.rhs_scale * rhs
    R = _ref(name, A, b, s.nv, val)
    with ctx:
        for rel_tol in (1e-8, 1e-10):
            info, x = _solve(ctx, rhs.size, rel_tol=rel_tol, precond=PRECOND_ILU0, rhs_scale=s.rhs_scale)
            ref = R.solve(rel_tol)
            ms, nbytes, colours = ctx.ilu_stats()
            print(f"{name} tol {rel_tol:g}: iterations GPU {info.iterations} (restarts {info.restarts}), yardstick {ref['iterations']}; "
                  f"{colours} colours; {info.device_ms:.2f} ms, of which set-up {ms:.2f}")
            assert info.reason == SOLVE_CONVERGED and ref["reason"] == solve_ref_ilu.CONVERGED, (info, ref)
            f = solve_ref.check_solution(A, b, x, s.nv, 2, rel_tol)
            assert abs(info.residual_norm - f["residual_norm"]) <= f["rho"], (info, f)
            assert info.iterations <= ref["iterations"] + SLACK, (info.iterations, ref)
            assert info.matrix_bits == 64 and info.bad_blocks == 0
            assert colours == ref["colours"]
        _unchanged(ctx, val, rhs)


@pytest.mark.parametrize("name", ["pihna_hydrogel", "hcc_hex"])
def test_two_solves_are_bitwise_equal(name):
    ctx, s, A, rhs, val = _open(name)
    kw = dict(rel_tol=1e-10, precond=PRECOND_ILU0, rhs_scale=s.rhs_scale)
    with ctx:
        ia, xa = _solve(ctx, rhs.size, **kw)
        fa = ctx.ilu_factor()
        ib, xb = _solve(ctx, rhs.size, **kw)
        fb = ctx.ilu_factor()
    assert ia.reason == SOLVE_CONVERGED
    assert _same(ia, ib) and xa.tobytes() == xb.tobytes(), "two solves differ"
    assert fa[0].tobytes() == fb[0].tobytes() and fa[1].tobytes() == fb[1].tobytes(), "two factorisations differ"


def test_existing_paths_are_undisturbed():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        j0, x0 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)
        m0, y0 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        levels, nbytes = ctx.mg_levels(), ctx.mg_stats()[1]
        i0, z0 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_ILU0)
        j1, x1 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_BLOCK_JACOBI)
        m1, y1 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_MULTIGRID)
        i1, z1 = _solve(ctx, rhs.size, rel_tol=1e-10, precond=PRECOND_ILU0)
        assert j0.reason == m0.reason == i0.reason == SOLVE_CONVERGED
        assert i0.iterations < j0.iterations
        assert _same(j0, j1) and x0.tobytes() == x1.tobytes(), "an ILU solve changed what the block-Jacobi solve returns"
        assert _same(m0, m1) and y0.tobytes() == y1.tobytes(), "an ILU solve changed what the multigrid solve returns"
        assert _same(i0, i1) and z0.tobytes() == z1.tobytes()
        assert z0.tobytes() != x0.tobytes()
        assert ctx.mg_levels() == levels and ctx.mg_stats()[1] == nbytes
        _unchanged(ctx, val, rhs)


def test_ghosted_context_is_refused():
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        x0 = np.random.default_rng(3).uniform(size=ctx.n_node * s.nv)
        xd = _dev(x0)
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_ILU0), match="ghost")
        yd = _dev(x0[:rhs.size])
        _raises(ERR_UNSUPPORTED, lambda: ctx.ilu_apply_device(yd.data_ptr(), xd.data_ptr()), match="ghost")
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        _raises(ERR_STATE, ctx.ilu_stats)


def test_mixed_and_partitioned_entries_refuse_the_value():
    from rdcfes_amd import SolveComm
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        x0 = np.random.default_rng(5).uniform(size=rhs.size)
        xd = _dev(x0)
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_ILU0, mixed=True), match="rdc_solve_mixed")
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        lp = partition.build_local(s.conn, s.xyz, np.zeros(s.conn.shape[0], dtype=np.int32), 0, 1)
        for sized in (False, True):
            comm = SolveComm(lp, s.nv, "cuda:0", sized=sized)
            for mixed in (False, True):
                _raises(ERR_UNSUPPORTED, lambda: ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-8, precond=PRECOND_ILU0, mixed=mixed), match="partitions")
            if sized:                                        # the wrapper sends only multigrid to rdc_solve_dist_mg: call it directly
                p, info = SolveParams(1e-8, 0.0, 1.0, 100, PRECOND_ILU0), SolveInfo()
                rc = ctx._lib.rdc_solve_dist_mg(ctx._h, C.byref(p), C.byref(comm.sized_struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info))
                assert rc == ERR_UNSUPPORTED
            assert (comm.exchanges, comm.allreduces) == (0, 0)
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        _raises(ERR_STATE, ctx.ilu_stats)                    # nothing was built
        info, x = _solve(ctx, rhs.size, rel_tol=1e-8, precond=PRECOND_ILU0)    # and rdc_solve takes it
        assert info.reason == SOLVE_CONVERGED


def test_zeroed_diagonal_block_is_reported():
    import torch
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    n = rhs.size
    with ctx:
        val_d = _values_tensor(ctx, val.size)
        rp, col = ctx.csr_pattern()
        node = 11
        idx = np.concatenate([np.arange(rp[node * 5 + a], rp[node * 5 + a + 1])[col[rp[node * 5 + a]:rp[node * 5 + a + 1]] // 5 == node]
                              for a in range(5)])
        assert idx.size == 25
        keep = val_d.clone()
        val_d[torch.from_numpy(idx).to("cuda:0")] = 0.0
        x0 = np.random.default_rng(2).uniform(size=n)
        xd = _dev(x0)
        info = ctx.solve(xd.data_ptr(), rel_tol=1e-10, max_its=2000, precond=PRECOND_ILU0)
        assert info.reason == SOLVE_BAD_DIAGONAL and info.bad_blocks >= 1 and info.iterations == 0
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        val_d.copy_(keep)
        torch.cuda.synchronize()
        info, x = _solve(ctx, n, rel_tol=1e-10, precond=PRECOND_ILU0)
        assert info.reason == SOLVE_CONVERGED and info.bad_blocks == 0
        solve_ref.check_solution(A, rhs, x, 5, 2, 1e-10)


def test_a_solve_that_does_not_converge_says_so():
    """ripf_tet_dt01 (Courant 900, indefinite): ILU(0) does not fix it; the residual reported is the true one of the x returned"""
    ctx, s, A, rhs, val = _open("ripf_tet_dt01")
    with ctx:
        xd = _dev(np.zeros(rhs.size))
        info = ctx.solve(xd.data_ptr(), rel_tol=1e-8, max_its=300, precond=PRECOND_ILU0)
        x = xd.cpu().numpy()
    print(f"ripf_tet_dt01: reason {info.reason}, {info.iterations} iterations, residual {info.residual_norm:.3e} of {info.rhs_norm:.3e}")
    assert info.reason == SOLVE_MAX_ITS and info.iterations == 300 and np.all(np.isfinite(x))
    M, _, _ = solve_ref.precond_inverse(A, s.nv, 2)
    rn = float(np.linalg.norm(M @ (rhs - A @ x)))
    rho = 4.0 * solve_ref.longest_row(A) * solve_ref.EPS * float(np.linalg.norm(abs(M) @ (abs(A) @ np.abs(x) + np.abs(rhs))))
    assert abs(info.residual_norm - rn) <= rho, (info.residual_norm, rn, rho)
    assert info.residual_norm > 1e-8 * info.rhs_norm
