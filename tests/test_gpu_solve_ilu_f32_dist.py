"""The fp32 copy of the rank-local block ILU(0) factor through the C-ABI (option "ilu_factor_bits" = 32; rdc_solve_dist with
precond = 5 and mixed 0 or 1; rdc_solve_ilu_local_apply):

1. In this process on a ghosted context: one apply of the owned square against the extended-precision sweeps of the FP64 factor the
   device built (rdc_solve_ilu_local_download), rounded by numpy -- reference, bound and margin of tests/test_gpu_solve_ilu_f32.py.
2. World 1: solve_dist(5) returns the bytes of solve(4) at the same value of the option, with either operator.
3. Worlds 2 and 3 (tests/solve_ilu_f32_dist_ranks.py: one process per rank, gloo, all on GPU 0), the option at 32 on every rank:
   the gathered x against the ORACLE's global system, iterations <= the numpy yardstick with every rank's factor rounded
   (tests/solve_ref_ilu_f32.py) + SLACK, identical info on every rank, repeatability, and the callback counts of the FP64 factor: two
   exchanges and three all-reduces per iteration, one of each per true residual -- whether a rank's sweeps stream its fp32 copy is
   that rank's own decision and travels nowhere.  With the fp32 operator as well: converged, matrix_bits 32, and iterations
   <= 2 x that yardstick + 2, the criterion of tests/test_gpu_solve_mixed.py held against the yardstick of the FP64 operator
   (which is never above the yardstick of the fp32 operator on these systems: the bound is the tighter of the two)."""
import numpy as np
import pytest

import solve_ilu_f32_dist_ranks
import solve_ref
import solve_ref_dist
import solve_ref_ilu
import solve_ref_ilu_f32
import solve_ref_mg_ld as ld
from solve_systems import _dev, _open, _unchanged
from test_gpu_solve_ilu_dist import _gather, _same_info, _world1_comm
from rdcfes_amd.context import PRECOND_ILU0, PRECOND_ILU0_LOCAL, SOLVE_CONVERGED

pytestmark = pytest.mark.gpu
MARGIN, SLACK = 64.0, 2          # those of tests/test_gpu_solve_ilu.py
ASSEMBLY_REL = 1e-10             # that of tests/test_gpu_solve_dist.py
EPS = ld.EPS
I = {f: i for i, f in enumerate(solve_ilu_f32_dist_ranks.INFO_FIELDS)}


# ---- 1. one apply of the owned square, in process ----
def test_apply_of_the_owned_square():
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    nv, n = s.nv, rhs.size // s.nv
    assert n < ctx.n_node
    f = solve_ref_ilu.Factor(A[:, :n * nv].tocsr(), nv)
    inputs = ld.probe_vectors(rhs.size, s.rhs_scale * rhs)
    with ctx:
        plain = [ctx.ilu_local_apply(v) for v in inputs]
        assert ctx.ilu_factor_bits() == 64
        bytes64 = ctx.ilu_stats()[1]
        ctx.set_option("ilu_factor_bits", 32)
        got = [ctx.ilu_local_apply(v) for v in inputs]
        again = ctx.ilu_local_apply(inputs[0])
        assert ctx.ilu_factor_bits() == 32
        fval, fuinv = ctx.ilu_local_factor()
        bytes32 = ctx.ilu_stats()[1]
        _unchanged(ctx, val, rhs)
    assert fval.size == f.F.size
    gl = solve_ref_ilu_f32.rounded(f, dtype=np.longdouble, val=fval, uinv=fuinv.reshape(-1))
    g = solve_ref_ilu_f32.rounded(f, val=fval, uinv=fuinv.reshape(-1))
    zs = [gl.apply(v) for v in inputs]
    noise = max(max(ld.rel_diff(g.apply(v), z)) for v, z in zip(inputs, zs))
    err = max(max(ld.rel_diff(z32, z)) for z32, z in zip(got, zs))
    diff = [float(np.linalg.norm(a - b) / np.linalg.norm(b)) for a, b in zip(got, plain)]
    off_diag = (f.F.shape[0] - n) * nv * nv              # of the owned square: a ghost block has no slot in the copy
    print(f"pihna_ghosted ({n} owned of {ctx.n_node} nodes): fp32-factor apply error {err:.2e} = {err / max(noise, 16 * EPS):.2f} x max(noise "
          f"{noise:.2e}, 16 eps); against the FP64-factor apply {min(diff):.2e} .. {max(diff):.2e}; +{bytes32 - bytes64} bytes, 4 x off-diagonal "
          f"non-zeros of the owned square = {4 * off_diag}, of the rows = {4 * (val.size - n * nv * nv)}")
    assert err <= ld.bound(MARGIN, noise), (err, noise)
    assert again.tobytes() == got[0].tobytes()
    assert 1e-9 <= min(diff) and max(diff) <= 1e-6, diff
    assert 4 * off_diag <= bytes32 - bytes64 <= 4 * (off_diag + 2 * 3 * nv * n) + 8 * (n + 1) + 2 * 256


# ---- 2. world 1: the bytes of rdc_solve with precond 4 ----
@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex"])
def test_world1_equals_the_single_partition_solve_bitwise(name):
    ctx, s, A, rhs, val = _open(name)
    tup = solve_ilu_f32_dist_ranks.info_tuple

    def solve(fn, precond, rel_tol, mixed):
        xd = _dev(np.zeros(rhs.size))
        info = fn(xd.data_ptr(), rel_tol=rel_tol, max_its=2000, precond=precond, rhs_scale=s.rhs_scale, mixed=mixed)
        return tup(info), xd.cpu().numpy().tobytes()

    with ctx:
        comm = _world1_comm(s)
        dist = lambda *a, **kw: ctx.solve_dist(comm, *a, **kw)   # noqa: E731
        plain = solve(ctx.solve, PRECOND_ILU0, 1e-10, False)
        ctx.set_option("ilu_factor_bits", 32)
        for rel_tol in (1e-8, 1e-10):
            for mixed in (False, True):
                e0, a0 = comm.exchanges, comm.allreduces
                d5 = solve(dist, PRECOND_ILU0_LOCAL, rel_tol, mixed)
                calls = (comm.exchanges - e0, comm.allreduces - a0)
                assert ctx.ilu_factor_bits() == 32
                s4 = solve(ctx.solve, PRECOND_ILU0, rel_tol, mixed)
                its, restarts = d5[0][I["iterations"]], d5[0][I["restarts"]]
                print(f"{name} tol {rel_tol:g} mixed {mixed}: {its} iterations (restarts {restarts}), callbacks {calls}")
                assert d5[0][I["reason"]] == SOLVE_CONVERGED and d5[0][I["matrix_bits"]] == (32 if mixed else 64)
                assert d5 == s4, "solve_dist(5) and solve(4) differ at world size 1"
                assert calls == (2 * its + 2 + restarts, 3 * its + 2 + restarts)
        assert solve(ctx.solve, PRECOND_ILU0, 1e-10, False)[1] != plain[1]
        _unchanged(ctx, val, rhs)


# ---- 3. two and three ranks against the global system ----
@pytest.mark.parametrize("name,world", [("pihna_kuhn", 2), ("hcc_hex", 3), ("pihna_kuhn3", 3)])
def test_ranks_against_global_system(oracle, name, world):
    s, A, b = solve_ref_dist.global_system(name, oracle)
    ranks = solve_ilu_f32_dist_ranks.run(name, world)
    print(f"{name} world {world}: owned {[rk['n_owned'] for rk in ranks]}, (set-up ms, bytes, colours) per rank {[rk['ilu_stats'] for rk in ranks]}")
    for rel_tol in (1e-8, 1e-10):
        ref = solve_ref_ilu_f32.yardstick_dist(name, world, oracle, rel_tol)[1]
        assert ref["reason"] == solve_ref.CONVERGED
        for what, bits, most in (("ilu", 64, ref["iterations"] + SLACK), ("mixed", 32, 2 * ref["iterations"] + 2)):
            key = (what, rel_tol)
            info = _same_info(ranks, key)
            xg = _gather(ranks, key, s.nv, s.xyz.shape[0])
            for r, rk in enumerate(ranks):
                loc = rk[key]["x"].reshape(-1, s.nv)
                assert loc[rk["n_owned"]:].tobytes() == xg[rk["node_global"][rk["n_owned"]:]].tobytes(), f"ghost rows of rank {r}"
            f = solve_ref.check_solution(A, b, xg.reshape(-1), s.nv, 2, rel_tol, extra_rel=ASSEMBLY_REL)
            print(f"  tol {rel_tol:g} {what}: iterations {info[I['iterations']]} (restarts {info[I['restarts']]}), yardstick {ref['iterations']}; "
                  f"residual {f['residual_norm']:.3e} <= {f['bound']:.3e}; callbacks per rank {[rk[key]['calls'] for rk in ranks]}")
            assert info[I["reason"]] == SOLVE_CONVERGED
            assert info[I["matrix_bits"]] == bits and info[I["bad_blocks"]] == 0
            assert all(rk[key]["bits"] == 32 for rk in ranks)
            assert abs(info[I["residual_norm"]] - f["residual_norm"]) <= f["rho"]
            assert info[I["iterations"]] <= most, (info, ref)
            assert all(rk[key]["repeat_same"] for rk in ranks), "a second solve in the same processes returned other bytes"
            nres = 2 + info[I["restarts"]]
            assert all(rk[key]["calls"] == (2 * info[I["iterations"]] + nres, 3 * info[I["iterations"]] + nres) for rk in ranks)
