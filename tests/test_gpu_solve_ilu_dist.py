"""RDC_PRECOND_ILU0_LOCAL through the C-ABI (rdc_solve_dist with precond = 5; rdc_solve_ilu_local_apply, rdc_solve_ilu_local_download):
the rank-local block ILU(0), block Jacobi between the ranks and ILU(0) inside each.

1. In this process on a ghosted context: factor and apply of the OWNED SQUARE against the extended-precision
   solve_ref_ilu.Factor of the values this context assembled; bound = MARGIN x max(noise, 16 eps), noise = numpy FP64's own error
   on the same system and inputs: margin and form of tests/test_gpu_solve_ilu.py, taken over unchanged.
2. World 1: solve_dist(5), solve(5) and solve(4) return the same bytes.
3. Worlds 2 and 3 (tests/solve_ilu_dist_ranks.py: one process per rank, gloo, all on GPU 0): the gathered x against the ORACLE's
   global system as tests/test_gpu_solve_dist.py judges it, iterations <= the numpy yardstick (tests/solve_ref_ilu_dist.py) + SLACK
   and below block Jacobi's in the same processes, identical info on every rank, ghost rows, repeatability, callback counts: two
   exchanges and three all-reduces per iteration, one of each per true residual -- the count of bad pivots rides in the all-reduce
   of the first residual, so there is no further one.
4. A singular diagonal block on rank 1: every rank reports it.
5. Refusals."""
import ctypes as C

import numpy as np
import pytest

import solve_ilu_dist_ranks
import solve_ref
import solve_ref_dist
import solve_ref_ilu
import solve_ref_ilu_dist
import solve_ref_mg_ld as ld
import solve_systems
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import RdcError, SolveInfo, SolveParams, partition
from rdcfes_amd.context import (ERR_INVALID, ERR_STATE, ERR_UNSUPPORTED, PRECOND_BLOCK_JACOBI, PRECOND_ILU0, PRECOND_ILU0_LOCAL,
                                PRECOND_MULTIGRID, SOLVE_BAD_DIAGONAL, SOLVE_CONVERGED)

pytestmark = pytest.mark.gpu
MARGIN, SLACK = 64.0, 2          # those of tests/test_gpu_solve_ilu.py
ASSEMBLY_REL = 1e-10             # that of tests/test_gpu_solve_dist.py
EPS = ld.EPS
I = {f: i for i, f in enumerate(solve_ilu_dist_ranks.INFO_FIELDS)}


def _raises(code, fn, match=None):
    with pytest.raises(RdcError, match=match) as ei:
        fn()
    assert ei.value.code == code, ei.value
    return ei.value


def _world1_comm(s, sized=False):
    from rdcfes_amd import SolveComm
    lp = partition.build_local(s.conn, s.xyz, np.zeros(s.conn.shape[0], dtype=np.int32), 0, 1)
    assert lp.n_owned == s.xyz.shape[0] and not lp.send_ids and not lp.recv_ids
    return SolveComm(lp, s.nv, "cuda:0", sized=sized)


# ---- 1. factor and apply of the owned square, in process ----
def test_factor_and_apply_of_the_owned_square():
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    nv, n = s.nv, rhs.size // s.nv
    assert n < ctx.n_node and A.shape == (n * nv, ctx.n_node * nv)
    sq = A[:, :n * nv].tocsr()
    f, fl = solve_ref_ilu.Factor(sq, nv), solve_ref_ilu.Factor(sq, nv, dtype=np.longdouble)
    assert f.singular == 0 and fl.singular == 0
    want, want_u = fl.values(), fl.Uinv.reshape(-1)
    noise_f = max(ld.rel_diff(f.values(), want))
    noise_u = max(ld.rel_diff(f.Uinv.reshape(-1), want_u))
    inputs = ld.probe_vectors(rhs.size, s.rhs_scale * rhs)
    zs = [fl.apply(v) for v in inputs]
    noise_a = max(max(ld.rel_diff(f.apply(v), z)) for v, z in zip(inputs, zs))
    with ctx:
        _raises(ERR_STATE, ctx.ilu_stats)
        _raises(ERR_STATE, ctx.ilu_local_factor)
        got = [ctx.ilu_local_apply(v) for v in inputs]
        again = ctx.ilu_local_apply(inputs[0])
        got_f, got_u = ctx.ilu_local_factor()
        ms, nbytes, colours = ctx.ilu_stats()
        _unchanged(ctx, val, rhs)
        # the existing hooks still refuse this context, and leave their output alone
        x0 = np.random.default_rng(3).uniform(size=ctx.n_node * nv)
        xd, yd = _dev(x0), _dev(x0[:rhs.size])
        _raises(ERR_UNSUPPORTED, lambda: ctx.ilu_apply_device(yd.data_ptr(), xd.data_ptr()), match="ghost")
        _raises(ERR_UNSUPPORTED, ctx.ilu_factor, match="ghost")
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_ILU0), match="ghost")
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
    assert got_f.size == want.size
    err_f, err_u = max(ld.rel_diff(got_f, want)), max(ld.rel_diff(got_u.reshape(-1), want_u))
    err_a = max(max(ld.rel_diff(g, z)) for g, z in zip(got, zs))
    print(f"pihna_ghosted ({n} owned of {ctx.n_node} nodes): factor error {err_f:.2e} = {err_f / max(noise_f, 16 * EPS):.2f} x max(noise {noise_f:.2e}, 16 eps); "
          f"U_ii^-1 error {err_u:.2e} = {err_u / max(noise_u, 16 * EPS):.2f} x max(noise {noise_u:.2e}, 16 eps); apply error {err_a:.2e} = "
          f"{err_a / max(noise_a, 16 * EPS):.2f} x max(noise {noise_a:.2e}, 16 eps); {colours} colours, {nbytes} bytes, set-up {ms:.3f} ms")
    assert np.all(np.isfinite(got_f)) and np.all(np.isfinite(got_u)) and all(np.all(np.isfinite(g)) for g in got)
    assert err_f <= ld.bound(MARGIN, noise_f), (err_f, noise_f)
    assert err_u <= ld.bound(MARGIN, noise_u), (err_u, noise_u)
    assert err_a <= ld.bound(MARGIN, noise_a), (err_a, noise_a)
    assert again.tobytes() == got[0].tobytes()
    assert colours == int(f.colour.max()) + 1
    # the ghost blocks keep their slots: values of every block, U_ii^-1, M p and M s with a ghost tail, five lists
    nnz, nblk, nloc = val.size, val.size // nv ** 2, ctx.n_node * nv
    assert 8 * (nnz + n * nv * nv + 2 * nloc) + 4 * (nblk + 4 * n) <= nbytes <= 8 * (nnz + n * nv * nv + 2 * nloc) + 4 * (nblk + 4 * n) + 9 * 256


# ---- 2. world 1: the bytes of rdc_solve with precond 4 ----
@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex"])
def test_world1_equals_the_single_partition_ilu_bitwise(name):
    ctx, s, A, rhs, val = _open(name)
    tup = solve_ilu_dist_ranks.info_tuple

    def solve(fn, precond, rel_tol):
        xd = _dev(np.zeros(rhs.size))
        info = fn(xd.data_ptr(), rel_tol=rel_tol, max_its=2000, precond=precond, rhs_scale=s.rhs_scale)
        return tup(info), xd.cpu().numpy().tobytes()

    with ctx:
        comm = _world1_comm(s)
        dist = lambda *a, **kw: ctx.solve_dist(comm, *a, **kw)
        before = [solve(ctx.solve, p, 1e-10) for p in (PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID)]
        for rel_tol in (1e-8, 1e-10):
            e0, a0 = comm.exchanges, comm.allreduces
            d5 = solve(dist, PRECOND_ILU0_LOCAL, rel_tol)
            calls = (comm.exchanges - e0, comm.allreduces - a0)
            s5, s4 = solve(ctx.solve, PRECOND_ILU0_LOCAL, rel_tol), solve(ctx.solve, PRECOND_ILU0, rel_tol)
            its, restarts = d5[0][I["iterations"]], d5[0][I["restarts"]]
            print(f"{name} tol {rel_tol:g}: {its} iterations (restarts {restarts}), callbacks {calls}")
            assert d5[0][I["reason"]] == SOLVE_CONVERGED and d5[0][I["matrix_bits"]] == 64
            assert d5 == s5 == s4, "solve_dist(5), solve(5) and solve(4) differ at world size 1"
            assert calls == (2 * its + 2 + restarts, 3 * its + 2 + restarts)
        after = [solve(ctx.solve, p, 1e-10) for p in (PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID)]
        assert before == after, "a solve with the rank-local ILU(0) changed what block Jacobi or multigrid return"
        y = np.random.default_rng(6).standard_normal(rhs.size)
        assert ctx.ilu_local_apply(y).tobytes() == ctx.ilu_apply(y).tobytes()
        fa, fb = ctx.ilu_local_factor(), ctx.ilu_factor()
        assert fa[0].tobytes() == fb[0].tobytes() and fa[1].tobytes() == fb[1].tobytes()
        _unchanged(ctx, val, rhs)


# ---- 3. two and three ranks against the global system ----
def _gather(ranks, key, nv, n_node):
    x = np.full((n_node, nv), np.nan)
    for rk in ranks:
        x[rk["node_global"][:rk["n_owned"]]] = rk[key]["x"].reshape(-1, nv)[:rk["n_owned"]]
    assert np.all(np.isfinite(x))
    return x


def _same_info(ranks, key):
    infos = [rk[key]["info"] for rk in ranks]
    assert all(i == infos[0] for i in infos), infos     # floats compared exactly: identical bits on every rank
    return infos[0]


@pytest.mark.parametrize("name,world", [("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("pihna_kuhn3", 3)])
def test_ranks_against_global_system(oracle, name, world):
    s, A, b = solve_ref_dist.global_system(name, oracle)
    ranks = solve_ilu_dist_ranks.run(name, world, extras=(name, world) == ("pihna_kuhn", 2))
    print(f"{name} world {world}: owned {[rk['n_owned'] for rk in ranks]}, interior {[rk['n_interior'] for rk in ranks]}, "
          f"(set-up ms, bytes, colours) per rank {[rk['ilu_stats'] for rk in ranks]}")
    for rel_tol in (1e-8, 1e-10):
        key = ("ilu", rel_tol)
        info, jac = _same_info(ranks, key), _same_info(ranks, ("jacobi", rel_tol))
        xg = _gather(ranks, key, s.nv, s.xyz.shape[0])
        for r, rk in enumerate(ranks):
            loc = rk[key]["x"].reshape(-1, s.nv)
            assert loc[rk["n_owned"]:].tobytes() == xg[rk["node_global"][rk["n_owned"]:]].tobytes(), f"ghost rows of rank {r}"
        ref = solve_ref_ilu_dist.yardstick(name, world, oracle, rel_tol)[1]
        f = solve_ref.check_solution(A, b, xg.reshape(-1), s.nv, 2, rel_tol, extra_rel=ASSEMBLY_REL)
        print(f"  tol {rel_tol:g}: iterations {info[I['iterations']]} (restarts {info[I['restarts']]}), yardstick {ref['iterations']}, block Jacobi "
              f"{jac[I['iterations']]}; residual {f['residual_norm']:.3e} <= {f['bound']:.3e}; reported {info[I['residual_norm']]:.3e}; "
              f"callbacks per rank {[rk[key]['calls'] for rk in ranks]}")
        assert info[I["reason"]] == SOLVE_CONVERGED and jac[I["reason"]] == SOLVE_CONVERGED and ref["reason"] == solve_ref.CONVERGED
        assert info[I["matrix_bits"]] == 64 and info[I["bad_blocks"]] == 0
        assert abs(info[I["residual_norm"]] - f["residual_norm"]) <= f["rho"]
        assert info[I["iterations"]] <= ref["iterations"] + SLACK
        assert info[I["iterations"]] < jac[I["iterations"]]
        assert all(rk[key]["repeat_same"] for rk in ranks), "a second solve in the same processes returned other bytes"
        nres = 2 + info[I["restarts"]]
        assert all(rk[key]["calls"] == (2 * info[I["iterations"]] + nres, 3 * info[I["iterations"]] + nres) for rk in ranks)


# ---- 4. a singular diagonal block on one rank ----
def test_a_bad_block_on_one_rank_is_reported_by_all():
    ranks = solve_ilu_dist_ranks.run("pihna_kuhn", 2, extras=True)
    info = _same_info(ranks, "singular")
    print(f"singular block on rank 1: reason {info[I['reason']]}, bad_blocks {info[I['bad_blocks']]}, callbacks {[rk['singular']['calls'] for rk in ranks]}")
    assert info[I["reason"]] == SOLVE_BAD_DIAGONAL and info[I["bad_blocks"]] >= 1 and info[I["iterations"]] == 0
    assert all(rk["singular"]["owned_untouched"] for rk in ranks)
    assert all(rk["singular"]["calls"] == (1, 1) for rk in ranks)          # the first true residual and nothing else
    assert _same_info(ranks, "restored") == _same_info(ranks, ("ilu", 1e-10))
    assert all(rk["restored"]["x"].tobytes() == rk[("ilu", 1e-10)]["x"].tobytes() for rk in ranks)


# ---- 5. refusals ----
def test_refusals():
    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        x0 = np.random.default_rng(5).uniform(size=rhs.size)
        xd = _dev(x0)
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_ILU0_LOCAL, mixed=True), match="FP64 factor")
        for sized in (False, True):
            comm = _world1_comm(s, sized=sized)
            _raises(ERR_UNSUPPORTED, lambda: ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-8, precond=PRECOND_ILU0_LOCAL, mixed=True), match="FP64 factor")
            if sized:                                        # the wrapper sends only multigrid to rdc_solve_dist_mg: call it directly
                for mixed in (0, 1):
                    p, info = SolveParams(1e-8, 0.0, 1.0, 100, PRECOND_ILU0_LOCAL), SolveInfo()
                    rc = ctx._lib.rdc_solve_dist_mg(ctx._h, C.byref(p), C.byref(comm.sized_struct), mixed, C.c_void_p(xd.data_ptr()), C.byref(info))
                    assert rc == ERR_INVALID
            assert (comm.exchanges, comm.allreduces) == (0, 0)
        _raises(ERR_INVALID, lambda: ctx.solve(xd.data_ptr(), precond=7), match="unknown preconditioner")
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        _raises(ERR_STATE, ctx.ilu_stats)                    # nothing was built
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        x0 = np.random.default_rng(3).uniform(size=ctx.n_node * s.nv)
        xd = _dev(x0)
        _raises(ERR_UNSUPPORTED, lambda: ctx.solve(xd.data_ptr(), precond=PRECOND_ILU0_LOCAL), match="ghost")
        comm = _world1_comm(solve_systems.get("pihna_kuhn"))
        p, info = SolveParams(1e-8, 0.0, 1.0, 100, PRECOND_ILU0_LOCAL), SolveInfo()
        with pytest.raises(RdcError, match="rdc_solve_dist_plan") as ei:    # ghosts and no plan: as for every value
            ctx._ck(ctx._lib.rdc_solve_dist(ctx._h, C.byref(p), C.byref(comm.struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info)))
        assert ei.value.code == ERR_STATE
        assert (comm.exchanges, comm.allreduces) == (0, 0)
        assert xd.cpu().numpy().tobytes() == x0.tobytes()
        _raises(ERR_STATE, ctx.ilu_stats)
