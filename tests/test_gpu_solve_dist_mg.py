"""Multigrid across ranks (rdc_solve_dist_mg; ctx.solve_dist with a sized SolveComm and precond = PRECOND_MULTIGRID).
World 1 in this process: bitwise what rdc_solve(precond = 3) returns.  Worlds 2 and 3 through tests/solve_dist_mg_ranks.py (gloo
ranks sharing GPU 0: correctness only) against the oracle's global assembly and the numpy yardstick tests/solve_ref_mg_dist.py,
whose hierarchy tests/test_host_solve_mg_dist.py shows to be that of the compiled host builder."""
import ctypes as C

import numpy as np
import pytest

import solve_dist_mg_ranks
import solve_dist_ranks
import solve_ref
import solve_ref_dist
import solve_ref_mg_dist
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import RdcError, SolveInfo, SolveParams, partition
from rdcfes_amd.context import (ERR_COMM, ERR_STATE, ERR_UNSUPPORTED, SOLVE_BAD_DIAGONAL, SOLVE_CONVERGED, SOLVE_MAX_ITS)

pytestmark = pytest.mark.gpu
ASSEMBLY_REL = 1e-10
I = {f: i for i, f in enumerate(solve_dist_ranks.INFO_FIELDS)}
MG = 3
_YARD = {}


def _world1_comm(s, cls=None, sized=True):
    from rdcfes_amd import SolveComm
    lp = partition.build_local(s.conn, s.xyz, np.zeros(s.conn.shape[0], dtype=np.int32), 0, 1)
    assert lp.n_owned == s.xyz.shape[0] and not lp.send_ids and not lp.recv_ids
    return (cls or SolveComm)(lp, s.nv, "cuda:0", sized=sized)


def _yardstick(name, world, oracle, rel_tol):
    """(info, hierarchy) of the numpy yardstick from x0 = 0; the hierarchy once per (name, world)"""
    s = solve_ref_dist.case(name)
    ranks = solve_ref_dist.ranks_of(name, world, oracle)
    if (name, world) not in _YARD:
        _YARD[(name, world)] = solve_ref_mg_dist.HierarchyDist(ranks, s.nv)
    H = _YARD[(name, world)]
    if (name, world, rel_tol) not in _YARD:
        _YARD[(name, world, rel_tol)] = solve_ref_mg_dist.bicgstab_dist(ranks, [np.zeros(rk.A.shape[1]) for rk in ranks], rel_tol, nv=s.nv, hierarchy=H)[1]
    return _YARD[(name, world, rel_tol)], H


# ---- 1. world 1 equals rdc_solve(precond = 3), bitwise ----
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex"])
def test_world1_equals_solve_bitwise(name, mixed):
    ctx, s, A, rhs, val = _open(name)
    with ctx:
        comm = _world1_comm(s)
        for rel_tol in (1e-8, 1e-10):
            kw = dict(rel_tol=rel_tol, max_its=5000, precond=MG, rhs_scale=s.rhs_scale, mixed=mixed)
            xa, xb, xc = (_dev(np.zeros(rhs.size)) for _ in range(3))
            ia = ctx.solve(xa.data_ptr(), **kw)
            la = ctx.mg_levels()
            c0 = (comm.exchanges, comm.sized_exchanges, comm.allreduces)
            ib = ctx.solve_dist(comm, xb.data_ptr(), **kw)
            lb = ctx.mg_levels()
            calls = tuple(b - a for a, b in zip(c0, (comm.exchanges, comm.sized_exchanges, comm.allreduces)))
            ic = ctx.solve(xc.data_ptr(), **kw)
            ta, tb, tc = (solve_dist_ranks.info_tuple(i) for i in (ia, ib, ic))
            print(f"{name} mixed {mixed} tol {rel_tol:g}: {ia.iterations} / {ib.iterations} iterations, restarts {ia.restarts} / {ib.restarts}, "
                  f"matrix bits {ib.matrix_bits}, levels {lb}, callbacks {calls}")
            assert ta == tb == tc, dict(zip(solve_dist_ranks.INFO_FIELDS, zip(ta, tb, tc)))
            assert la == lb == ctx.mg_levels() and len(lb) >= 3
            assert xa.cpu().numpy().tobytes() == xb.cpu().numpy().tobytes(), "the multigrid solve across ranks at world size 1 differs from solve"
            assert xa.cpu().numpy().tobytes() == xc.cpu().numpy().tobytes(), "a solve after it differs from the one before"
            assert ib.reason == SOLVE_CONVERGED and ib.matrix_bits == (32 if mixed else 64)
        _unchanged(ctx, val, rhs)


# ---- 2. two and three ranks against the global system and the yardstick ----
def _gather(ranks, key, nv, n_node):
    x = np.full((n_node, nv), np.nan)
    for rk in ranks:
        x[rk["node_global"][:rk["n_owned"]]] = rk[key]["x"].reshape(-1, nv)[:rk["n_owned"]]
    assert np.all(np.isfinite(x))
    return x


def _ghosts_hold_owner_values(ranks, key, xg, nv):
    for r, rk in enumerate(ranks):
        loc = rk[key]["x"].reshape(-1, nv)
        assert loc[rk["n_owned"]:].tobytes() == xg[rk["node_global"][rk["n_owned"]:]].tobytes(), f"ghost rows of rank {r} ({key})"


def _same_info(ranks, key):
    infos = [rk[key]["info"] if isinstance(rk[key], dict) else rk[key] for rk in ranks]
    assert all(i == infos[0] for i in infos), infos     # floats compared exactly: identical bits on every rank
    return infos[0]


@pytest.mark.parametrize("name,world", [("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("pihna_kuhn3", 3)])
def test_ranks_against_global_system(oracle, name, world):
    s, A, b = solve_ref_dist.global_system(name, oracle)
    ranks = solve_dist_mg_ranks.run(name, world, extras=(name, world) == ("pihna_kuhn", 2))
    for rel_tol in (1e-8, 1e-10):
        key = ("solve", rel_tol)
        info = _same_info(ranks, key)
        jac = _same_info(ranks, ("jacobi", rel_tol))
        xg = _gather(ranks, key, s.nv, s.xyz.shape[0])
        _ghosts_hold_owner_values(ranks, key, xg, s.nv)
        ref, H = _yardstick(name, world, oracle, rel_tol)
        f = solve_ref.check_solution(A, b, xg.reshape(-1), s.nv, 2, rel_tol, extra_rel=ASSEMBLY_REL)
        its, L = info[I["iterations"]], H.n_levels
        print(f"{name} world {world} tol {rel_tol:g}: iterations {its} (restarts {info[I['restarts']]}), yardstick {ref['iterations']}, block Jacobi "
              f"{jac[I['iterations']]}; residual {f['residual_norm']:.3e} <= {f['bound']:.3e}; levels per rank {[rk[('levels', rel_tol)] for rk in ranks]}; "
              f"callbacks (exchanges, sized, all-reduces) first solve {[rk[key]['first_calls'] for rk in ranks]}, second {[rk[key]['calls'] for rk in ranks]}")
        assert info[I["reason"]] == SOLVE_CONVERGED and info[I["matrix_bits"]] == 64
        assert abs(its - ref["iterations"]) <= 2
        assert its <= jac[I["iterations"]] and jac[I["reason"]] == SOLVE_CONVERGED
        assert abs(info[I["rhs_norm"]] - f["rhs_norm"]) <= (1e-13 + ASSEMBLY_REL) * f["rhs_norm"]
        assert abs(info[I["residual_norm"]] - f["residual_norm"]) <= f["rho"]
        assert all(rk[key]["repeat_same"] for rk in ranks), "a second solve in the same processes returned other bytes"
        for r, rk in enumerate(ranks):
            assert rk[("levels", rel_tol)] == H.level_sizes(r), f"rank {r}"
        # callbacks: 6 exchanges of the plan's size per iteration and one per true residual; 2 (2 (L - 2) + 7) sized ones per iteration;
        # the all-reduces of rdc_solve_dist.  The first solve builds the hierarchy: one sized exchange and one all-reduce per
        # coarsening step, and the all-reduce of the step that decides to stop.
        nres = 2 + info[I["restarts"]]
        want = (6 * its + nres, 2 * (2 * (L - 2) + 7) * its, 3 * its + nres)
        assert all(rk[key]["calls"] == want for rk in ranks)
        if rel_tol == 1e-8:
            assert all(rk[key]["first_calls"] == (want[0], want[1] + L - 1, want[2] + L) for rk in ranks)
        else:
            assert all(rk[key]["first_calls"] == want for rk in ranks)


# ---- 3. two ranks: mixed precision, ghosts that arrive late, collective decisions ----
def test_mixed_across_two_ranks(oracle):
    s, A, b = solve_ref_dist.global_system("pihna_kuhn", oracle)
    ranks = solve_dist_mg_ranks.run("pihna_kuhn", 2, extras=True)
    info = _same_info(ranks, "mixed")
    ref, _ = _yardstick("pihna_kuhn", 2, oracle, 1e-8)
    xg = _gather(ranks, "mixed", s.nv, s.xyz.shape[0])
    _ghosts_hold_owner_values(ranks, "mixed", xg, s.nv)
    f = solve_ref.check_solution(A, b, xg.reshape(-1), s.nv, 2, 1e-8, extra_rel=ASSEMBLY_REL)
    print(f"mixed, world 2: {info[I['iterations']]} iterations (yardstick in FP64: {ref['iterations']}), restarts {info[I['restarts']]}, residual "
          f"{f['residual_norm']:.3e} <= {f['bound']:.3e}")
    assert info[I["reason"]] == SOLVE_CONVERGED and info[I["matrix_bits"]] == 32


def test_nothing_reads_a_ghost_before_it_arrives():
    ranks = solve_dist_mg_ranks.run("pihna_kuhn", 2, extras=True)
    for rk in ranks:
        assert np.all(np.isfinite(rk["nan"]["x"]))
        assert rk["nan"]["info"] == rk[("solve", 1e-10)]["info"] and rk["nan"]["info"][I["reason"]] == SOLVE_CONVERGED
        assert rk["nan"]["x"].tobytes() == rk[("solve", 1e-10)]["x"].tobytes()


def test_collective_decisions(oracle):
    s, A, b = solve_ref_dist.global_system("pihna_kuhn", oracle)
    ranks = solve_dist_mg_ranks.run("pihna_kuhn", 2, extras=True)
    nv, n_node = s.nv, s.xyz.shape[0]
    # (a) b = 0 on rank 1 only: it iterates with rank 0, and the x is that of the system
    info = _same_info(ranks, "zero_rhs_rank1")
    b1 = b.reshape(-1, nv).copy()
    b1[ranks[1]["node_global"][:ranks[1]["n_owned"]]] = 0.0
    xg = _gather(ranks, "zero_rhs_rank1", nv, n_node)
    _ghosts_hold_owner_values(ranks, "zero_rhs_rank1", xg, nv)
    f = solve_ref.check_solution(A, b1.reshape(-1), xg.reshape(-1), nv, 2, 1e-10, extra_rel=ASSEMBLY_REL)
    print(f"b = 0 on rank 1: {info[I['iterations']]} iterations, residual {f['residual_norm']:.3e} <= {f['bound']:.3e}")
    assert info[I["reason"]] == SOLVE_CONVERGED and info[I["iterations"]] > 0 and info[I["rhs_norm"]] > 0.0
    # (b) one singular diagonal block, on rank 1: every rank reports it and leaves its x alone.  The block is singular on level 0; the
    # aggregate that holds it may or may not be on level 1, so the count is at least 1.
    info = _same_info(ranks, "singular")
    assert info[I["reason"]] == SOLVE_BAD_DIAGONAL and info[I["bad_blocks"]] >= 1 and info[I["iterations"]] == 0
    assert all(rk["singular"]["owned_untouched"] for rk in ranks)
    assert _same_info(ranks, "restored") == _same_info(ranks, ("solve", 1e-10))
    assert all(rk["restored"]["x"].tobytes() == rk[("solve", 1e-10)]["x"].tobytes() for rk in ranks)
    # (c) max_its = 3: the same true residual everywhere, and it is the residual of the gathered x
    info = _same_info(ranks, "max_its")
    xg = _gather(ranks, "max_its", nv, n_node).reshape(-1)
    M, _, cond = solve_ref.precond_inverse(A, nv, 2)
    true = float(np.linalg.norm(M @ (b - A @ xg)))
    rho = (4.0 * solve_ref.longest_row(A) * solve_ref.EPS + ASSEMBLY_REL) * np.linalg.norm(abs(M) @ (abs(A) @ np.abs(xg) + np.abs(b)))
    assert info[I["reason"]] == SOLVE_MAX_ITS and info[I["iterations"]] == 3
    assert abs(info[I["residual_norm"]] - true) <= rho + 64.0 * solve_ref.EPS * cond * true
    assert info[I["residual_norm"]] > 1e-10 * info[I["rhs_norm"]]


# ---- 4. errors ----
def test_errors():
    from rdcfes_amd import SolveComm

    class Failing(SolveComm):
        """the k-th sized begin (counted from 0) returns 7"""
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls, self.fail_at = 0, None

        def begin(self, send, recv, stream):
            self.calls += 1
            return super().begin(send, recv, stream)

        def end(self, stream):
            self.calls += 1
            return super().end(stream)

        def allreduce(self, vals, stream):
            self.calls += 1
            return super().allreduce(vals, stream)

        def sized_end(self, stream):
            self.calls += 1
            return super().sized_end(stream)

        def sized_begin(self, send, recv, send_off, recv_off, stream):
            self.calls += 1
            if self.fail_at is not None and self.sized_exchanges == self.fail_at:
                self.sized_exchanges += 1
                return 7
            return super().sized_begin(send, recv, send_off, recv_off, stream)

    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        comm = _world1_comm(s, Failing)
        xd = _dev(np.zeros(rhs.size))
        with pytest.raises(RdcError) as ei:                                  # the new entry takes the multigrid preconditioner only
            p, info = SolveParams(1e-8, 0.0, 1.0, 100, 2), SolveInfo()
            ctx.solve_dist(comm, xd.data_ptr(), precond=2)                   # (uploads plan and peers; goes to rdc_solve_dist)
            ctx._ck(ctx._lib.rdc_solve_dist_mg(ctx._h, C.byref(p), C.byref(comm.sized_struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info)))
        assert ei.value.code == 1
        xd = _dev(np.zeros(rhs.size))
        ref = ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-10, max_its=2000, precond=MG)
        want = xd.cpu().numpy()
        assert ref.reason == SOLVE_CONVERGED
        # the hierarchy exists: a solve starts with 1 residual (2 exchange calls, 1 all-reduce), then the first cycle: a level-0
        # exchange (2 calls) and the first sized begin, which fails
        comm.calls, comm.sized_exchanges, comm.fail_at = 0, 0, 0
        xd = _dev(np.zeros(rhs.size))
        with pytest.raises(RdcError) as ei:
            ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-10, max_its=2000, precond=MG)
        assert ei.value.code == ERR_COMM == 6 and "7" in str(ei.value)
        assert comm.calls == 3 + 2 + 1, comm.calls                           # nothing was called after the failure
        comm.fail_at = None                                                  # the context and the communicator stay usable
        xd = _dev(np.zeros(rhs.size))
        again = ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-10, max_its=2000, precond=MG)
        assert solve_dist_ranks.info_tuple(again) == solve_dist_ranks.info_tuple(ref) and xd.cpu().numpy().tobytes() == want.tobytes()
        plain = _world1_comm(s, sized=False)                                 # without the sized exchange: as before
        with pytest.raises(RdcError) as ei:
            ctx.solve_dist(plain, xd.data_ptr(), precond=MG)
        assert ei.value.code == ERR_UNSUPPORTED
        one = (C.c_int64 * 1)(1)
        assert ctx._lib.rdc_solve_dist_plan_peers(ctx._h, 1, one, one) == 1   # counts that do not add up to the (empty) plan
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        comm = _world1_comm(solve_ref_dist.case("pihna_kuhn"), Failing)
        xd = _dev(np.zeros(ctx.n_node * s.nv))
        p, info = SolveParams(1e-8, 0.0, 1.0, 100, MG), SolveInfo()
        zero = (C.c_int64 * 1)(0)
        assert ctx._lib.rdc_solve_dist_plan_peers(ctx._h, 0, zero, zero) == ERR_STATE      # before a plan
        with pytest.raises(RdcError, match="rdc_solve_dist_plan") as ei:                 # ghosts, no plan, no peers
            ctx._ck(ctx._lib.rdc_solve_dist_mg(ctx._h, C.byref(p), C.byref(comm.sized_struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info)))
        assert ei.value.code == ERR_STATE
        ctx.solve_dist_plan(np.zeros(0, dtype=np.int32))
        with pytest.raises(RdcError, match="rdc_solve_dist_plan_peers") as ei:           # a plan, still no peers
            ctx._ck(ctx._lib.rdc_solve_dist_mg(ctx._h, C.byref(p), C.byref(comm.sized_struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info)))
        assert ei.value.code == ERR_STATE
        assert comm.calls == 0 and comm.exchanges == 0 and comm.sized_exchanges == 0 and comm.allreduces == 0
