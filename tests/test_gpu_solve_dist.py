"""Partitioned linear solve through the C-ABI (rdc_solve_dist, AssemblyContext.solve_dist with halo.SolveComm).

World 1, in this process: with an exchange that moves nothing and an all-reduce that leaves its values alone the partitioned
entry must return the bytes of rdc_solve / rdc_solve_mixed; the error returns.  World 2 and 3 (tests/solve_dist_ranks.py: one
process per rank, gloo, all on GPU 0 -- a correctness rig, no measure of speed): every rank assembles its part on the GPU, and
the gathered x is judged with solve_ref.check_solution against the ORACLE's global assembly (rounding term enlarged by the
1e-10 per-block assembly tolerance of tests/parity.py, as test_gpu_solve.py::test_time_loop does), the iteration count against
the global numpy yardstick within +-2 (tests/test_solve_ref_dist.py: the partitioned numpy iteration gives +-0; the margin is
for the order of the sums), and everything a rank decides by against what the other ranks report."""
import numpy as np
import pytest

import solve_dist_ranks
import solve_ref
import solve_ref_dist
import solve_systems
from solve_systems import _dev, _open, _unchanged
from rdcfes_amd import AssemblyContext, RdcError, partition
from rdcfes_amd.context import (ERR_COMM, ERR_STATE, ERR_UNSUPPORTED, SOLVE_BAD_DIAGONAL, SOLVE_CONVERGED, SOLVE_MAX_ITS)

pytestmark = pytest.mark.gpu
ASSEMBLY_REL = 1e-10
I = {f: i for i, f in enumerate(solve_dist_ranks.INFO_FIELDS)}


def _world1_comm(s, cls=None):
    from rdcfes_amd import SolveComm
    lp = partition.build_local(s.conn, s.xyz, np.zeros(s.conn.shape[0], dtype=np.int32), 0, 1)
    assert lp.n_owned == s.xyz.shape[0] and not lp.send_ids and not lp.recv_ids
    return (cls or SolveComm)(lp, s.nv, "cuda:0")


# ---- 1. world 1 equals rdc_solve, bitwise ----
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", ["pihna_kuhn", "hcc_hex"])
def test_world1_equals_solve_bitwise(name, mixed):
    ctx, s, A, rhs, val = _open(name)
    fields = solve_dist_ranks.INFO_FIELDS
    with ctx:
        comm = _world1_comm(s)
        for precond in (0, 1, 2):
            for rel_tol in (1e-8, 1e-10):
                kw = dict(rel_tol=rel_tol, max_its=5000, precond=precond, rhs_scale=s.rhs_scale, mixed=mixed)
                xa, xb, xc = (_dev(np.zeros(rhs.size)) for _ in range(3))
                ia = ctx.solve(xa.data_ptr(), **kw)
                e0, a0 = comm.exchanges, comm.allreduces
                ib = ctx.solve_dist(comm, xb.data_ptr(), **kw)
                ic = ctx.solve(xc.data_ptr(), **kw)
                ta, tb, tc = (solve_dist_ranks.info_tuple(i) for i in (ia, ib, ic))
                print(f"{name} mixed {mixed} precond {precond} tol {rel_tol:g}: {ia.iterations} / {ib.iterations} iterations, restarts "
                      f"{ia.restarts} / {ib.restarts}, reason {ib.reason}, matrix bits {ib.matrix_bits}, callbacks {comm.exchanges - e0} + {comm.allreduces - a0}")
                assert ta == tb == tc, dict(zip(fields, zip(ta, tb, tc)))
                assert xa.cpu().numpy().tobytes() == xb.cpu().numpy().tobytes(), "solve_dist at world size 1 differs from solve"
                assert xa.cpu().numpy().tobytes() == xc.cpu().numpy().tobytes(), "a solve after solve_dist differs from the one before"
                # two exchanges and three all-reduces per iteration, one of each per true residual (first, confirming, restarts)
                assert ib.reason == SOLVE_CONVERGED or precond < 2
                nres = 2 + ib.restarts if ib.reason == SOLVE_CONVERGED else None
                assert nres is None or (comm.exchanges - e0, comm.allreduces - a0) == (2 * ib.iterations + nres, 3 * ib.iterations + nres)
        _unchanged(ctx, val, rhs)


# ---- 2. two and three ranks against the global system ----
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
    infos = [rk[key]["info"] for rk in ranks]
    assert all(i == infos[0] for i in infos), infos     # floats compared exactly: identical bits on every rank
    return infos[0]


@pytest.mark.parametrize("name,world", [("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("pihna_kuhn3", 3)])
def test_ranks_against_global_system(oracle, name, world):
    s, A, b = solve_ref_dist.global_system(name, oracle)
    ranks = solve_dist_ranks.run(name, world, extras=(name, world) == ("pihna_kuhn", 2))
    print(f"{name} world {world}: owned {[rk['n_owned'] for rk in ranks]}, interior {[rk['n_interior'] for rk in ranks]}, "
          f"bytes per exchange {[rk['bytes_per_exchange'] for rk in ranks]}")
    for rel_tol in (1e-8, 1e-10):
        key = ("solve", rel_tol)
        info = _same_info(ranks, key)
        xg = _gather(ranks, key, s.nv, s.xyz.shape[0])
        _ghosts_hold_owner_values(ranks, key, xg, s.nv)
        ref = solve_ref_dist.yardstick(name, oracle, rel_tol)[1]
        f = solve_ref.check_solution(A, b, xg.reshape(-1), s.nv, 2, rel_tol, extra_rel=ASSEMBLY_REL)
        print(f"  tol {rel_tol:g}: iterations {info[I['iterations']]} (restarts {info[I['restarts']]}), yardstick {ref['iterations']}; "
              f"residual {f['residual_norm']:.3e} <= {f['bound']:.3e}; reported {info[I['residual_norm']]:.3e}; callbacks per rank "
              f"{[rk[key]['calls'] for rk in ranks]}")
        assert info[I["reason"]] == SOLVE_CONVERGED
        assert abs(info[I["iterations"]] - ref["iterations"]) <= 2
        assert abs(info[I["rhs_norm"]] - f["rhs_norm"]) <= (1e-13 + ASSEMBLY_REL) * f["rhs_norm"]
        assert abs(info[I["residual_norm"]] - f["residual_norm"]) <= f["rho"]
        assert all(rk[key]["repeat_same"] for rk in ranks), "a second solve in the same processes returned other bytes"
        nres = 2 + info[I["restarts"]]
        assert all(rk[key]["calls"] == (2 * info[I["iterations"]] + nres, 3 * info[I["iterations"]] + nres) for rk in ranks)


# ---- 3. interior rows read no ghost ----
def test_interior_rows_run_before_the_ghosts_arrive():
    ranks = solve_dist_ranks.run("pihna_kuhn", 2, extras=True)
    assert all(0 < rk["n_interior"] < rk["n_owned"] and rk["n_interior"] % 32 for rk in ranks)
    for rk in ranks:
        assert np.all(np.isfinite(rk["nan"]["x"]))
        assert rk["nan"]["info"] == rk[("solve", 1e-10)]["info"] and rk["nan"]["info"][I["reason"]] == SOLVE_CONVERGED
        assert rk["nan"]["x"].tobytes() == rk[("solve", 1e-10)]["x"].tobytes()


# ---- 4. collective decisions ----
def test_collective_decisions(oracle):
    s, A, b = solve_ref_dist.global_system("pihna_kuhn", oracle)
    ranks = solve_dist_ranks.run("pihna_kuhn", 2, extras=True)
    nv, n_node = s.nv, s.xyz.shape[0]
    # (a) b = 0 on rank 1 only: its own ||D^-1 b|| is 0, the global one is not -- it iterates with rank 0, and the x is that of the system
    info = _same_info(ranks, "zero_rhs_rank1")
    b1 = b.reshape(-1, nv).copy()
    b1[ranks[1]["node_global"][:ranks[1]["n_owned"]]] = 0.0
    xg = _gather(ranks, "zero_rhs_rank1", nv, n_node)
    _ghosts_hold_owner_values(ranks, "zero_rhs_rank1", xg, nv)
    f = solve_ref.check_solution(A, b1.reshape(-1), xg.reshape(-1), nv, 2, 1e-10, extra_rel=ASSEMBLY_REL)
    print(f"b = 0 on rank 1: {info[I['iterations']]} iterations, residual {f['residual_norm']:.3e} <= {f['bound']:.3e}")
    assert info[I["reason"]] == SOLVE_CONVERGED and info[I["iterations"]] > 0 and info[I["rhs_norm"]] > 0.0
    # (b) b = 0 everywhere: x = 0 in no iteration, ghost rows included, from a start of ones
    info = _same_info(ranks, "zero_rhs")
    assert info[I["reason"]] == SOLVE_CONVERGED and info[I["iterations"]] == 0 and info[I["residual_norm"]] == 0.0
    assert all(not rk["zero_rhs"]["x"].any() for rk in ranks)
    # (c) one singular diagonal block, on rank 1: every rank reports it with the global count and leaves its x alone
    info = _same_info(ranks, "singular")
    assert info[I["reason"]] == SOLVE_BAD_DIAGONAL and info[I["bad_blocks"]] == 1 and info[I["iterations"]] == 0
    assert all(rk["singular"]["owned_untouched"] for rk in ranks)
    assert _same_info(ranks, "restored") == _same_info(ranks, ("solve", 1e-10))
    assert all(rk["restored"]["x"].tobytes() == rk[("solve", 1e-10)]["x"].tobytes() for rk in ranks)
    # (d) max_its = 3: the same true residual everywhere, and it is the residual of the gathered x
    info = _same_info(ranks, "max_its")
    xg = _gather(ranks, "max_its", nv, n_node).reshape(-1)
    M, _, cond = solve_ref.precond_inverse(A, nv, 2)
    true = float(np.linalg.norm(M @ (b - A @ xg)))
    rho = (4.0 * solve_ref.longest_row(A) * solve_ref.EPS + ASSEMBLY_REL) * np.linalg.norm(abs(M) @ (abs(A) @ np.abs(xg) + np.abs(b)))
    assert info[I["reason"]] == SOLVE_MAX_ITS and info[I["iterations"]] == 3
    assert abs(info[I["residual_norm"]] - true) <= rho + 64.0 * solve_ref.EPS * cond * true
    assert info[I["residual_norm"]] > 1e-10 * info[I["rhs_norm"]]


# ---- 5. mixed precision, world 2 ----
def test_mixed_across_two_ranks(oracle):
    s, A, b = solve_ref_dist.global_system("pihna_kuhn", oracle)
    ranks = solve_dist_ranks.run("pihna_kuhn", 2, extras=True)
    info, info64 = _same_info(ranks, "mixed"), _same_info(ranks, ("solve", 1e-8))
    xg = _gather(ranks, "mixed", s.nv, s.xyz.shape[0])
    _ghosts_hold_owner_values(ranks, "mixed", xg, s.nv)
    f = solve_ref.check_solution(A, b, xg.reshape(-1), s.nv, 2, 1e-8, extra_rel=ASSEMBLY_REL)
    print(f"mixed, world 2: {info[I['iterations']]} iterations (FP64: {info64[I['iterations']]}), restarts {info[I['restarts']]}, residual "
          f"{f['residual_norm']:.3e} <= {f['bound']:.3e}")
    assert info[I["reason"]] == SOLVE_CONVERGED and info[I["matrix_bits"]] == 32 and info64[I["matrix_bits"]] == 64
    assert info[I["iterations"]] <= 1.5 * info64[I["iterations"]] + 2


# ---- 6. errors, world 1 ----
def test_errors():
    from rdcfes_amd import SolveComm

    class Failing(SolveComm):
        """the k-th all-reduce (counted from 0) returns 7 or raises"""
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls, self.fail_at, self.raise_ = 0, None, False

        def begin(self, send, recv, stream):
            self.calls += 1
            return super().begin(send, recv, stream)

        def end(self, stream):
            self.calls += 1
            return super().end(stream)

        def allreduce(self, vals, stream):
            self.calls += 1
            if self.fail_at is not None and self.allreduces == self.fail_at:
                self.allreduces += 1
                if self.raise_:
                    raise KeyError("lost a peer")
                return 7
            return super().allreduce(vals, stream)

    ctx, s, A, rhs, val = _open("pihna_kuhn")
    with ctx:
        comm = _world1_comm(s, Failing)
        x0 = np.zeros(rhs.size)
        xd = _dev(x0)
        ref = ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-10, max_its=2000)
        assert ref.reason == SOLVE_CONVERGED
        want = xd.cpu().numpy()
        # the 5th all-reduce is the first of the second iteration: 1 residual (2 exchange calls, 1 all-reduce), 1 iteration (4, 3), 2 + 1
        comm.calls, comm.allreduces, comm.fail_at = 0, 0, 4
        xd = _dev(x0)
        with pytest.raises(RdcError) as ei:
            ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-10, max_its=2000)
        assert ei.value.code == ERR_COMM == 6 and "7" in str(ei.value)
        assert comm.calls == 3 + 7 + 3, comm.calls                       # nothing was called after the failure
        x = xd.cpu().numpy()
        assert np.all(np.isfinite(x)) and x.any()                        # the last iterate: one iteration from 0
        comm.calls, comm.allreduces, comm.raise_ = 0, 0, True
        with pytest.raises(KeyError, match="lost a peer"):
            ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-10, max_its=2000)
        assert comm.calls == 13
        comm.fail_at = None                                              # the context and the communicator stay usable
        xd = _dev(x0)
        again = ctx.solve_dist(comm, xd.data_ptr(), rel_tol=1e-10, max_its=2000)
        assert solve_dist_ranks.info_tuple(again) == solve_dist_ranks.info_tuple(ref) and xd.cpu().numpy().tobytes() == want.tobytes()
        with pytest.raises(RdcError) as ei:
            ctx.solve_dist(comm, xd.data_ptr(), precond=3)
        assert ei.value.code == ERR_UNSUPPORTED
        with pytest.raises(RdcError) as ei:
            ctx.solve_dist_plan([rhs.size // s.nv])                      # one past the last owned node
        assert ei.value.code == 1
    ctx, s, A, rhs, val = _open("pihna_ghosted")
    with ctx:
        import ctypes as C
        from rdcfes_amd import SolveInfo, SolveParams
        comm = _world1_comm(solve_systems.get("pihna_kuhn"))
        xd = _dev(np.zeros(ctx.n_node * s.nv))
        p, info = SolveParams(1e-8, 0.0, 1.0, 100, 2), SolveInfo()
        with pytest.raises(RdcError, match="rdc_solve_dist_plan") as ei:    # ghosts and no plan
            ctx._ck(ctx._lib.rdc_solve_dist(ctx._h, C.byref(p), C.byref(comm.struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info)))
        assert ei.value.code == ERR_STATE
        assert comm.exchanges == 0 and comm.allreduces == 0
        with pytest.raises(RdcError, match="ghost") as ei:                  # the single-partition entry still refuses
            ctx.solve(xd.data_ptr())
        assert ei.value.code == ERR_UNSUPPORTED
