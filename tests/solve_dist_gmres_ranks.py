"""The rank processes of tests/test_gpu_solve_dist_gmres.py, beside tests/solve_ilu_dist_ranks.py and of its shape: run(name, world)
starts one process per rank (spawn, gloo on 127.0.0.1, every rank on GPU 0 -- a correctness rig, no measure of speed), each assembles
its part of solve_ref_dist.CASES[name] on the GPU and runs, through a SolveComm(..., wide=True):

  solves   every case of solve_ref_gmres_dist.CASES for (name, world), at both tolerances, twice each: the returned local x, the
           fields of SolveInfo that must agree across ranks, the callback counts (of the second solve: the first multigrid solve
           after a plan also builds the hierarchy) and the lengths of the wide all-reduces;
  arnoldi  (ARNOLDI_ON) rdc_solve_dist_gmres_arnoldi, 12 steps, precond 2, 5 and 3, one and two passes, from the rhs and from a
           seeded random vector: this rank's rows of the basis, H, the steps done -- and the system this rank assembled, downloaded,
           so that the parent can build the very operator the ranks applied;
  extras   (EXTRAS_ON) a singular diagonal block on rank 1 and the solve after it is restored; a wide all-reduce that fails at its
           third call on every rank.

A rank that raises puts its traceback on the queue; the parent ends the others as soon as one has failed or died."""
import queue
import socket
import traceback
from datetime import timedelta

import numpy as np

from solve_dist_ranks import INFO_FIELDS, SINGULAR_NODE, _view, info_tuple  # noqa: F401 (the test names the fields through this module)

ARNOLDI_ON = {("pihna_kuhn", 2), ("hcc_hex", 2)}
EXTRAS_ON = {("pihna_kuhn", 2)}
STEPS = 12
ARNOLDI_SEED = 21


def random_start(n_global_dofs):
    """the seeded random start of the Arnoldi runs, in the global numbering; a rank takes the rows it owns"""
    return np.random.default_rng(ARNOLDI_SEED).standard_normal(n_global_dofs)


def _rank_body(rank, world, name):
    import torch
    import solve_ref_dist
    import solve_ref_gmres_dist
    from rdcfes_amd import AssemblyContext, RdcError, SolveComm
    from rdcfes_amd.context import ERR_COMM, PRECOND_ILU0_LOCAL
    s = solve_ref_dist.case(name)
    lp = solve_ref_dist.partitions(s, world)[rank]
    loc = solve_ref_dist.local_system(s, lp)
    torch.cuda.set_device(0)
    nv = s.nv
    nloc, nown = lp.xyz.shape[0] * nv, lp.n_owned * nv
    out = dict(n_owned=lp.n_owned, n_interior=lp.n_interior, node_global=lp.node_global, n_nodes=lp.xyz.shape[0])

    class FailingWide(SolveComm):
        """the wide all-reduce returns 1 at its third call -- on every rank alike, so that no rank waits for another"""
        def allreduce_wide(self, vals, stream):
            if self.wide_allreduces == 2:
                self.wide_allreduces += 1
                return 1
            return super().allreduce_wide(vals, stream)

    with AssemblyContext(0) as ctx:
        ctx.set_option("interior_nodes", int(lp.n_interior))
        loc.upload(ctx)
        loc.assemble(ctx)
        ctx.synchronize()
        comm = SolveComm(lp, nv, "cuda:0", wide=True)

        def counts(c):
            return (c.exchanges, c.allreduces, c.sized_exchanges, c.wide_allreduces)

        def solve(x0, c=comm, **kw):
            xd = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)).to("cuda:0")
            torch.cuda.synchronize()
            before, nw = counts(c), len(c.wide_lengths)
            info = ctx.solve_dist_gmres(c, xd.data_ptr(), max_its=2000, rhs_scale=s.rhs_scale, **kw)
            return dict(x=xd.cpu().numpy(), info=info_tuple(info), calls=tuple(a - b for a, b in zip(counts(c), before)),
                        wide=list(c.wide_lengths[nw:]), stats=ctx.gmres_stats())

        zeros = np.zeros(nloc)
        for case in solve_ref_gmres_dist.CASES:
            if case[:2] != (name, world):
                continue
            _, _, precond, restart, refine = case
            ctx.set_option("gmres_restart", restart)
            ctx.set_option("gmres_refine", int(refine))
            for tol in solve_ref_gmres_dist.TOLS:
                a = solve(zeros, rel_tol=tol, precond=precond)
                b = solve(zeros, rel_tol=tol, precond=precond)
                a["repeat_same"] = all(a[k] == b[k] for k in ("info", "wide")) and a["x"].tobytes() == b["x"].tobytes()
                a["calls_first"], a["calls"] = a["calls"], b["calls"]   # the first multigrid solve after a plan also builds the hierarchy
                out[(case, tol)] = a
        if (name, world) in ARNOLDI_ON:
            val, rhs = ctx.csr_download()
            rp, col = ctx.csr_pattern()
            out["system"] = dict(rp=rp, col=col, val=val, rhs=rhs)
            dofs = (lp.node_global[:lp.n_owned].astype(np.int64)[:, None] * nv + np.arange(nv)).reshape(-1)
            starts = dict(rhs=s.rhs_scale * rhs, random=random_start(s.xyz.shape[0] * nv)[dofs])
            ctx.set_option("gmres_restart", STEPS)
            for precond in (2, 5, 3):
                for refine in (0, 1):
                    ctx.set_option("gmres_refine", refine)
                    for label, v0 in starts.items():
                        before, nw = counts(comm), len(comm.wide_lengths)
                        V, H = ctx.gmres_arnoldi_dist(comm, v0, STEPS, precond)
                        calls, wide = tuple(a - b for a, b in zip(counts(comm), before)), list(comm.wide_lengths[nw:])
                        V2, H2 = ctx.gmres_arnoldi_dist(comm, v0, STEPS, precond)
                        out[("arnoldi", precond, refine, label)] = dict(V=V, H=H, calls=calls, wide=wide,
                                                                         repeat_same=V.tobytes() == V2.tobytes() and H.tobytes() == H2.tobytes())
            v, r = ctx.csr_download()
            out["system"]["unchanged"] = v.tobytes() == val.tobytes() and r.tobytes() == rhs.tobytes()
        if (name, world) in EXTRAS_ON:
            ctx.set_option("gmres_restart", 30)
            ctx.set_option("gmres_refine", 0)
            good = dict(rel_tol=1e-10, precond=PRECOND_ILU0_LOCAL)
            out["undisturbed"] = solve(zeros, **good)
            vptr, _ = ctx.csr_values_device_ptr()
            val_d = _view(vptr, ctx.csr_dims()[1])
            keep_val = val_d.clone()
            if rank == 1:
                rp, col = ctx.csr_pattern()
                node = SINGULAR_NODE
                idx = np.concatenate([np.arange(rp[node * nv + a], rp[node * nv + a + 1])[col[rp[node * nv + a]:rp[node * nv + a + 1]] // nv == node]
                                      for a in range(nv)])
                assert idx.size == nv * nv
                val_d[torch.from_numpy(idx).to("cuda:0")] = 0.0
            x0 = np.random.default_rng(2 + rank).uniform(size=nloc)
            out["singular"] = solve(x0, **good)
            out["singular"]["owned_untouched"] = out["singular"]["x"][:nown].tobytes() == x0[:nown].tobytes()
            val_d.copy_(keep_val)
            torch.cuda.synchronize()
            out["restored"] = solve(zeros, **good)
            bad = FailingWide(lp, nv, "cuda:0", wide=True)
            xd = torch.from_numpy(x0.copy()).to("cuda:0")
            torch.cuda.synchronize()
            code = None
            try:
                ctx.solve_dist_gmres(bad, xd.data_ptr(), max_its=2000, rhs_scale=s.rhs_scale, rel_tol=1e-10, precond=2)
            except RdcError as e:
                code = e.code
            out["comm_failure"] = dict(is_err_comm=code == ERR_COMM, calls=counts(bad), wide=list(bad.wide_lengths),
                                       finite=bool(torch.isfinite(xd).all().item()))
            out["after_failure"] = solve(zeros, **good)
    return out


def _rank_main(rank, world, port, q, name):
    import os
    import torch.distributed as dist
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
        try:
            out = _rank_body(rank, world, name)
            dist.barrier()
        finally:
            dist.destroy_process_group()
        q.put((rank, True, out))
    except BaseException:
        q.put((rank, False, traceback.format_exc()))


_RUNS = {}


def run(name, world, limit=240.0):
    """[per-rank dict] of _rank_body, computed once per (name, world)"""
    key = (name, world)
    if key in _RUNS:
        return _RUNS[key]
    import time
    import torch.multiprocessing as mp
    assert world <= 3
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q, name)) for r in range(world)]
    for p in procs:
        p.start()
    res, failure, t_end = {}, None, time.monotonic() + limit
    try:
        while len(res) < world and failure is None:
            try:
                rank, ok, payload = q.get(timeout=0.25)
            except queue.Empty:
                dead = [i for i, p in enumerate(procs) if p.exitcode not in (None, 0)]
                if dead:
                    failure = f"rank(s) {dead} died with exit code(s) {[procs[i].exitcode for i in dead]}"
                elif time.monotonic() > t_end:
                    failure = f"no result from ranks {sorted(set(range(world)) - set(res))} after {limit:.0f} s"
                continue
            if ok:
                res[rank] = payload
            else:
                failure = f"rank {rank} failed:\n{payload}"
    finally:
        for p in procs:
            if failure is not None and p.is_alive():
                p.terminate()
        for p in procs:
            p.join(timeout=30)
    assert failure is None, failure
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    _RUNS[key] = [res[r] for r in range(world)]
    return _RUNS[key]
