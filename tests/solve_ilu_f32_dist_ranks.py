"""The rank processes of tests/test_gpu_solve_ilu_f32_dist.py, beside tests/solve_ilu_dist_ranks.py and of its shape: run(name,
world) starts one process per rank (spawn, gloo on 127.0.0.1, every rank on GPU 0 -- a correctness rig, no measure of speed), each
assembles its part of solve_ref_dist.CASES[name] on the GPU, sets the option "ilu_factor_bits" to 32 and runs partitioned solves
with the rank-local block ILU(0) (PRECOND_ILU0_LOCAL), twice each, with the FP64 and with the fp32 operator; the parent gets, per
rank and scenario, the returned local x, the fields of SolveInfo that must agree across ranks, the callback counts and what the
sweeps streamed.  A rank that raises puts its traceback on the queue; the parent ends the others as soon as one has failed or died."""
import queue
import socket
import traceback
from datetime import timedelta

import numpy as np

from solve_dist_ranks import INFO_FIELDS, info_tuple  # noqa: F401 (the test names the fields through this module)


def _rank_body(rank, world, name):
    import torch
    import solve_ref_dist
    from rdcfes_amd import AssemblyContext, SolveComm
    from rdcfes_amd.context import PRECOND_ILU0_LOCAL
    s = solve_ref_dist.case(name)
    lp = solve_ref_dist.partitions(s, world)[rank]
    loc = solve_ref_dist.local_system(s, lp)
    torch.cuda.set_device(0)
    nloc = lp.xyz.shape[0] * s.nv
    out = dict(n_owned=lp.n_owned, n_interior=lp.n_interior, node_global=lp.node_global)
    with AssemblyContext(0) as ctx:
        ctx.set_option("interior_nodes", int(lp.n_interior))
        ctx.set_option("ilu_factor_bits", 32)
        loc.upload(ctx)
        loc.assemble(ctx)
        ctx.synchronize()
        comm = SolveComm(lp, s.nv, "cuda:0")

        def solve(**kw):
            xd = torch.zeros(nloc, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            e0, a0 = comm.exchanges, comm.allreduces
            info = ctx.solve_dist(comm, xd.data_ptr(), max_its=2000, rhs_scale=s.rhs_scale, precond=PRECOND_ILU0_LOCAL, **kw)
            return dict(x=xd.cpu().numpy(), info=info_tuple(info), calls=(comm.exchanges - e0, comm.allreduces - a0), bits=ctx.ilu_factor_bits())

        for tol in (1e-8, 1e-10):
            for mixed in (False, True):
                a, b = solve(rel_tol=tol, mixed=mixed), solve(rel_tol=tol, mixed=mixed)
                a["repeat_same"] = a["x"].tobytes() == b["x"].tobytes() and a["info"] == b["info"] and a["calls"] == b["calls"]
                out[("mixed" if mixed else "ilu", tol)] = a
        out["ilu_stats"] = ctx.ilu_stats()
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
