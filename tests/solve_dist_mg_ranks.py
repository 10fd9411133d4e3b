"""The rank processes of tests/test_gpu_solve_dist_mg.py, in the shape of solve_dist_ranks.py:
run(name, world, extras) starts one process per rank (spawn, gloo on 127.0.0.1, every rank on GPU 0); each assembles its part of
solve_ref_dist.CASES[name] on the GPU and runs a fixed list of multigrid solves across the ranks (ctx.solve_dist with a sized
SolveComm and precond = PRECOND_MULTIGRID), and the block-Jacobi solve of the same rig for comparison."""
import numpy as np

from solve_dist_ranks import SINGULAR_NODE, _view, info_tuple

MG = 3


def _rank_body(rank, world, name, extras):
    import torch
    import solve_ref_dist
    from rdcfes_amd import AssemblyContext, SolveComm
    s = solve_ref_dist.case(name)
    lp = solve_ref_dist.partitions(s, world)[rank]
    loc = solve_ref_dist.local_system(s, lp)
    torch.cuda.set_device(0)
    nloc = lp.xyz.shape[0] * s.nv
    out = dict(n_owned=lp.n_owned, n_interior=lp.n_interior, node_global=lp.node_global)

    class NanBeforeArrival(SolveComm):
        """the ghost tail holds NaN from every begin, sized ones included, until its end delivers"""
        def begin(self, send, recv, stream):
            with torch.cuda.stream(stream):
                recv.fill_(float("nan"))
            return super().begin(send, recv, stream)

        def sized_begin(self, send, recv, send_off, recv_off, stream):
            with torch.cuda.stream(stream):
                recv.fill_(float("nan"))
            return super().sized_begin(send, recv, send_off, recv_off, stream)

    with AssemblyContext(0) as ctx:
        ctx.set_option("interior_nodes", int(lp.n_interior))
        loc.upload(ctx)
        loc.assemble(ctx)
        ctx.synchronize()
        comm = SolveComm(lp, s.nv, "cuda:0", sized=True)

        def solve(x0, c=comm, precond=MG, **kw):
            xd = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)).to("cuda:0")
            torch.cuda.synchronize()
            info = ctx.solve_dist(c, xd.data_ptr(), max_its=kw.pop("max_its", 2000), rhs_scale=s.rhs_scale, precond=precond, **kw)
            return xd.cpu().numpy(), info_tuple(info)

        zeros = np.zeros(nloc)
        for tol in (1e-8, 1e-10):
            c0 = (comm.exchanges, comm.sized_exchanges, comm.allreduces)
            x, info = solve(zeros, rel_tol=tol)
            c1 = (comm.exchanges, comm.sized_exchanges, comm.allreduces)
            x2, info2 = solve(zeros, rel_tol=tol)
            c2 = (comm.exchanges, comm.sized_exchanges, comm.allreduces)
            out[("solve", tol)] = dict(x=x, info=info, repeat_same=x.tobytes() == x2.tobytes() and info == info2,
                                       first_calls=tuple(b - a for a, b in zip(c0, c1)), calls=tuple(b - a for a, b in zip(c1, c2)))
            out[("levels", tol)] = ctx.mg_levels()
            out[("jacobi", tol)] = solve(zeros, precond=2, rel_tol=tol)[1]
        if extras:
            out["mixed"] = dict(zip(("x", "info"), solve(zeros, rel_tol=1e-8, mixed=True)))
            out["nan"] = dict(zip(("x", "info"), solve(zeros, c=NanBeforeArrival(lp, s.nv, "cuda:0", sized=True), rel_tol=1e-10)))
            out["max_its"] = dict(zip(("x", "info"), solve(zeros, rel_tol=1e-10, max_its=3)))
            vptr, rptr = ctx.csr_values_device_ptr()
            n_rows, nnz = ctx.csr_dims()
            rhs_d, val_d = _view(rptr, n_rows), _view(vptr, nnz)
            keep_rhs, keep_val = rhs_d.clone(), val_d.clone()
            if rank == 1:
                rhs_d.zero_()
            out["zero_rhs_rank1"] = dict(zip(("x", "info"), solve(zeros, rel_tol=1e-10)))
            rhs_d.copy_(keep_rhs)
            if rank == 1:
                rp, col = ctx.csr_pattern()
                nv, node = s.nv, SINGULAR_NODE
                idx = np.concatenate([np.arange(rp[node * nv + a], rp[node * nv + a + 1])[col[rp[node * nv + a]:rp[node * nv + a + 1]] // nv == node]
                                      for a in range(nv)])
                assert idx.size == nv * nv
                val_d[torch.from_numpy(idx).to("cuda:0")] = 0.0
            x0 = np.random.default_rng(2 + rank).uniform(size=nloc)
            xs, info = solve(x0, rel_tol=1e-10)
            out["singular"] = dict(x=xs, info=info, owned_untouched=xs[:lp.n_owned * s.nv].tobytes() == x0[:lp.n_owned * s.nv].tobytes())
            val_d.copy_(keep_val)
            torch.cuda.synchronize()
            out["restored"] = dict(zip(("x", "info"), solve(zeros, rel_tol=1e-10)))
    return out


def _rank_main(rank, world, port, q, name, extras):
    import os
    import traceback
    from datetime import timedelta
    import torch.distributed as dist
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
        try:
            out = _rank_body(rank, world, name, extras)
            dist.barrier()
        finally:
            dist.destroy_process_group()
        q.put((rank, True, out))
    except BaseException:
        q.put((rank, False, traceback.format_exc()))


_RUNS = {}


def run(name, world, extras=False, limit=240.0):
    """[per-rank dict] of _rank_body, computed once per (name, world, extras); ends every rank as soon as one has failed or died"""
    key = (name, world, extras)
    if key in _RUNS:
        return _RUNS[key]
    import queue
    import socket
    import time
    import torch.multiprocessing as mp
    assert world <= 3
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, q, name, extras)) for r in range(world)]
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
