"""The rank processes of tests/test_gpu_solve_mg_gs_dist.py, in the shape of solve_dist_mg_ranks.py: run(name, world) starts one
process per rank (spawn, gloo on 127.0.0.1, every rank on GPU 0 -- a correctness rig, no measure of speed); each assembles its part
of solve_ref_dist.CASES[name] on the GPU and runs, through ONE SolveComm(..., sized=True, wide=True):

  solves   (SOLVES_ON) precond 6 with BiCGStab (ctx.solve_dist) and GMRES (ctx.solve_dist_gmres), at both tolerances, under
           "mg_gs_fuse" = 1 and 0, twice each: the local x, the fields of SolveInfo, the callback counts of the first and the second
           solve, mg_levels() and mg_colours(); and precond 3 on the same rig, for its iteration and callback counts;
  arnoldi  (ARNOLDI_ON) rdc_solve_dist_gmres_arnoldi, ONE step, precond 6, FP64 and mixed, under both values of "mg_gs_fuse", from the
           rhs and from a seeded random vector, and the system this rank assembled, downloaded;
  extras   (EXTRAS_ON) the mixed solve; the solve under a communicator that keeps NaN in every ghost tail between begin and end,
           "mg_gs_fuse" = 0; what a new plan does to the colours; the refusals; a singular diagonal block on rank 1; max_its = 3."""
import queue
import socket
import traceback
from datetime import timedelta

import numpy as np

from solve_dist_ranks import INFO_FIELDS, SINGULAR_NODE, _view, info_tuple  # noqa: F401 (the test names the fields through this module)

GS, MG = 6, 3
TOLS = (1e-8, 1e-10)
SOLVES_ON = {("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("pihna_kuhn3", 3)}
ARNOLDI_ON = {("pihna_kuhn", 2), ("pihna_kuhn", 3), ("hcc_hex", 2), ("hcc_hex", 3)}
EXTRAS_ON = {("pihna_kuhn", 2)}
ARNOLDI_SEED = 23


def random_start(n_global_dofs):
    """the seeded random start of the Arnoldi runs, in the global numbering; a rank takes the rows it owns"""
    return np.random.default_rng(ARNOLDI_SEED).standard_normal(n_global_dofs)


def _rank_body(rank, world, name):
    import ctypes as C
    import torch
    import solve_ref_dist
    from rdcfes_amd import AssemblyContext, RdcError, SolveComm, SolveInfo, SolveParams
    s = solve_ref_dist.case(name)
    lp = solve_ref_dist.partitions(s, world)[rank]
    loc = solve_ref_dist.local_system(s, lp)
    torch.cuda.set_device(0)
    nv = s.nv
    nloc, nown = lp.xyz.shape[0] * nv, lp.n_owned * nv
    out = dict(n_owned=lp.n_owned, n_interior=lp.n_interior, node_global=lp.node_global, n_nodes=lp.xyz.shape[0])

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
        comm = SolveComm(lp, nv, "cuda:0", sized=True, wide=True)

        def counts(c):
            return (c.exchanges, c.sized_exchanges, c.allreduces, c.wide_allreduces)

        def solve(x0, method="bicgstab", c=comm, **kw):
            xd = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)).to("cuda:0")
            torch.cuda.synchronize()
            before = counts(c)
            fn = ctx.solve_dist if method == "bicgstab" else ctx.solve_dist_gmres
            info = fn(c, xd.data_ptr(), max_its=kw.pop("max_its", 2000), rhs_scale=s.rhs_scale, **kw)
            return dict(x=xd.cpu().numpy(), info=info_tuple(info), calls=tuple(a - b for a, b in zip(counts(c), before)))

        def refused(fn):
            """(error code, message, callbacks made, x untouched) of a call that must raise"""
            x0 = np.random.default_rng(5 + rank).uniform(size=nloc)
            xd = torch.from_numpy(x0.copy()).to("cuda:0")
            torch.cuda.synchronize()
            before = counts(comm)
            try:
                fn(xd)
            except RdcError as e:
                return dict(code=e.code, message=str(e), calls=tuple(a - b for a, b in zip(counts(comm), before)),
                            untouched=xd.cpu().numpy().tobytes() == x0.tobytes())
            return dict(code=0, message="", calls=None, untouched=False)

        zeros = np.zeros(nloc)
        if (name, world) in SOLVES_ON:
            for method in ("bicgstab", "gmres"):
                for tol in TOLS:
                    for fuse in (1, 0):
                        ctx.set_option("mg_gs_fuse", fuse)
                        a = solve(zeros, method, rel_tol=tol, precond=GS)
                        b = solve(zeros, method, rel_tol=tol, precond=GS)
                        a["repeat_same"] = a["info"] == b["info"] and a["x"].tobytes() == b["x"].tobytes()
                        a["calls_first"], a["calls"] = a["calls"], b["calls"]   # the very first solve also builds the hierarchy
                        a["levels"], a["colours"] = ctx.mg_levels(), ctx.mg_colours()
                        out[(method, tol, fuse)] = a
                    ctx.set_option("mg_gs_fuse", 1)
                    ctx.set_option("mg_smoother", 1)      # not consulted under precond 6
                    c = solve(zeros, method, rel_tol=tol, precond=GS)
                    out[(method, tol, "smoother1_same")] = c["x"].tobytes() == out[(method, tol, 1)]["x"].tobytes() and c["info"] == out[(method, tol, 1)]["info"]
                    ctx.set_option("mg_smoother", 0)
                    j = solve(zeros, method, rel_tol=tol, precond=MG)
                    out[(method, tol, "jacobi")] = dict(info=j["info"], calls=j["calls"])
        if (name, world) in ARNOLDI_ON:
            val, rhs = ctx.csr_download()
            rp, col = ctx.csr_pattern()
            out["system"] = dict(rp=rp, col=col, val=val, rhs=rhs)
            dofs = (lp.node_global[:lp.n_owned].astype(np.int64)[:, None] * nv + np.arange(nv)).reshape(-1)
            starts = dict(rhs=s.rhs_scale * rhs, random=random_start(s.xyz.shape[0] * nv)[dofs])
            for mixed in (False, True):
                for label, v0 in starts.items():
                    got = {}
                    for fuse in (1, 0):
                        ctx.set_option("mg_gs_fuse", fuse)
                        before = counts(comm)
                        V, H = ctx.gmres_arnoldi_dist(comm, v0, 1, GS, mixed=mixed)
                        got[fuse] = dict(V=V, H=H, calls=tuple(a - b for a, b in zip(counts(comm), before)))
                    got[1]["fuse0_same"] = got[0]["V"].tobytes() == got[1]["V"].tobytes() and got[0]["H"].tobytes() == got[1]["H"].tobytes()
                    got[1]["calls"] = got[0]["calls"]   # of the second call: the very first one may also build the hierarchy
                    out[("arnoldi", mixed, label)] = got[1]
            ctx.set_option("mg_gs_fuse", 1)
            v, r = ctx.csr_download()
            out["system"]["unchanged"] = v.tobytes() == val.tobytes() and r.tobytes() == rhs.tobytes()
        if (name, world) in EXTRAS_ON:
            out["mixed"] = solve(zeros, rel_tol=1e-8, precond=GS, mixed=True)
            out["mixed_jacobi"] = solve(zeros, rel_tol=1e-8, precond=MG, mixed=True)
            # a new communicator is a new plan: the hierarchy and this rank's colours go and are built again
            ctx.set_option("mg_gs_fuse", 0)
            out["nan"] = solve(zeros, c=NanBeforeArrival(lp, nv, "cuda:0", sized=True, wide=True), rel_tol=1e-10, precond=GS)
            out["nan"]["colours"] = ctx.mg_colours()
            ctx.set_option("mg_gs_fuse", 1)
            ctx.solve_dist_plan(comm.send_nodes)      # a plan alone: no hierarchy, no colours
            ctx._dist_plan = None
            codes = []
            for fn in (ctx.mg_levels, ctx.mg_colours):
                try:
                    fn()
                    codes.append(0)
                except RdcError as e:
                    codes.append(e.code)
            out["after_plan"] = codes
            out["replanned"] = solve(zeros, rel_tol=1e-10, precond=GS)
            out["replanned"]["colours"] = ctx.mg_colours()
            out["max_its"] = solve(zeros, rel_tol=1e-10, precond=GS, max_its=3)
            # refusals: none makes a callback, so no rank waits for another
            p = SolveParams(1e-8, 0.0, s.rhs_scale, 100, GS)

            def plain_dist(xd):
                info = SolveInfo()
                ctx._ck(ctx._lib.rdc_solve_dist(ctx._h, C.byref(p), C.byref(comm.struct), 0, C.c_void_p(xd.data_ptr()), C.byref(info)))
            out["refused_dist"] = refused(plain_dist)
            out["refused_solve"] = refused(lambda xd: ctx.solve(xd.data_ptr(), precond=GS, rhs_scale=s.rhs_scale))
            ctx.set_option("mg_smoother", 1)
            out["refused_mg_smoother1"] = refused(lambda xd: ctx.solve_dist(comm, xd.data_ptr(), precond=MG, rhs_scale=s.rhs_scale))
            out["refused_gmres_smoother1"] = refused(lambda xd: ctx.solve_dist_gmres(comm, xd.data_ptr(), precond=MG, rhs_scale=s.rhs_scale))
            ctx.set_option("mg_smoother", 0)
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
            out["singular"] = solve(x0, rel_tol=1e-10, precond=GS)
            out["singular"]["owned_untouched"] = out["singular"]["x"][:nown].tobytes() == x0[:nown].tobytes()
            val_d.copy_(keep_val)
            torch.cuda.synchronize()
            out["restored"] = solve(zeros, rel_tol=1e-10, precond=GS)
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
    """[per-rank dict] of _rank_body, computed once per (name, world); ends every rank as soon as one has failed or died"""
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
