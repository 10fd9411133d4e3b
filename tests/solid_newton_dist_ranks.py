"""The rank processes of tests/test_gpu_solid_newton_dist.py, of the shape of tests/solve_dist_gmres_ranks.py: run(name, world)
starts one process per rank (spawn, gloo on 127.0.0.1, every rank on GPU 0 -- a correctness rig, no measure of speed), each uploads
its part of a shipped solid case (solid_newton_ref.system: "cube" | "hydrogel", split by solve_ref_dist.partitions) and runs
rdc_solid_newton_dist through a SolveComm.  Everything of one (name, world) happens in that one spawn; the parent compares.

Every run starts from the undeformed mesh on the owned rows and from WRONG ghost coordinates (shifted by GHOST_SHIFT): the entry
ignores the ghost rows it is given.  A run returns the fields of info that must agree across ranks, the history, the local
coordinates and the rhs the context holds behind the call.

  tight     TIGHT options, linear 1e-10, block Jacobi, at every pseudo_time of PSEUDO_TIMES[name]
  inexact   (world 2) the shipped options at the same pseudo_times
  world 2, cube only:
  callbacks a LoggingComm around the tight runs at 0.1 with BiCGStab and with GMRES, and around the halving case
  halving   pseudo_time 1.5, require_reduction, HALVING_CAP iterations
  through   precond 5, 3, 6, mixed with precond 2, GMRES with precond 2 and 5, at 0.1
  refusals  precond 4; precond 3 without the sized pair; GMRES without the wide all-reduce; no plan; bad parameters
  abort     the second all-reduce of 8 doubles returns 1 on every rank; then the tight run again on the same context

A rank that raises puts its traceback on the queue; the parent ends the others as soon as one has failed or died."""
import copy
import queue
import socket
import traceback
from datetime import timedelta

import numpy as np

GHOST_SHIFT = 0.25
TIGHT = dict(max_nonlinear_iterations=10, require_reduction=False, relative_step_tolerance=0.0, relative_residual_tolerance=1e-8,
             absolute_residual_tolerance=1e-8)
PSEUDO_TIMES = {"cube": (0.1, 1.0), "hydrogel": (0.1,)}
INFO_FIELDS = ("reason", "nonlinear_iterations", "linear_iterations", "assemblies", "halvings", "last_linear_reason", "first_residual",
               "last_residual", "last_step_norm", "last_solution_norm")   # everything but device_ms, which is a rank's own
THROUGH = {"ilu_local": dict(precond=5), "multigrid": dict(precond=3), "multigrid_gs_local": dict(precond=6), "mixed": dict(precond=2, mixed=True),
           "gmres": dict(precond=2, gmres=True), "gmres_ilu_local": dict(precond=5, gmres=True)}
FIELD_UNDEFORMED_XYZ, FIELD_ELEM_FIBRE = 2, 3


def info_tuple(info):
    return tuple(getattr(info, f) for f in INFO_FIELDS)


def local_solid(s, lp):
    """the solid System of one rank: local mesh, nodal fields of its nodes, element fields, materials and sides of its elements"""
    loc = copy.copy(s)
    loc.name = f"{s.name}_r{lp.rank}of{lp.nparts}"
    loc.conn, loc.xyz, loc.n_owned = lp.conn, lp.xyz, lp.n_owned
    eg = np.asarray(lp.elem_global, dtype=np.int64)
    loc.fields = {FIELD_UNDEFORMED_XYZ: np.ascontiguousarray(s.fields[FIELD_UNDEFORMED_XYZ][lp.node_global]),
                  FIELD_ELEM_FIBRE: np.ascontiguousarray(s.fields[FIELD_ELEM_FIBRE][eg])}
    g2l = np.full(s.conn.shape[0], -1, dtype=np.int64)
    g2l[eg] = np.arange(eg.size)
    se, ss, sd = s.solid["sides"]
    keep = g2l[np.asarray(se, dtype=np.int64)] >= 0                      # boundary sides of the local elements
    loc.solid = dict(em=np.ascontiguousarray(np.asarray(s.solid["em"])[eg]), mats=s.solid["mats"],
                     sides=(g2l[np.asarray(se, dtype=np.int64)[keep]], np.asarray(ss)[keep], np.asarray(sd)[keep]))
    return loc


def _rank_body(rank, world, name):
    import torch
    import solid_newton_ref as N
    import solve_ref_dist
    from rdcfes_amd import AssemblyContext, RdcError, SolveComm
    from test_solid_newton_ref import HALVING_CAP
    s = N.system(name)
    lp = solve_ref_dist.partitions(s, world)[rank]
    loc = local_solid(s, lp)
    torch.cuda.set_device(0)
    n_loc, n_own = lp.xyz.shape[0], lp.n_owned
    assert 0 < lp.n_interior and n_own < n_loc and loc.solid["sides"][0].size > 0    # interior nodes, ghosts and sides on every rank
    out = dict(n_owned=n_own, n_nodes=n_loc, node_global=np.asarray(lp.node_global), ghosts_of={q: np.asarray(v) for q, v in lp.recv_ids.items()},
               sends_to={q: np.asarray(v) for q, v in lp.send_ids.items()})
    x_start = np.ascontiguousarray(lp.xyz).copy()
    x_start[n_own:] += GHOST_SHIFT

    class LoggingComm(SolveComm):
        """logs every callback in order -- ("exchange", d_recv address), ("allreduce", n), ("sized",), ("wide", n) -- keeps the send buffer
        of the first exchange, and returns 1 from the fail_at-th all-reduce of 8 doubles"""
        def __init__(self, *a, fail_at=None, **kw):
            super().__init__(*a, **kw)
            self.log, self.first_send, self.fail_at, self.n8 = [], None, fail_at, 0

        def _c_begin(self, user, d_send, d_recv, stream):
            if not any(e[0] == "exchange" for e in self.log):
                with torch.cuda.stream(self._stream(stream)):
                    self.first_send = self._view(d_send, self.n_send).clone()
            self.log.append(("exchange", int(d_recv or 0)))
            return super()._c_begin(user, d_send, d_recv, stream)

        def _c_allreduce(self, user, d_vals, n, stream):
            self.log.append(("allreduce", int(n)))
            if n == 8:
                self.n8 += 1
                if self.n8 == self.fail_at:
                    return 1
            return super()._c_allreduce(user, d_vals, n, stream)

        def _c_sized_begin(self, *a):
            self.log.append(("sized",))
            return super()._c_sized_begin(*a)

        def _c_allreduce_wide(self, user, d_vals, n, stream):
            self.log.append(("wide", int(n)))
            return super()._c_allreduce_wide(user, d_vals, n, stream)

    with AssemblyContext(0) as ctx:
        ctx.set_option("interior_nodes", int(lp.n_interior))
        loc.upload(ctx)
        comm = SolveComm(lp, 3, "cuda:0", wide=True)
        tail = ctx.coords_device_ptr() + 8 * 3 * n_own          # where the ghost coordinates lie

        def coords():
            return ctx.coords_tensor().cpu().numpy().copy()

        def run(pt, c=comm, gmres=False, rel_tol=1e-10, max_its=50000, **kw):
            ctx.set_option("solve_method", 1 if gmres else 0)
            ctx.mesh_update_coords(x_start)
            info = ctx.solid_newton_dist(c, N.at(s, pt).params, rel_tol=rel_tol, max_its=max_its, **kw)
            ctx.set_option("solve_method", 0)
            res, step, its, reason = ctx.solid_newton_history()
            _, rhs = ctx.csr_download(want_val=False)
            return dict(info=info_tuple(info), residuals=res, steps=step, lin_its=its, lin_reasons=reason, xyz=coords(), rhs=rhs,
                        device_ms=info.device_ms)

        def logged(r, c):
            sent = c.first_send.cpu().numpy() if c.first_send is not None else None
            r.update(log=list(c.log), first_send=sent, tail=tail, want_send=np.ascontiguousarray(lp.xyz)[c.send_nodes])
            return r

        for pt in PSEUDO_TIMES[name]:
            out[("tight", pt)] = run(pt, **TIGHT)
        if world == 2:
            for pt in PSEUDO_TIMES[name]:
                opt = N.shipped_options(name)
                out[("inexact", pt)] = run(pt, rel_tol=opt.pop("rel_tol"), max_its=opt.pop("max_its"), **opt)
        if world == 2 and name == "cube":
            for label, gm in (("bicgstab", False), ("gmres", True)):
                c = LoggingComm(lp, 3, "cuda:0", wide=True)
                out[("callbacks", label)] = logged(run(0.1, c=c, gmres=gm, **TIGHT), c)
            c = LoggingComm(lp, 3, "cuda:0", wide=True)
            out["halving"] = logged(run(1.5, c=c, **dict(TIGHT, require_reduction=True, max_nonlinear_iterations=HALVING_CAP)), c)
            for label, kw in THROUGH.items():
                out[("through", label)] = run(0.1, **dict(TIGHT, **kw))

            # -- refusals: (code, callbacks made, owned coordinates unchanged bitwise)
            def refused(c, fresh=None, **kw):
                target = fresh or ctx
                target.mesh_update_coords(x_start)
                gm = kw.pop("gmres", False)
                target.set_option("solve_method", 1 if gm else 0)
                code = None
                opt = dict(TIGHT, rel_tol=1e-10, max_its=50000)
                opt.update(kw)
                try:
                    target.solid_newton_dist(c, N.at(s, 0.1).params, **opt)
                except RdcError as e:
                    code = e.code
                target.set_option("solve_method", 0)
                own = target.coords_tensor().cpu().numpy()[:n_own]
                return dict(code=code, log=list(c.log), owned_unchanged=own.tobytes() == x_start[:n_own].tobytes())

            mk = lambda **kw: LoggingComm(lp, 3, "cuda:0", **kw)
            ref = {}
            ref["precond4"] = refused(mk(wide=True), precond=4)
            ref["mg_without_sized"] = refused(mk(), precond=3)
            ref["gmres_without_wide"] = refused(mk(sized=True), gmres=True)
            for label, bad in (("its0", dict(max_nonlinear_iterations=0)), ("its1001", dict(max_nonlinear_iterations=1001)),
                               ("nan", dict(relative_step_tolerance=float("nan"))), ("negative", dict(absolute_residual_tolerance=-1.0)),
                               ("precond17", dict(precond=17)), ("max_its0", dict(max_its=0))):
                ref[("bad", label)] = refused(mk(wide=True), **bad)
            with AssemblyContext(0) as fresh:         # a ghosted context that never got a send list
                loc.upload(fresh)
                c = mk(wide=True)
                fresh._dist_plan = c                  # the wrapper believes the plan of c is uploaded: the library is asked without one
                ref["no_plan"] = refused(c, fresh=fresh)
            out["refusals"] = ref

            # -- abort: the second all-reduce of the loop fails on every rank alike, so that no rank waits for another
            bad = LoggingComm(lp, 3, "cuda:0", wide=True, fail_at=2)
            ab = refused(bad)
            ab.update(last=bad.log[-1], n8=bad.n8, finite=bool(np.isfinite(coords()).all()), moved=not ab["owned_unchanged"])
            out["abort"] = ab
            out["after_abort"] = run(0.1, **TIGHT)    # run() uploads the coordinates again
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
