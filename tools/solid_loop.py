#!/usr/bin/env python3
"""Load steps of the hyperelastic solid on H(n) that never leave the card: the uniaxial compression of the shipped cube case
(side z = 0 held, side z = 1 pushed down by 0.75 * pseudo_time, penalty 1e8, the Hyperelastic defaults) on the unit cube of n^3
HEX8, pseudo_time = 0.1, 0.2, ... from the undeformed mesh, every step one rdc_solid_newton with the shipped solver options.

    python tools/solid_loop.py --n 126 --steps 3 [--precond 2|3|4] [--mixed] [--rel-tol 1e-3] [--ab newton|dist]
    python tools/solid_loop.py --n 32 --steps 3 --ranks 2 [--backend gloo|nccl] [--precond 2|3|5|6]

The device loop prints one record per load step with what the call itself measures, since nothing comes back in between: wall ms
and device ms of the whole call, the device ms of every assembly in it (rdc_timing_samples_ms), per iteration the linear
iterations and ||R||, and per Newton iteration the wall ms, the assembly ms and the remainder (the linear solve and the rest).

--ab newton runs the same load steps from the same state in one process in the order device, composed, composed, device.
"composed" is the loop the library call replaces, made of the existing calls with the hand-back of the host mirror's solve():
solid_assemble, a full csr_download (matrix and rhs), the norm of the rhs in numpy, solve(rhs_scale=-1) into a device vector,
mesh_update_coords.  Its per-iteration record splits the wall time into assembly, hand-back, solve and the rest.

--ranks N: one process per rank (recursive coordinate bisection, one ghost layer, interior nodes first; side list and materials
restricted to the local elements), every load step one rdc_solid_newton_dist through a halo.SolveComm; rank 0 prints one record per
step (info and history are global; the times are rank 0's own).  Rank r uses GPU r modulo the number of GPUs: on a one-GPU machine
the ranks share it, and with --backend gloo every message is staged through the host -- such a run checks correctness and measures
nothing.  --ranks 1 is the partitioned entry at world size 1 in this process; --ab dist runs the load steps in the order
rdc_solid_newton, rdc_solid_newton_dist at world size 1, the same again, rdc_solid_newton: what the entry costs over the plain one."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402


def build_case(n):
    from rdcfes_amd import SolidMaterial, synth
    conn, X = synth.hex_mesh(n)
    e0, s0 = synth.boundary_sides(8, conn, X, 2, 0.0)
    e1, s1 = synth.boundary_sides(8, conn, X, 2, 1.0)
    side_elem = np.concatenate([e0, e1]).astype(np.int64)
    side_id = np.concatenate([s0, s1]).astype(np.int32)
    disp = np.concatenate([np.zeros((len(e0), 3)), np.tile([np.nan, np.nan, -0.75], (len(e1), 1))])
    mats = [SolidMaterial(1.0e3, 0.3, 0.0, (0.0, 0.0, 0.0))]   # the defaults input() takes for the shipped file (its keys are not the ones read)
    return conn, X, (side_elem, side_id, disp), mats


def open_context(case):
    from rdcfes_amd import AssemblyContext
    from rdcfes_amd.context import FIELD_ELEM_FIBRE, FIELD_UNDEFORMED_XYZ
    conn, X, sides, mats = case
    ctx = AssemblyContext(0)
    ctx.mesh_upload(8, conn, X, 3)
    ctx.field_upload(FIELD_UNDEFORMED_XYZ, X)
    ctx.field_upload(FIELD_ELEM_FIBRE, np.tile([0.0, 0.0, 1.0], (conn.shape[0], 1)))
    ctx.solid_set_materials(np.zeros(conn.shape[0], dtype=np.int32), mats)
    ctx.solid_set_sides(*sides)
    return ctx


def world1_comm(X):
    """the communicator of world size 1 for a context without ghosts: no peers, an empty send list"""
    from types import SimpleNamespace
    from rdcfes_amd import SolveComm
    return SolveComm(SimpleNamespace(rank=0, send_ids={}, recv_ids={}, xyz=X, n_owned=X.shape[0]), 3, "cuda:0", sized=True, wide=True)


def device_steps(ctx, X, a, opt, comm=None):
    """the load steps with rdc_solid_newton, or with rdc_solid_newton_dist through comm -> one record per step"""
    from rdcfes_amd import SolidParams
    ctx.mesh_update_coords(X)
    out = []
    for k in range(1, a.steps + 1):
        sp = SolidParams(0.1 * k, 1.0e8, 0, 0)
        ctx.timing_enable(True)
        t0 = time.perf_counter()
        if comm is None:
            info = ctx.solid_newton(sp, precond=a.precond, mixed=a.mixed, **opt)
        else:
            info = ctx.solid_newton_dist(comm, sp, precond=a.precond, mixed=a.mixed, **opt)
        wall = 1e3 * (time.perf_counter() - t0)
        asm = ctx.timing_samples_ms()
        ctx.timing_enable(False)
        res, step, its, reason = ctx.solid_newton_history()
        nl = max(info.nonlinear_iterations, 1)
        out.append(dict(path="device" if comm is None else "dist", step=k, reason=info.reason, newton_iterations=info.nonlinear_iterations, assemblies=info.assemblies,
                        linear_iterations=[int(v) for v in its], residuals=[float(v) for v in res] + [info.last_residual],
                        wall_ms=wall, device_ms=info.device_ms, assembly_ms=[round(float(v), 3) for v in asm],
                        per_iteration_ms=wall / nl, per_iteration_assembly_ms=float(np.sum(asm)) / nl,
                        per_iteration_rest_and_solve_ms=(wall - float(np.sum(asm))) / nl))
    return out


def composed_steps(ctx, X, a, opt):
    """the same load steps with the existing calls and the full hand-back of the host mirror's solve()"""
    import torch
    from rdcfes_amd import SolidParams
    ctx.mesh_update_coords(X)
    u = np.array(X, copy=True)
    delta = torch.zeros(u.size, dtype=torch.float64, device="cuda:0")
    out = []
    for k in range(1, a.steps + 1):
        sp = SolidParams(0.1 * k, 1.0e8, 0, 0)
        rec = dict(path="composed", step=k, iterations=[], reason=None)
        t_step = time.perf_counter()
        it, first = 0, None
        while True:
            t0 = time.perf_counter()
            ctx.timing_enable(True)
            ctx.solid_assemble(sp, True)
            ctx.synchronize()
            asm = ctx.timing_last_ms()
            ctx.timing_enable(False)
            t1 = time.perf_counter()
            val, rhs = ctx.csr_download()                     # the whole matrix and the rhs, as SolidSystem::assembly hands them back
            rn = float(np.linalg.norm(rhs))
            del val
            t2 = time.perf_counter()
            first = rn if first is None else first
            if rn <= opt["absolute_residual_tolerance"] or rn <= opt["relative_residual_tolerance"] * first:
                rec["reason"] = 0
            elif it >= opt["max_nonlinear_iterations"]:
                rec["reason"] = 2
            if rec["reason"] is not None:
                rec["closing"] = dict(residual=rn, assembly_ms=asm, handback_ms=1e3 * (t2 - t1))
                break
            delta.zero_()
            torch.cuda.synchronize()
            li = ctx.solve(delta.data_ptr(), rel_tol=opt["rel_tol"], max_its=opt["max_its"], precond=a.precond, rhs_scale=-1.0, mixed=a.mixed)
            t3 = time.perf_counter()
            d = delta.cpu().numpy().reshape(u.shape)
            u = u + d
            ctx.mesh_update_coords(u)
            t4 = time.perf_counter()
            rec["iterations"].append(dict(residual=rn, assembly_ms=asm, handback_ms=1e3 * (t2 - t1), solve_ms=li.device_ms,
                                          rest_ms=1e3 * (t4 - t0) - asm - 1e3 * (t2 - t1) - li.device_ms, linear_iterations=li.iterations,
                                          wall_ms=1e3 * (t4 - t0)))
            it += 1
            if float(np.linalg.norm(d)) <= opt["relative_step_tolerance"] * float(np.linalg.norm(u)):
                rec["reason"] = 1                              # by step; the closing residual-only assembly is not timed here
                break
        rec["newton_iterations"] = it
        rec["wall_ms"] = 1e3 * (time.perf_counter() - t_step)
        rec["per_iteration_ms"] = rec["wall_ms"] / max(it, 1)
        out.append(rec)
    return out


def rank_main(rank, world, port, a, opt):
    """one rank of --ranks"""
    import os
    from datetime import timedelta
    import torch
    import torch.distributed as dist
    from rdcfes_amd import AssemblyContext, SolveComm, partition
    from rdcfes_amd.context import FIELD_ELEM_FIBRE, FIELD_UNDEFORMED_XYZ
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    gpu = rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(gpu)
    dist.init_process_group(a.backend, rank=rank, world_size=world, timeout=timedelta(seconds=300))
    try:
        conn, X, (se, ss, sd), mats = build_case(a.n)
        part = partition.partition_rcb(X[conn.astype(np.int64)].mean(axis=1), world)
        lp = partition.build_local(conn, X, part, rank, world)
        eg = np.asarray(lp.elem_global, dtype=np.int64)
        g2l = np.full(conn.shape[0], -1, dtype=np.int64)
        g2l[eg] = np.arange(eg.size)
        keep = g2l[se] >= 0                                              # boundary sides of the local elements
        ctx = AssemblyContext(gpu)
        ctx.set_option("interior_nodes", int(lp.n_interior))
        ctx.mesh_upload(8, lp.conn, lp.xyz, 3, n_owned=lp.n_owned)
        ctx.field_upload(FIELD_UNDEFORMED_XYZ, lp.xyz)
        ctx.field_upload(FIELD_ELEM_FIBRE, np.tile([0.0, 0.0, 1.0], (eg.size, 1)))
        ctx.solid_set_materials(np.zeros(eg.size, dtype=np.int32), mats)
        ctx.solid_set_sides(g2l[se[keep]], ss[keep], sd[keep])
        comm = SolveComm(lp, 3, f"cuda:{gpu}", sized=True, wide=True)
        shared = world > max(torch.cuda.device_count(), 1)
        if rank == 0:
            print(json.dumps(dict(n=a.n, ranks=world, backend=a.backend, nodes=int(X.shape[0]), owned=int(lp.n_owned), ghosts=int(lp.xyz.shape[0] - lp.n_owned),
                                  neighbours=len(comm.send_peers), precond=a.precond, mixed=a.mixed,
                                  timing="correctness only: ranks share a GPU or stage through the host" if shared or a.backend == "gloo" else "device",
                                  **opt)), flush=True)
        with ctx:
            for r in device_steps(ctx, lp.xyz, a, opt, comm):
                if rank == 0:
                    print(json.dumps(dict(r, exchanges=comm.exchanges, allreduces=comm.allreduces)), flush=True)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=126)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--precond", type=int, default=2)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--rel-tol", type=float, default=1e-3, help="solver/linear/initial_linear_tolerance")
    ap.add_argument("--max-its", type=int, default=50000, help="solver/linear/max_linear_iterations")
    ap.add_argument("--ab", choices=["newton", "dist"])
    ap.add_argument("--ranks", type=int, default=None)
    ap.add_argument("--backend", choices=("gloo", "nccl"), default="gloo")
    a = ap.parse_args()
    if a.ranks is not None and (a.ranks < 1 or a.ab):
        ap.error("--ranks N >= 1, without --ab (--ab dist is the comparison at world size 1)")
    if a.precond == 4 and (a.ranks is not None or a.ab == "dist"):
        ap.error("the block ILU(0) (--precond 4) is rdc_solid_newton only; across ranks: --precond 5")
    opt = dict(max_nonlinear_iterations=10, require_reduction=False, relative_step_tolerance=1e-3, relative_residual_tolerance=1e-8,
               absolute_residual_tolerance=1e-8, rel_tol=a.rel_tol, max_its=a.max_its)
    if a.ranks is not None and a.ranks > 1:
        import socket
        import torch.multiprocessing as mp
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        mp.spawn(rank_main, args=(a.ranks, port, a, opt), nprocs=a.ranks, join=True)
        return
    import torch
    torch.cuda.init()                       # before the library opens the device: one runtime initialisation order for both
    t0 = time.perf_counter()
    case = build_case(a.n)
    ctx = open_context(case)
    X = case[1]
    print(json.dumps(dict(n=a.n, nodes=int(X.shape[0]), rows=int(3 * X.shape[0]), elements=int(case[0].shape[0]), nnz=int(ctx.csr_dims()[1]),
                          matrix_gb=ctx.csr_dims()[1] * 8 / 1e9, precond=a.precond, mixed=a.mixed, setup_s=time.perf_counter() - t0, **opt)), flush=True)
    with ctx:
        legs = {"newton": ["device", "composed", "composed", "device"], "dist": ["device", "dist", "dist", "device"]}.get(a.ab, ["device"])
        if a.ranks == 1:
            legs = ["dist"]
        comm = world1_comm(X) if "dist" in legs else None
        mean = {}
        for leg in legs:
            recs = composed_steps(ctx, X, a, opt) if leg == "composed" else device_steps(ctx, X, a, opt, comm if leg == "dist" else None)
            for r in recs:
                print(json.dumps(r), flush=True)
            its = sum(r["newton_iterations"] for r in recs)
            mean.setdefault(leg, []).append(sum(r["wall_ms"] for r in recs) / max(its, 1))
        print(json.dumps(dict(summary="wall ms per Newton iteration, per leg in run order", **mean)), flush=True)


if __name__ == "__main__":
    main()
