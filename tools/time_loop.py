"""PIHNA time loop that never leaves the card: k steps of assemble -> solve (initial guess = old solution, in place in
the storage of FIELD_OLD_SOLUTION) -> clamp_nonnegative on a Kuhn mesh K(n), shipped parameters, synth.pihna_fields.

    python tools/time_loop.py --n 119 --steps 5 [--rel-tol 1e-8] [--precond 2|3|4|5|6] [--mixed] [--smoother 0|1] [--gs-fuse 0|1]
                              [--ilu-bits 32|64] [--method bicgstab|gmres] [--restart N]
                              [--ab [precond|precision|dist|smoother|ilu_bits|method]] [--dump DIR]
    python tools/time_loop.py --n 32 --steps 3 --ranks 2 [--backend gloo|nccl] [--precond 2|3|5|6] [--method bicgstab|gmres] [--restart N]
                              [--ab precond|method|smoother]

Per step: assembly ms (rdc_timing_last_ms), solve ms (device time of rdc_solve), iterations, restarts, the true
preconditioned residual, and the share of nodes / elements still in the exact background state (n = c = h = a = 0),
counted on the device after the clamp.  --mixed solves with rdc_solve_mixed (the iteration streams an fp32 copy of D^-1 A;
matrix_bits in every record says what ran).  --precond 3 is the aggregation-multigrid preconditioner: every record then also has
the device ms the solve spent building the hierarchy (mg_setup_ms, part of solve_ms), its level sizes and the device bytes it
holds.  --precond 4 is the multicolour block ILU(0): every record then has the device ms the solve spent on the copy of D^-1 A and
its factorisation (ilu_setup_ms, part of solve_ms), the device bytes the factor holds and the colours; FP64 and one partition only.
--precond 5 is its rank-local form (the ILU(0) of every rank's owned square: block Jacobi between the ranks, ILU(0) inside each), the
one --ranks takes, with the same three figures per record (rank 0's own); on one partition it runs what --precond 4 runs.
--ab runs the loop several times from the same initial state on one upload, so that the kinds of solve are timed in one
process on one device: --ab (= --ab precond) in the order block Jacobi, multigrid, ILU(0), ILU(0), multigrid, block Jacobi (fp64; with
--mixed, which has no ILU(0), block Jacobi, multigrid, multigrid, block Jacobi); --ab precision in the order fp64, mixed, mixed, fp64 with --precond; --ab dist in the order rdc_solve,
rdc_solve_dist, rdc_solve_dist, rdc_solve, the partitioned entry at world size 1 (its exchange moves nothing and its all-reduce
leaves the values alone: what is timed is the pack launches, the k_reduce / k_advance split and the callbacks; with --precond 3
the partitioned entry is rdc_solve_dist_mg, whose cycle adds the sized callbacks of the levels below the matrix); --ab smoother
(multigrid) in the order damped Jacobi, Gauss-Seidel, Gauss-Seidel, damped Jacobi.  --smoother 1 is the multicolour Gauss-Seidel
smoother of the cycle (option "mg_smoother"; single partition, --precond 3), --gs-fuse 0 gives every level one launch per colour
(option "mg_gs_fuse"); every record of a multigrid solve has the smoother, with Gauss-Seidel the colours per level, and the
kernel launches of one cycle (counted from the level sizes and colours: tools/time_loop.py, cycle_launches).  --ilu-bits 32
(--precond 4 or 5, with or without --mixed and --ranks) sets the option "ilu_factor_bits": the sweeps of the ILU(0) stream an fp32
copy of the FP64 factor, and every record has ilu_factor_bits, what they streamed; --ab ilu_bits runs the loop in the order 64, 32,
32, 64 (with --mixed the legs at 64 run on the FP64 operator, since the FP64 factor has no mixed form: they are today's ILU(0),
the legs at 32 the fp32 operator with the fp32 factor).  --method gmres (one partition) sets the option "solve_method": restarted
GMRES(m) in place of BiCGStab, m = --restart (option "gmres_restart", default 30); iterations are then Arnoldi steps, restarts the
cycles after the first, and every record has the method, the restart length and the device bytes of the basis; --ab method runs
the loop in the order BiCGStab, GMRES, GMRES, BiCGStab with --precond (and --mixed).  With --ranks N (N = 1 included: the partitioned
entry at world size 1 in this process) or --ab dist, --method gmres is rdc_solve_dist_gmres, GMRES(m) across ranks through a
communicator with the wide all-reduce, whatever the preconditioner (2, 3, 5); --ab dist --method gmres times rdc_solve under
"solve_method" = 1 against it in the order rdc_solve, rdc_solve_dist_gmres, rdc_solve_dist_gmres, rdc_solve.  --dump writes the state after the last step as DIR/state.npy (+ conn, xyz).
--precond 6 is the cycle of --precond 3 with the rank-local multicolour Gauss-Seidel smoother (Gauss-Seidel inside each rank, Jacobi
between the ranks; "mg_smoother" is not consulted), the form --ranks takes; every record has the multigrid figures and this rank's
colours per level.  On one partition it runs what --precond 3 --smoother 1 runs; --precond 6 --ab dist times exactly that pair in the
order rdc_solve (precond 3, smoother 1), rdc_solve_dist_mg (precond 6), rdc_solve_dist_mg, rdc_solve.  --ab smoother with --ranks runs
the loop in the order precond 3, 6, 6, 3 in the same processes.

--ranks N: one process per rank (recursive coordinate bisection, one ghost layer, interior nodes first), every step assemble ->
rdc_solve_dist (--precond 3: rdc_solve_dist_mg, multigrid with rank-local aggregates) -> clamp on each rank's part; the solve leaves the owners' values in the ghost rows, so the next assembly needs
no halo update of its own.  --ab (= --ab precond) with --ranks runs the loop from the same initial state in the order block Jacobi,
multigrid, rank-local ILU(0), rank-local ILU(0), multigrid, block Jacobi in the same processes, --ab method in the order BiCGStab, GMRES,
GMRES, BiCGStab with --precond.  Prints per rank the owned / interior / ghost nodes and the bytes of one exchange, and per step the
iterations and the global true residual.  Rank r uses GPU r modulo the number of GPUs: on a one-GPU machine the ranks share it,
and with --backend gloo every message is staged through the host -- such a run checks correctness and measures nothing."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402


def state_tensor(ctx):
    """zero-copy torch view [n_node][nvar] of the context's FIELD_OLD_SOLUTION storage"""
    import torch

    class _View:
        pass
    v = _View()
    ptr = ctx.field_device_ptr(0, ctx.n_node * ctx.nvar)
    v.__cuda_array_interface__ = {"shape": (ctx.n_node, ctx.nvar), "typestr": "<f8", "data": (ptr, False), "version": 2, "strides": None}
    return torch.as_tensor(v, device=torch.device("cuda", ctx.device))


def background_share(u, conn_dev):
    """(share of nodes, share of elements all of whose nodes) with n = c = h = a = 0 exactly; u, conn_dev: torch, on the device"""
    bg = (u[:, 0] == 0) & (u[:, 1] == 0) & (u[:, 2] == 0) & (u[:, 4] == 0)
    return float(bg.double().mean()), float(bg[conn_dev].all(dim=1).double().mean())


def cycle_launches(levels, colours=None, fuse=True, fused_nodes=512):
    """kernel launches of one V(1,1) cycle on one partition.  Both smoothers: the first sweep of level 0, an operator application and
    a restriction per step down, a prolongation per step up.  Damped Jacobi: 2 more (operator, update) for each of the 7 further sweeps
    of the last level and for the post-smoothing of every other level.  Gauss-Seidel (colours = [colours per level]): a sweep is one
    launch per colour, or one launch for all sweeps on a level of at most fused_nodes (rdc_solve.h, MG_GS_FUSED_NODES) nodes"""
    last = len(levels) - 1
    sweeps = [1] * last + [7]

    def smooth(l):
        if colours is None:
            return 2 * sweeps[l]
        return 1 if fuse and levels[l][0] <= fused_nodes else colours[l] * sweeps[l]
    return 1 + 3 * last + sum(smooth(l) for l in range(last + 1))


def run(ctx, conn, params, steps, rel_tol=1e-8, precond=2, max_its=20000, on_step=None, mixed=False, comm=None, smoother=0, gs_fuse=1,
        ilu_bits=64, method="bicgstab", restart=30):
    """the loop on an uploaded context whose FIELD_OLD_SOLUTION is set; returns one dict per step.
    on_step(k, phase, ctx) is called with phase 'assembled' and 'solved' (tests look at the state there).
    comm: a halo.SolveComm -- the solve is solve_dist across its ranks (the background shares are then those of the local nodes)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    u = state_tensor(ctx)
    conn_dev = torch.from_numpy(np.ascontiguousarray(conn, dtype=np.int64)).to(dev)
    ctx.timing_enable(True)
    if precond == 3 and comm is None:   # across partitions the smoother is damped Jacobi, and the option would be refused
        ctx.set_option("mg_smoother", smoother)
        ctx.set_option("mg_gs_fuse", gs_fuse)
    if precond == 3 and comm is not None:
        ctx.set_option("mg_smoother", 0)
    if precond == 6:                    # the rank-local Gauss-Seidel smoother: "mg_smoother" is not consulted
        ctx.set_option("mg_gs_fuse", gs_fuse)
    if precond in (4, 5):
        ctx.set_option("ilu_factor_bits", ilu_bits)
    # across partitions the method is in the entry's name, and rdc_solve_dist would refuse "solve_method" = 1
    ctx.set_option("solve_method", 1 if method == "gmres" and comm is None else 0)
    ctx.set_option("gmres_restart", restart)
    out = []
    for k in range(steps):
        ctx.assemble_pihna(params)
        ctx.synchronize()
        asm_ms = ctx.timing_last_ms()
        if on_step:
            on_step(k, "assembled", ctx)
        if comm is None:
            info = ctx.solve(u.data_ptr(), rel_tol=rel_tol, precond=precond, max_its=max_its, mixed=mixed)
        else:
            dist_solve = ctx.solve_dist_gmres if method == "gmres" else ctx.solve_dist
            info = dist_solve(comm, u.data_ptr(), rel_tol=rel_tol, precond=precond, max_its=max_its, mixed=mixed)
        if on_step:
            on_step(k, "solved", ctx)
        ctx.clamp_nonnegative(0)
        ctx.synchronize()
        nodes, elems = background_share(u, conn_dev)
        out.append(dict(step=k + 1, assembly_ms=asm_ms, solve_ms=info.device_ms, iterations=info.iterations, restarts=info.restarts,
                        reason=info.reason, matrix_bits=info.matrix_bits, residual_norm=info.residual_norm, rhs_norm=info.rhs_norm,
                        background_nodes=nodes, background_elems=elems))
        if method == "gmres":
            out[-1].update(method="gmres", gmres_restart=restart, gmres_basis_bytes=ctx.gmres_stats()[1] if info.iterations else 0)
        if precond in (3, 6):
            setup_ms, level_bytes = ctx.mg_stats()
            out[-1].update(mg_setup_ms=setup_ms, mg_level_bytes=level_bytes, mg_levels=ctx.mg_levels())
            if comm is None and precond == 3:
                colours = ctx.mg_colours() if smoother else None
                out[-1].update(mg_smoother=smoother, cycle_launches=cycle_launches(out[-1]["mg_levels"], colours, bool(gs_fuse)))
                if smoother:
                    out[-1].update(mg_colours=colours, mg_gs_fuse=gs_fuse)
            if precond == 6:
                out[-1].update(mg_colours=ctx.mg_colours(), mg_gs_fuse=gs_fuse)
        if precond in (4, 5):
            setup_ms, nbytes, colours = ctx.ilu_stats()
            out[-1].update(ilu_setup_ms=setup_ms, ilu_bytes=nbytes, ilu_colours=colours, ilu_factor_bits=ctx.ilu_factor_bits())
    return out


def rank_main(rank, world, port, a):
    """one rank of --ranks"""
    import os
    from datetime import timedelta
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    gpu = rank % torch.cuda.device_count()
    torch.cuda.set_device(gpu)
    dist.init_process_group(a.backend, rank=rank, world_size=world, timeout=timedelta(seconds=300))
    try:
        from rdcfes_amd import AssemblyContext, SolveComm, partition, pihna_params_from_dict, synth
        conn, xyz = synth.kuhn_tet_mesh(a.n, order="lex")
        p = pihna_params_from_dict(synth.pihna_param_dict("shipped"))
        part = partition.partition_rcb(xyz[conn.astype(np.int64)].mean(axis=1), world)
        lp = partition.build_local(conn, xyz, part, rank, world)
        with AssemblyContext(gpu) as ctx:
            ctx.set_option("interior_nodes", int(lp.n_interior))
            ctx.mesh_upload(4, lp.conn, lp.xyz, 5, n_owned=lp.n_owned)
            ctx.field_upload(0, synth.pihna_fields(xyz)[lp.node_global])
            preconds = (2, 3, 5, 5, 3, 2) if a.ab == "precond" else (3, 6, 6, 3) if a.ab == "smoother" else (a.precond,)
            methods = ("bicgstab", "gmres", "gmres", "bicgstab") if a.ab == "method" else (a.method,) * len(preconds)
            preconds = preconds * (len(methods) // len(preconds))
            # multigrid: rdc_solve_dist_mg; GMRES: rdc_solve_dist_gmres
            comm = SolveComm(lp, 5, torch.device("cuda", gpu), sized=3 in preconds or 6 in preconds, wide="gmres" in methods)
            shared = world > torch.cuda.device_count()
            head = dict(rank=rank, gpu=gpu, owned_nodes=int(lp.n_owned), interior_nodes=int(lp.n_interior),
                        ghost_nodes=int(lp.xyz.shape[0] - lp.n_owned), halo_bytes_per_exchange=comm.bytes_per_exchange,
                        neighbours=len(comm.send_peers), backend=a.backend,
                        timing="correctness only: ranks share a GPU or stage through the host" if shared or a.backend == "gloo" else "device")
            for r in range(world):     # one line per rank, in rank order
                if r == rank:
                    print(json.dumps(head), flush=True)
                dist.barrier()
            for precond, method in zip(preconds, methods):
                if len(preconds) > 1:
                    ctx.field_upload(0, synth.pihna_fields(xyz)[lp.node_global])
                    if rank == 0:
                        print(json.dumps(dict(precond=precond, method=method)), flush=True)
                for rec in run(ctx, lp.conn, p, a.steps, a.rel_tol, precond, a.max_its, mixed=a.mixed, comm=comm, ilu_bits=a.ilu_bits,
                               method=method, restart=a.restart):
                    if rank == 0:          # every figure of the solve is global and the same on every rank
                        keep = ("step", "iterations", "restarts", "reason", "matrix_bits", "residual_norm", "rhs_norm", "solve_ms", "assembly_ms")
                        keep += ("mg_setup_ms", "mg_level_bytes", "mg_levels") if precond in (3, 6) else ()     # rank 0's own levels
                        keep += ("mg_colours", "mg_gs_fuse") if precond == 6 else ()                           # rank 0's own colours
                        keep += ("ilu_setup_ms", "ilu_bytes", "ilu_colours", "ilu_factor_bits") if precond == 5 else ()        # rank 0's own factor
                        keep += ("method", "gmres_restart", "gmres_basis_bytes") if method == "gmres" else ()                  # rank 0's own basis
                        print(json.dumps({k: rec[k] for k in keep}), flush=True)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=119)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rel-tol", type=float, default=1e-8)
    ap.add_argument("--precond", type=int, default=2)
    ap.add_argument("--max-its", type=int, default=20000)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--smoother", type=int, choices=(0, 1), default=0)
    ap.add_argument("--gs-fuse", type=int, choices=(0, 1), default=1)
    ap.add_argument("--ab", nargs="?", const="precond", choices=("precond", "precision", "dist", "smoother", "ilu_bits", "method"), default=None)
    ap.add_argument("--method", choices=("bicgstab", "gmres"), default="bicgstab")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--ilu-bits", type=int, choices=(32, 64), default=64)
    ap.add_argument("--dump", default=None)
    ap.add_argument("--ranks", type=int, default=None)
    ap.add_argument("--backend", choices=("gloo", "nccl"), default="gloo")
    a = ap.parse_args()
    world1 = a.ranks == 1        # asked for: the partitioned entry at world size 1, in this process
    a.ranks = a.ranks or 1
    if a.ab == "smoother":
        a.precond = 3
    if (a.smoother or (a.ab == "smoother" and a.ranks == 1)) and (a.precond != 3 or a.ranks > 1 or world1 or a.ab == "dist"):
        ap.error("the Gauss-Seidel smoother belongs to --precond 3 on one partition (across ranks: --precond 6, or --ab smoother with --ranks)")
    if a.precond == 6 and a.ab not in (None, "dist", "method"):
        ap.error("--precond 6 takes --ab dist and --ab method only")
    f32 = a.ilu_bits == 32 or a.ab == "ilu_bits"
    if (f32 or a.ab == "ilu_bits") and a.precond not in (4, 5):
        ap.error("--ilu-bits and --ab ilu_bits belong to the block ILU(0): --precond 4 or 5")
    if a.precond == 4 and ((a.mixed and not f32) or a.ranks > 1 or world1 or a.ab in ("precision", "dist")):
        ap.error("the block ILU(0) (--precond 4) is FP64 on one partition: rdc_solve only (across ranks: --precond 5; --mixed: --ilu-bits 32)")
    if a.precond == 5 and not f32 and (a.mixed or a.ab == "precision"):
        ap.error("the rank-local block ILU(0) (--precond 5) is FP64 only, unless --ilu-bits 32")
    if a.ab == "method" and world1:
        ap.error("--ab method at world size 1 in one process: leave --ranks out")
    if world1 and a.ab not in (None, "dist"):
        ap.error("--ranks 1 is the partitioned entry at world size 1 and takes no --ab but dist, which is the same comparison")
    if not 1 <= a.restart <= 128:
        ap.error("--restart is 1 .. 128")
    if a.ranks > 1 and a.ab not in (None, "precond", "method", "smoother"):
        ap.error("--ranks takes --ab precond, --ab method and --ab smoother only")
    if a.ranks > 1 and a.ab == "precond" and a.mixed:
        ap.error("--ab precond with --ranks is FP64: the rank-local ILU(0) has no mixed form")
    if a.ranks > 1:
        import socket
        import torch.multiprocessing as mp
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        print(json.dumps(dict(mesh=f"K({a.n})", ranks=a.ranks, backend=a.backend, rel_tol=a.rel_tol, precond=a.precond, mixed=a.mixed,
                              method=a.method if a.ab != "method" else "bicgstab, gmres, gmres, bicgstab",
                              restart=a.restart if a.method == "gmres" or a.ab == "method" else None)), flush=True)
        mp.spawn(rank_main, args=(a.ranks, port, a), nprocs=a.ranks, join=True)
        return
    import torch
    torch.cuda.init()                       # before the library opens the device: one runtime initialisation order for both
    from rdcfes_amd import AssemblyContext, pihna_params_from_dict, synth
    conn, xyz = synth.kuhn_tet_mesh(a.n, order="lex")
    p = pihna_params_from_dict(synth.pihna_param_dict("shipped"))
    with AssemblyContext(0) as ctx:
        ctx.mesh_upload(4, conn, xyz, 5)
        u0 = synth.pihna_fields(xyz)
        runs = [(a.precond, a.mixed, world1, a.smoother, a.ilu_bits)]
        methods = ("bicgstab", "gmres", "gmres", "bicgstab") if a.ab == "method" else None
        if methods:
            runs = runs * len(methods)
        if a.ab == "precond":
            runs = [(pc, a.mixed, False, a.smoother, a.ilu_bits) for pc in ((2, 3, 3, 2) if a.mixed and not f32 else (2, 3, 4, 4, 3, 2))]
        elif a.ab == "precision":
            runs = [(a.precond, mixed, False, a.smoother, a.ilu_bits) for mixed in (False, True, True, False)]
        elif a.ab == "dist":
            runs = [(a.precond, a.mixed, d, 0, a.ilu_bits) for d in (False, True, True, False)]
            if a.precond == 6:     # the single-partition leg is what the partitioned one must equal: precond 3 under "mg_smoother" = 1
                runs = [(6 if d else 3, a.mixed, d, 0 if d else 1, a.ilu_bits) for d in (False, True, True, False)]
        elif a.ab == "smoother":
            runs = [(3, a.mixed, False, sm, 64) for sm in (0, 1, 1, 0)]
        elif a.ab == "ilu_bits":
            runs = [(a.precond, a.mixed and bits == 32, False, 0, bits) for bits in (64, 32, 32, 64)]
        comm = None
        if a.ab == "dist" or world1:      # world size 1: no peers, no process group
            from rdcfes_amd import SolveComm, partition
            lp = partition.LocalPartition(rank=0, nparts=1, conn=conn, xyz=xyz, n_owned=xyz.shape[0], node_global=np.arange(xyz.shape[0]),
                                          elem_global=np.arange(conn.shape[0]), n_elem_owned=conn.shape[0])
            comm = SolveComm(lp, 5, torch.device("cuda", 0), sized=a.precond in (3, 6), wide=a.method == "gmres")
        for leg, (precond, mixed, dist_entry, smoother, ilu_bits) in enumerate(runs):
            method = methods[leg] if methods else a.method
            ctx.field_upload(0, u0)
            print(json.dumps(dict(mesh=f"K({a.n})", tets=int(conn.shape[0]), unknowns=int(xyz.shape[0] * 5), rel_tol=a.rel_tol, precond=precond, mixed=mixed,
                                  smoother=smoother if precond == 3 else 1 if precond == 6 else None, ilu_bits=ilu_bits if precond in (4, 5) else None,
                                  method=method, restart=a.restart if method == "gmres" else None,
                                  entry=("rdc_solve_dist_gmres" if method == "gmres" else "rdc_solve_dist_mg" if precond in (3, 6) else "rdc_solve_dist") +
                                  ", world size 1" if dist_entry else "rdc_solve")))
            for rec in run(ctx, conn, p, a.steps, a.rel_tol, precond, a.max_its, mixed=mixed, comm=comm if dist_entry else None,
                           smoother=smoother, gs_fuse=a.gs_fuse, ilu_bits=ilu_bits, method=method, restart=a.restart):
                print(json.dumps(rec), flush=True)
        if a.dump:
            d = Path(a.dump)
            d.mkdir(parents=True, exist_ok=True)
            np.save(d / "state.npy", ctx.field_download(0, xyz.shape[0] * 5).reshape(-1, 5))
            np.save(d / "conn.npy", conn)
            np.save(d / "xyz.npy", xyz)


if __name__ == "__main__":
    main()
