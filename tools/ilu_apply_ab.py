"""One apply of the multicolour block ILU(0) (forward + backward sweep, RDC_PRECOND_ILU0) against one rdc_csr_matvec on the same
assembled PIHNA matrix of a Kuhn mesh K(n), alternating, median of --reps after warm-up, as tools/spmv_ab.py times its kernels.

    python tools/ilu_apply_ab.py --n 119 [--reps 25] [--its 10] [--bits 32]

The apply has no entry of its own that runs it alone (rdc_solve_ilu_apply factors first), so it is timed as a difference: the
device time of a solve with max_its = 2 ITS minus that of one with ITS, over ITS, is one iteration (set-up, factorisation and the
closing residual are the same in both and cancel); an ILU(0) iteration differs from a block-Jacobi iteration by its two applies.
Each repetition runs block-Jacobi ITS / 2 ITS, ILU(0) ITS / 2 ITS and one matvec, in that order.
Algorithmic bytes of one apply: 8 nnz (the factor once: lower blocks forward, upper blocks backward, U_ii^-1 in place of the
diagonal blocks) + 4 blocks (column list) + 8 * 4 rows (y read, z written, read and written) + 2 * 20 nodes (bptr, lower count, node list
per sweep); the gathers of z are not counted, as the gathers of x are not counted for the SpMV.
--bits 32 times the apply on the fp32 copy of the factor (option "ilu_factor_bits" = 32) BESIDE the FP64 one: every repetition then
also runs ILU(0) ITS / 2 ITS with the option at 32, alternating with 64.  Its byte model: the floats of the copy (4 bytes per
off-diagonal non-zero and the padding of the rows, measured: what rdc_solve_ilu_stats grows by, less the 8 bytes of offset per node)
+ 8 nvar^2 nodes (U_ii^-1, FP64) + 4 blocks + 8 * 4 rows + 2 * 28 nodes (the offset of the node's floats comes on top per sweep)."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=119)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--its", type=int, default=10)
    ap.add_argument("--bits", type=int, choices=(32, 64), default=64)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from rdcfes_amd import AssemblyContext, pihna_params_from_dict, synth
    dev = torch.device("cuda", 0)
    conn, xyz = synth.kuhn_tet_mesh(a.n, order="lex")
    p = pihna_params_from_dict(synth.pihna_param_dict("shipped"))
    with AssemblyContext(0) as ctx:
        ctx.mesh_upload(4, conn, xyz, 5)
        ctx.field_upload(0, synth.pihna_fields(xyz))
        ctx.assemble_pihna(p)
        ctx.synchronize()
        n_rows, nnz = ctx.csr_dims()
        blocks, nodes = nnz // 25, n_rows // 5
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n_rows)).to(dev)
        y = torch.zeros(n_rows, dtype=torch.float64, device=dev)
        xs = torch.zeros(n_rows, dtype=torch.float64, device=dev)

        def iteration_ms(precond, bits=64):
            ctx.set_option("ilu_factor_bits", bits)
            xs.zero_()
            one = ctx.solve(xs.data_ptr(), rel_tol=0.0, max_its=a.its, precond=precond)
            xs.zero_()
            two = ctx.solve(xs.data_ptr(), rel_tol=0.0, max_its=2 * a.its, precond=precond)
            assert two.iterations == 2 * one.iterations == 2 * a.its, (one.iterations, two.iterations)
            return (two.device_ms - one.device_ms) / a.its, one.device_ms

        def matvec_ms():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.csr_matvec_device(x.data_ptr(), y.data_ptr())
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(2):
            iteration_ms(2), iteration_ms(4), matvec_ms()
        bytes64 = ctx.ilu_stats()[1]
        if a.bits == 32:
            iteration_ms(4, 32), iteration_ms(4, 32)
            assert ctx.ilu_factor_bits() == 32, "the factor does not fit fp32: the sweeps fell back to FP64"
        bj, ilu, mv, first, ilu32, first32 = [], [], [], [], [], []
        for _ in range(max(a.reps, 1)):
            bj.append(iteration_ms(2)[0])
            it, one = iteration_ms(4)
            ilu.append(it)
            first.append(one)
            if a.bits == 32:
                it, one = iteration_ms(4, 32)
                ilu32.append(it)
                first32.append(one)
            mv.append(matvec_ms())
        setup_ms, nbytes, colours = ctx.ilu_stats()
        ctx.set_option("ilu_factor_bits", 64)
        ctx.set_stream(0)
        bj_ms, ilu_ms, mv_ms = float(np.median(bj)), float(np.median(ilu)), float(np.median(mv))
        apply_ms = (ilu_ms - bj_ms) / 2.0
        apply_bytes = 8 * nnz + 4 * blocks + 8 * 4 * n_rows + 2 * 20 * nodes
        spmv_bytes = 8 * nnz + 4 * blocks + 8 * (2 * n_rows) + 8 * nodes
        out = dict(mesh=f"K({a.n})", rows=n_rows, nnz=nnz, reps=a.reps, its=a.its, colours=colours,
                              spmv_ms=mv_ms, spmv_min_ms=float(min(mv)), spmv_bytes=spmv_bytes, spmv_TBps=spmv_bytes / mv_ms * 1e-9,
                              block_jacobi_ms_per_iteration=bj_ms, ilu_ms_per_iteration=ilu_ms,
                              ilu_apply_ms=apply_ms, ilu_apply_bytes=apply_bytes, ilu_apply_TBps=apply_bytes / apply_ms * 1e-9,
                              ilu_apply_over_spmv=apply_ms / mv_ms, launches_per_apply=2 * colours,
                              ilu_setup_ms=setup_ms, ilu_bytes=nbytes, ilu_iteration_over_block_jacobi_iteration=ilu_ms / bj_ms,
                              solve_ms_at_its=float(np.median(first)))
        if a.bits == 32:
            ilu32_ms = float(np.median(ilu32))
            apply32_ms = (ilu32_ms - bj_ms) / 2.0
            floats = (nbytes - bytes64 - 8 * (nodes + 1)) // 4     # the copy, padding included (and at most 2 x 256 bytes of alignment)
            apply32_bytes = 4 * floats + 8 * 25 * nodes + 4 * blocks + 8 * 4 * n_rows + 2 * 28 * nodes
            out.update(ilu_f32_ms_per_iteration=ilu32_ms, ilu_f32_apply_ms=apply32_ms, ilu_f32_apply_bytes=apply32_bytes,
                       ilu_f32_apply_TBps=apply32_bytes / apply32_ms * 1e-9, ilu_f32_apply_over_fp64_apply=apply32_ms / apply_ms,
                       ilu_f32_copy_bytes=nbytes - bytes64, ilu_bytes_fp64_only=bytes64, solve_f32_ms_at_its=float(np.median(first32)),
                       ilu_f32_iteration_over_block_jacobi_iteration=ilu32_ms / bj_ms)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
