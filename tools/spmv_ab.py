"""rdc_csr_matvec (block-pattern SpMV on the context's own values), rdc_csr_matvec_f32 (the same pattern over the fp32
copy of D^-1 A that rdc_solve_mixed iterates on) and rocsparse_dcsrmv on the same assembled PIHNA matrix of a Kuhn mesh
K(n), alternating, median of --reps launches each after warm-up.  The two fp64 results are compared with each other; of
the fp32-value result the tool checks only that two launches agree bitwise (its accuracy is held by
tests/test_gpu_solve_mixed.py).

    python tools/spmv_ab.py --n 119 [--reps 25]

rocSPARSE is loaded with ctypes by this tool only (the product does not link it); its scalar row_ptr / col_idx are
built on the host and uploaded (4 B per non-zero more on the device: when that does not fit, the tool steps down to the
largest K(n) that does -- first to what free memory suggests, then one by one -- and says which).  Also times one BiCGStab
iteration: the device time of a solve with max_its = 2 ITS minus that of one with ITS, over ITS.
The same difference is taken for a mixed solve, and the set-up cost of the fp32 copy is the difference of the two kinds'
"set-up and closing residual" figures.
Algorithmic bytes of the block-pattern kernel: 8 nnz + 4 blocks + 8 (rows_in + rows_out) + 8 n_owned (bptr); of the
fp32-value kernel: 4 nnz + 4 blocks + 8 (rows_in + rows_out) + 16 n_owned (bptr and the offsets of the padded rows)."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12


def _rocsparse():
    for name in ("librocsparse.so", "librocsparse.so.1", "/opt/rocm/lib/librocsparse.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise RuntimeError("librocsparse.so not found")


def _events(torch, fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def measure(n, reps, its):
    import torch
    from rdcfes_amd import AssemblyContext, pihna_params_from_dict, synth
    dev = torch.device("cuda", 0)
    conn, xyz = synth.kuhn_tet_mesh(n, order="lex")
    p = pihna_params_from_dict(synth.pihna_param_dict("shipped"))
    with AssemblyContext(0) as ctx:
        ctx.mesh_upload(4, conn, xyz, 5)
        ctx.field_upload(0, synth.pihna_fields(xyz))
        ctx.assemble_pihna(p)
        ctx.synchronize()
        n_rows, nnz = ctx.csr_dims()
        rp, col = ctx.csr_pattern()
        if nnz >= 2 ** 31:
            raise MemoryError("more than 2^31 non-zeros: rocsparse_int is 32 bits")
        rp_d = torch.from_numpy(rp.astype(np.int32)).to(dev)
        col_d = torch.from_numpy(col).to(dev)
        del rp, col
        x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, n_rows)).to(dev)
        y_a = torch.zeros(n_rows, dtype=torch.float64, device=dev)
        y_b = torch.zeros(n_rows, dtype=torch.float64, device=dev)
        y_c = torch.zeros(n_rows, dtype=torch.float64, device=dev)
        vptr, _ = ctx.csr_values_device_ptr()
        rs = _rocsparse()
        handle, descr = C.c_void_p(), C.c_void_p()
        assert rs.rocsparse_create_handle(C.byref(handle)) == 0
        assert rs.rocsparse_create_mat_descr(C.byref(descr)) == 0
        assert rs.rocsparse_set_stream(handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        one, zero = C.c_double(1.0), C.c_double(0.0)
        rs.rocsparse_dcsrmv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p]

        def roc():
            st = rs.rocsparse_dcsrmv(handle, 111, n_rows, n_rows, nnz, C.byref(one), descr, C.c_void_p(vptr), C.c_void_p(rp_d.data_ptr()),
                                     C.c_void_p(col_d.data_ptr()), None, C.c_void_p(x.data_ptr()), C.byref(zero), C.c_void_p(y_b.data_ptr()))
            assert st == 0, st

        ctx.set_stream(torch.cuda.current_stream().cuda_stream)

        def ours():
            ctx.csr_matvec_device(x.data_ptr(), y_a.data_ptr())

        ctx.csr_scale_f32(2)

        def ours32():
            ctx.csr_matvec_f32_device(x.data_ptr(), y_c.data_ptr())

        for _ in range(3):
            ours()
            ours32()
            roc()
        torch.cuda.synchronize()
        t_a, t_b, t_c = [], [], []
        for _ in range(reps):                      # alternate the three
            t_a += _events(torch, ours, 1)
            t_c += _events(torch, ours32, 1)
            t_b += _events(torch, roc, 1)
        scale = torch.abs(y_b).max().item()
        diff = torch.abs(y_a - y_b).max().item()
        blocks = nnz // 25
        bytes_block = 8 * nnz + 4 * blocks + 8 * (2 * n_rows) + 8 * (n_rows // 5)
        bytes_csr = 12 * nnz + 8 * (2 * n_rows) + 4 * n_rows
        bytes_f32 = 4 * nnz + 4 * blocks + 8 * (2 * n_rows) + 16 * (n_rows // 5)
        ms_a, ms_b, ms_c = float(np.median(t_a)), float(np.median(t_b)), float(np.median(t_c))
        xs = torch.zeros(n_rows, dtype=torch.float64, device=dev)
        ctx.solve(xs.data_ptr(), rel_tol=0.0, max_its=3)          # warm-up, allocates the work vectors
        # set-up (preconditioner, first residual) and the closing residual are the same in both runs: the difference is 'its' iterations
        xs.zero_()
        info1 = ctx.solve(xs.data_ptr(), rel_tol=0.0, max_its=its)
        xs.zero_()
        info = ctx.solve(xs.data_ptr(), rel_tol=0.0, max_its=2 * its)
        ms_it = (info.device_ms - info1.device_ms) / max(info.iterations - info1.iterations, 1)
        ctx.solve(xs.data_ptr(), rel_tol=0.0, max_its=3, mixed=True)
        xs.zero_()
        m1 = ctx.solve(xs.data_ptr(), rel_tol=0.0, max_its=its, mixed=True)
        xs.zero_()
        m2 = ctx.solve(xs.data_ptr(), rel_tol=0.0, max_its=2 * its, mixed=True)
        assert m1.matrix_bits == 32 and m2.matrix_bits == 32
        ms_it32 = (m2.device_ms - m1.device_ms) / max(m2.iterations - m1.iterations, 1)
        setup64 = info1.device_ms - info1.iterations * ms_it
        setup32 = m1.device_ms - m1.iterations * ms_it32
        # fixed summation order: a second launch on the same x (and the same copy, rebuilt by the solves above) agrees bitwise
        y_c2 = torch.zeros_like(y_c)
        ctx.csr_matvec_f32_device(x.data_ptr(), y_c2.data_ptr())
        torch.cuda.synchronize()
        f32_repeatable = bool(torch.equal(y_c, y_c2))
        ctx.set_stream(0)
        rs.rocsparse_destroy_mat_descr(descr)
        rs.rocsparse_destroy_handle(handle)
        return dict(mesh=f"K({n})", rows=n_rows, nnz=nnz, reps=reps,
                    block_spmv_ms=ms_a, block_spmv_min_ms=float(min(t_a)), block_bytes=bytes_block,
                    block_TBps=bytes_block / ms_a * 1e-9, block_fraction_of_8TBps=bytes_block / (ms_a * 1e-3) / HBM_PEAK,
                    rocsparse_ms=ms_b, rocsparse_min_ms=float(min(t_b)), rocsparse_bytes=bytes_csr, rocsparse_TBps=bytes_csr / ms_b * 1e-9,
                    f32_spmv_ms=ms_c, f32_spmv_min_ms=float(min(t_c)), f32_bytes=bytes_f32, f32_TBps=bytes_f32 / ms_c * 1e-9,
                    f32_fraction_of_8TBps=bytes_f32 / (ms_c * 1e-3) / HBM_PEAK, f32_over_block_spmv=ms_c / ms_a,
                    f32_bitwise_repeatable=f32_repeatable,
                    max_abs_difference=diff, max_abs_y=scale,
                    bicgstab_iterations_timed=info.iterations - info1.iterations, bicgstab_ms_per_iteration=ms_it,
                    bicgstab_ms_setup_and_closing_residual=info1.device_ms - info1.iterations * ms_it,
                    iteration_over_two_spmv=ms_it / (2.0 * ms_a),
                    mixed_ms_per_iteration=ms_it32, mixed_ms_setup_and_closing_residual=setup32,
                    f32_copy_setup_ms=setup32 - setup64, mixed_iteration_over_two_f32_spmv=ms_it32 / (2.0 * ms_c))


def device_bytes(n):
    """what this tool holds on the device for K(n): values, rocSPARSE's indices, work lists of the assembly (about as much
    again as the indices), solver work vectors, the test vectors"""
    nodes = (n + 1) ** 3
    nnz = 25 * 15 * nodes
    return 12 * nnz + 4 * nnz + 4 * nnz + 8 * 5 * nodes * (6 + 5 + 4) + 4 * nnz // 25   # + the fp32 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=119)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--its", type=int, default=20)
    a = ap.parse_args()
    import torch
    n = a.n
    while True:
        try:
            rec = measure(n, max(a.reps, 20), a.its)
            break
        except (MemoryError, torch.cuda.OutOfMemoryError, RuntimeError) as e:
            if n <= 8 or not ("memory" in str(e).lower() or isinstance(e, MemoryError)):
                raise
            torch.cuda.empty_cache()
            free, _ = torch.cuda.mem_get_info()
            nxt = n - 1
            while nxt > 8 and device_bytes(nxt) > free:
                nxt -= 1
            print(f"K({n}) does not fit next to rocSPARSE's index arrays ({e}); trying K({nxt})", flush=True)
            n = nxt
    rec["requested_mesh"] = f"K({a.n})"
    assert rec["max_abs_difference"] <= 1e-9 * rec["max_abs_y"], rec
    assert rec["f32_bitwise_repeatable"], rec
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
