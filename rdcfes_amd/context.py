"""Thin object wrapper over the C-ABI (include/rdc_assembly.h); one instance == one rdc_ctx."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .params import (HccParams, PihnaParams, RipfParams, SolidMaterial, SolidNewtonInfo, SolidNewtonParams, SolidParams, SolveCommSizedStruct,
                     SolveCommWideStruct, SolveInfo, SolveParams)

TET4, HEX8 = 4, 8
SCATTER_AUTO, SCATTER_COLOURED, SCATTER_ROWGATHER = 0, 1, 2
FIELD_OLD_SOLUTION, FIELD_AUX_NODAL, FIELD_UNDEFORMED_XYZ, FIELD_ELEM_FIBRE = 0, 1, 2, 3
FIELD_PREV_SOLUTION, FIELD_TIME_DERIV, FIELD_RT_DOSE = 4, 5, 6
FIELD_ELEM_TRACTS = FIELD_ELEM_FIBRE  # ADPM: same per-element slot
VARIANT_AUTO, VARIANT_GENERIC = 0, 1
PRECOND_NONE, PRECOND_JACOBI, PRECOND_BLOCK_JACOBI, PRECOND_MULTIGRID, PRECOND_ILU0, PRECOND_ILU0_LOCAL = 0, 1, 2, 3, 4, 5
PRECOND_MULTIGRID_GS_LOCAL = 6   # the cycle of PRECOND_MULTIGRID with the rank-local multicolour Gauss-Seidel smoother
SOLVE_CONVERGED, SOLVE_MAX_ITS, SOLVE_BREAKDOWN, SOLVE_BAD_DIAGONAL, SOLVE_NOT_FINITE = 0, 1, 2, 3, 4
NEWTON_CONVERGED_RESIDUAL, NEWTON_CONVERGED_STEP, NEWTON_MAX_ITS, NEWTON_LINEAR_FAILED, NEWTON_NOT_FINITE = 0, 1, 2, 3, 4
ERR_INVALID, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED, ERR_ALLOC, ERR_COMM = 1, 2, 3, 4, 5, 6


class RdcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"rdc error {code}: {msg}")
        self.code = code


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class AssemblyContext:
    """Owns one rdc_ctx (one GPU, one mesh partition, one system)."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.rdc_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise RdcError(rc, self._lib.rdc_last_error(None).decode())
        self._h = h
        self.device = int(device)
        self.n_elem = self.n_node = self.n_owned = 0
        self.nvar = 0
        self._dist_plan = None   # the SolveComm whose send list the uploaded mesh holds (solve_dist)

    # -- plumbing
    def _ck(self, rc):
        if rc != 0:
            raise RdcError(rc, self._lib.rdc_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rdc_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, hip_stream_ptr):
        self._ck(self._lib.rdc_set_stream(self._h, C.c_void_p(int(hip_stream_ptr) if hip_stream_ptr else None)))

    def synchronize(self):
        self._ck(self._lib.rdc_synchronize(self._h))

    def set_scatter(self, strategy):
        self._ck(self._lib.rdc_set_scatter(self._h, int(strategy)))

    def set_kernel_variant(self, variant):
        self._ck(self._lib.rdc_set_kernel_variant(self._h, int(variant)))

    def set_option(self, key, value):
        self._ck(self._lib.rdc_set_option(self._h, key.encode(), int(value)))
        if key == "gmres_restart":
            self._gmres_restart = int(value)   # the shape of the Hessenberg matrix gmres_arnoldi returns

    def set_tet4_cluster(self, mode):
        """rdc_tet4_cluster_mode: 0 = off (default), 1 = the TET4 cluster kernel where the mesh has no pair lists (Gmsh and
        Delaunay meshes), 2 = on every TET4 mesh whose cluster lists can be built"""
        self._ck(self._lib.rdc_tet4_cluster_mode(self._h, int(mode)))

    def tet4_cluster_info(self):
        """rdc_tet4_cluster_info: mode, active (the last assembly call launched the cluster kernel), the lists' clusters,
        pairs and element visits, the dynamic LDS of that launch; last_error = rdc_last_error (after a refused list build:
        the builder's reason)"""
        mode, active = C.c_int32(), C.c_int32()
        n = [C.c_int64() for _ in range(4)]
        self._ck(self._lib.rdc_tet4_cluster_info(self._h, C.byref(mode), C.byref(active), *(C.byref(x) for x in n)))
        return {"mode": mode.value, "active": active.value, "n_clusters": n[0].value, "n_pairs": n[1].value,
                "n_elem_visits": n[2].value, "lds_bytes": n[3].value, "last_error": self._lib.rdc_last_error(self._h).decode()}

    def get_scatter(self):
        s = C.c_int()
        self._ck(self._lib.rdc_get_scatter(self._h, C.byref(s)))
        return s.value

    # -- mesh
    def mesh_upload(self, elem_type, conn, xyz, nvar, n_owned=None):
        conn = np.ascontiguousarray(conn, dtype=np.uint32)
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        if conn.ndim != 2 or conn.shape[1] != elem_type:
            raise ValueError("conn must be [n_elem][elem_type]")
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("xyz must be [n_node][3]")
        n_owned = xyz.shape[0] if n_owned is None else int(n_owned)
        self._ck(self._lib.rdc_mesh_upload(self._h, int(elem_type), conn.shape[0], xyz.shape[0], n_owned,
                                           conn.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(xyz), int(nvar)))
        self.elem_type, self.n_elem, self.n_node, self.n_owned, self.nvar = elem_type, conn.shape[0], xyz.shape[0], n_owned, nvar
        self._dist_plan = None

    def mesh_update_coords(self, xyz):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        if xyz.shape != (self.n_node, 3):
            raise ValueError("xyz shape mismatch")
        self._ck(self._lib.rdc_mesh_update_coords(self._h, _dp(xyz)))

    def coords_device_ptr(self):
        """device address of the CURRENT node coordinates [n_node][3] (rdc_mesh_coords_device_ptr)"""
        p = C.c_void_p()
        self._ck(self._lib.rdc_mesh_coords_device_ptr(self._h, C.byref(p)))
        return p.value

    def coords_tensor(self):
        """zero-copy torch view [n_node][3] of the context's current coordinates: the moving-mesh models update them in
        place on the device (mesh = solution of the solid system) and the halo exchange writes their ghost rows"""
        import torch

        class _View:
            pass
        v = _View()
        v.__cuda_array_interface__ = {"shape": (self.n_node, 3), "typestr": "<f8", "data": (self.coords_device_ptr(), False),
                                      "version": 2, "strides": None}
        return torch.as_tensor(v, device=torch.device("cuda", self.device))

    def n_colours(self):
        nc = C.c_int()
        self._ck(self._lib.rdc_mesh_dims(self._h, None, None, None, None, None, C.byref(nc)))
        return nc.value

    def colours(self):
        out = np.empty(self.n_elem, dtype=np.int32)
        self._ck(self._lib.rdc_mesh_colours_download(self._h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def csr_dims(self):
        r, z = C.c_int64(), C.c_int64()
        self._ck(self._lib.rdc_csr_dims(self._h, C.byref(r), C.byref(z)))
        return r.value, z.value

    def csr_pattern(self):
        n_rows, nnz = self.csr_dims()
        row_ptr = np.empty(n_rows + 1, dtype=np.int64)
        col = np.empty(nnz, dtype=np.int32)
        self._ck(self._lib.rdc_csr_pattern_download(self._h, row_ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    col.ctypes.data_as(C.POINTER(C.c_int32))))
        return row_ptr, col

    # -- fields
    def field_upload(self, field, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        self._ck(self._lib.rdc_field_upload(self._h, int(field), _dp(arr), arr.size))

    def field_download(self, field, count):
        out = np.empty(int(count), dtype=np.float64)
        self._ck(self._lib.rdc_field_download(self._h, int(field), _dp(out), out.size))
        return out

    def field_device_ptr(self, field, count):
        p = C.c_void_p()
        self._ck(self._lib.rdc_field_device_ptr(self._h, int(field), int(count), C.byref(p)))
        return p.value

    def field_bind_device(self, field, dptr, count):
        self._ck(self._lib.rdc_field_bind_device(self._h, int(field), C.c_void_p(int(dptr)), int(count)))

    def clamp_nonnegative(self, field):
        self._ck(self._lib.rdc_clamp_nonnegative(self._h, int(field)))

    def pihna_volume_integrals(self, ranges, n_elem=-1):
        """the four volume sums of PIHNA's CSV line (src/pihna.C:842-976) over the first n_elem elements"""
        out = np.zeros(4)
        self._ck(self._lib.rdc_pihna_volume_integrals(self._h, C.byref(ranges), int(n_elem), _dp(out)))
        return out

    def ripf_volume_integrals(self, ranges, n_elem=-1):
        """Tumour_Volume, Fibrosis_Volume of RIPF's CSV line (src/ripf.C:777-866) over the first n_elem elements"""
        out = np.zeros(2)
        self._ck(self._lib.rdc_ripf_volume_integrals(self._h, C.byref(ranges), int(n_elem), _dp(out)))
        return out

    def adpm_parcellation_integrals(self, ranges, elem_subdomain, ids, n_elem=-1):
        """ADPM's CSV line (src/adpm.C:690-829): -> ([n_ids][4] = A_b concentration, Tau concentration, A_b volume,
        Tau volume per parcellation id; last element of every region, -1 if it has none here)"""
        sub = np.ascontiguousarray(elem_subdomain, dtype=np.int32)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if sub.size < (self.n_elem if n_elem < 0 else n_elem):
            raise ValueError("elem_subdomain shorter than the element range")
        out, last = np.zeros((ids.size, 4)), np.full(ids.size, -1, dtype=np.int64)
        self._ck(self._lib.rdc_adpm_parcellation_integrals(
            self._h, C.byref(ranges), sub.ctypes.data_as(C.POINTER(C.c_int32)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
            int(ids.size), int(n_elem), _dp(out), last.ctypes.data_as(C.POINTER(C.c_int64))))
        return out, last

    def solid_post_process(self, params):
        """SolidSystem::post_process -> (pressure [ne], von_mises [ne], fibre_current [ne][3])"""
        pr, vm, fc = np.empty(self.n_elem), np.empty(self.n_elem), np.empty((self.n_elem, 3))
        self._ck(self._lib.rdc_solid_post_process(self._h, C.byref(params), _dp(pr), _dp(vm), _dp(fc)))
        return pr, vm, fc

    def ripf_check_solution(self, params):
        """RIPF check_solution on the device fields (src/ripf.C:675-775); returns the maximum total RT dose."""
        mx = C.c_double(0.0)
        self._ck(self._lib.rdc_ripf_check_solution(self._h, C.byref(params), C.byref(mx)))
        return mx.value

    # -- solid set-up
    def solid_set_materials(self, elem_material, materials):
        em = np.ascontiguousarray(elem_material, dtype=np.int32)
        if em.shape != (self.n_elem,):
            raise ValueError("elem_material must have one entry per element")
        arr = (SolidMaterial * len(materials))(*materials)
        self._ck(self._lib.rdc_solid_set_materials(self._h, em.ctypes.data_as(C.POINTER(C.c_int32)), len(materials), arr))

    def solid_set_sides(self, side_elem, side_id, side_disp):
        se = np.ascontiguousarray(side_elem, dtype=np.int64)
        si = np.ascontiguousarray(side_id, dtype=np.int32)
        sd = np.ascontiguousarray(side_disp, dtype=np.float64).reshape(-1, 3)
        if not (se.shape[0] == si.shape[0] == sd.shape[0]):
            raise ValueError("side arrays must have equal length")
        self._ck(self._lib.rdc_solid_set_sides(self._h, se.shape[0], se.ctypes.data_as(C.POINTER(C.c_int64)),
                                               si.ctypes.data_as(C.POINTER(C.c_int32)), _dp(sd)))

    # -- the hot path
    def assemble_pihna(self, p: PihnaParams):
        self._ck(self._lib.rdc_assemble_pihna(self._h, C.byref(p)))

    def assemble_ripf(self, p: RipfParams):
        self._ck(self._lib.rdc_assemble_ripf(self._h, C.byref(p)))

    def assemble_hcc(self, p: HccParams):
        self._ck(self._lib.rdc_assemble_hcc(self._h, C.byref(p)))

    def assemble_proteas(self, p):
        """assemble_proteas_model (src/proteas.C:338-705); FIELD_AUX_NODAL = {HU, RTD, 0} per node."""
        self._ck(self._lib.rdc_assemble_proteas(self._h, C.byref(p)))

    def assemble_adpm(self, p):
        """assemble_adpm (src/adpm.C:324-652); the tract vectors go into FIELD_ELEM_TRACTS first."""
        self._ck(self._lib.rdc_assemble_adpm(self._h, C.byref(p)))

    def assemble_pihna_part(self, p: PihnaParams, part, stream=0):
        """one part (1 | 2, 0 = whole) of a two-part step on the given hipStream_t, in one C-ABI call"""
        self._ck(self._lib.rdc_assemble_pihna_part(self._h, C.byref(p), int(part), C.c_void_p(int(stream) or None)))

    def assemble_hcc_part(self, p: HccParams, part, stream=0):
        self._ck(self._lib.rdc_assemble_hcc_part(self._h, C.byref(p), int(part), C.c_void_p(int(stream) or None)))

    def solid_assemble_part(self, p: SolidParams, request_jacobian, part, stream=0):
        self._ck(self._lib.rdc_solid_assemble_part(self._h, C.byref(p), 1 if request_jacobian else 0, int(part), C.c_void_p(int(stream) or None)))

    def solid_assemble(self, p: SolidParams, request_jacobian=True):
        self._ck(self._lib.rdc_solid_assemble(self._h, C.byref(p), 1 if request_jacobian else 0))

    # -- device-resident Newton solve of the solid system
    def solid_newton(self, params: SolidParams, *, max_nonlinear_iterations, require_reduction, relative_step_tolerance,
                     relative_residual_tolerance, absolute_residual_tolerance, rel_tol, max_its, precond=PRECOND_BLOCK_JACOBI,
                     mixed=False) -> SolidNewtonInfo:
        """rdc_solid_newton: SolidSystem::solve() in one call.  The unknowns are the context's current coordinates (start iterate
        in, result out: coords_tensor(), or solid_post_process on them); params carries pseudo_time, so the caller runs the load
        steps.  The keyword arguments are the "solver/nonlinear/*" options and, for the linear solve of every iteration, rel_tol =
        "solver/linear/initial_linear_tolerance", max_its, precond and mixed as in solve(); the options of solve() that are set with
        set_option ("solve_method", "mg_smoother", ...) hold.  No matrix, rhs or vector is handed back.  A solver outcome is not an
        error: info.reason is one of NEWTON_*; solid_newton_history() lists the iterations."""
        np_ = SolidNewtonParams(int(max_nonlinear_iterations), 1 if require_reduction else 0, float(relative_step_tolerance),
                                float(relative_residual_tolerance), float(absolute_residual_tolerance),
                                SolveParams(float(rel_tol), 0.0, -1.0, int(max_its), int(precond)), 1 if mixed else 0, 0)
        info = SolidNewtonInfo()
        self._ck(self._lib.rdc_solid_newton(self._h, C.byref(params), C.byref(np_), C.byref(info)))
        return info

    def solid_newton_dist(self, comm, params: SolidParams, *, max_nonlinear_iterations, require_reduction, relative_step_tolerance,
                          relative_residual_tolerance, absolute_residual_tolerance, rel_tol, max_its, precond=PRECOND_BLOCK_JACOBI,
                          mixed=False) -> SolidNewtonInfo:
        """rdc_solid_newton_dist: solid_newton across the ranks of comm (halo.SolveComm), every rank calling with its own ghosted
        context.  Arguments as solid_newton.  The norms the loop decides on are global, so the returned info and
        solid_newton_history() are the same on every rank (device_ms is this rank's own).  Ghost coordinates are ignored on entry
        and hold the owners' values on exit.  The linear solve of an iteration is rdc_solve_dist_gmres under
        set_option("solve_method", 1), rdc_solve_dist_mg for PRECOND_MULTIGRID and PRECOND_MULTIGRID_GS_LOCAL, rdc_solve_dist
        otherwise; comm needs the callbacks of that entry (SolveComm(..., sized=True) / wide=True) and the library refuses,
        RdcError invalid, before any callback if one is missing.  The send list of comm is uploaded once per mesh, as in
        solve_dist.  An exception raised inside a callback of comm is re-raised here."""
        self._dist_plan_for(comm)
        # the superset struct; what comm does not have stays NULL, and the library says which callback the dispatch misses
        wide = getattr(comm, "wide_struct", None)
        if wide is None:
            sized = getattr(comm, "sized_struct", None)
            wide = SolveCommWideStruct(sized if sized is not None else SolveCommSizedStruct(comm.struct))
        np_ = SolidNewtonParams(int(max_nonlinear_iterations), 1 if require_reduction else 0, float(relative_step_tolerance),
                                float(relative_residual_tolerance), float(absolute_residual_tolerance),
                                SolveParams(float(rel_tol), 0.0, -1.0, int(max_its), int(precond)), 1 if mixed else 0, 0)
        info = SolidNewtonInfo()
        comm.error = None
        rc = self._lib.rdc_solid_newton_dist(self._h, C.byref(params), C.byref(np_), C.byref(wide), C.byref(info))
        if comm.error is not None:
            err, comm.error = comm.error, None
            raise err
        self._ck(rc)
        return info

    def solid_newton_history(self):
        """rdc_solid_newton_history -> (residual, step, lin_its, lin_reason), one entry per Newton iteration of the last
        solid_newton or solid_newton_dist: ||R|| before the solve, the accepted step length, the linear iterations and the reason of that solve"""
        n = C.c_int32()
        self._ck(self._lib.rdc_solid_newton_history(self._h, 0, None, None, None, None, C.byref(n)))
        res, step = np.zeros(n.value), np.zeros(n.value)
        its, reason = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        self._ck(self._lib.rdc_solid_newton_history(self._h, n.value, _dp(res), _dp(step), its.ctypes.data_as(i32p),
                                                    reason.ctypes.data_as(i32p), C.byref(n)))
        return res, step, its, reason

    # -- results
    def csr_values_device_ptr(self):
        v, r = C.c_void_p(), C.c_void_p()
        self._ck(self._lib.rdc_csr_values_device_ptr(self._h, C.byref(v), C.byref(r)))
        return v.value, r.value

    def csr_download(self, want_val=True, want_rhs=True):
        n_rows, nnz = self.csr_dims()
        val = np.empty(nnz, dtype=np.float64) if want_val else None
        rhs = np.empty(n_rows, dtype=np.float64) if want_rhs else None
        self._ck(self._lib.rdc_csr_download(self._h, _dp(val) if want_val else None, _dp(rhs) if want_rhs else None))
        return val, rhs

    def csr_download_rows(self, node_begin, node_end, val_ptr, rhs_ptr, asynchronous=False):
        """rows of nodes [node_begin, node_end) into full-size host arrays given by ADDRESS (e.g. pinned torch tensors)"""
        self._ck(self._lib.rdc_csr_download_rows(self._h, int(node_begin), int(node_end), C.c_void_p(int(val_ptr) if val_ptr else None),
                                                 C.c_void_p(int(rhs_ptr) if rhs_ptr else None), 1 if asynchronous else 0))

    # -- device-resident linear solve
    def csr_matvec_device(self, x_ptr, y_ptr):
        """y[n_owned*nvar] = A x[n_node*nvar] on device addresses; enqueued on the context's stream, no synchronise"""
        self._ck(self._lib.rdc_csr_matvec(self._h, C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr))))

    def csr_matvec(self, x):
        """numpy in, numpy out (tests): x over owned and ghost dofs, y over the owned rows"""
        import torch
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != self.n_node * self.nvar:
            raise ValueError("x must have n_node * nvar entries")
        dev = torch.device("cuda", self.device)
        xd = torch.from_numpy(x).to(dev)
        yd = torch.empty(self.n_owned * self.nvar, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.csr_matvec_device(xd.data_ptr(), yd.data_ptr())
        self.synchronize()
        return yd.cpu().numpy()

    def csr_scale_f32(self, precond=PRECOND_BLOCK_JACOBI):
        """rdc_csr_scale_f32: builds D^-1 and the fp32 copy of D^-1 A from the current values (raises RdcError, invalid,
        if a diagonal block is not invertible or an entry is not finite in fp32)"""
        self._ck(self._lib.rdc_csr_scale_f32(self._h, int(precond)))

    def csr_matvec_f32_device(self, x_ptr, y_ptr):
        """y[n_owned*nvar] = fl32(D^-1 A) x[n_node*nvar] on device addresses (FP64 vectors), with the copy the last
        csr_scale_f32 / solve(mixed=True) built; enqueued on the context's stream, no synchronise"""
        self._ck(self._lib.rdc_csr_matvec_f32(self._h, C.c_void_p(int(x_ptr)), C.c_void_p(int(y_ptr))))

    def csr_matvec_f32(self, x):
        """numpy in, numpy out (tests), as csr_matvec"""
        import torch
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != self.n_node * self.nvar:
            raise ValueError("x must have n_node * nvar entries")
        dev = torch.device("cuda", self.device)
        xd = torch.from_numpy(x).to(dev)
        yd = torch.empty(self.n_owned * self.nvar, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        self.csr_matvec_f32_device(xd.data_ptr(), yd.data_ptr())
        self.synchronize()
        return yd.cpu().numpy()

    def solve(self, x=None, *, field=None, rel_tol=1e-8, abs_tol=0.0, max_its=10000, precond=PRECOND_BLOCK_JACOBI, rhs_scale=1.0,
              mixed=False):
        """rdc_solve on the values and rhs of the last assemble call.  x: device address of n_owned*nvar doubles
        (initial guess in, solution out); or field=FIELD_*: the device storage of that field is used in place.
        mixed=True: rdc_solve_mixed, the iteration streams an fp32 copy of D^-1 A (info.matrix_bits tells).
        precond=PRECOND_MULTIGRID: block Jacobi's system with an aggregation-multigrid cycle applied from the right: same
        stopping test and norms, fewer iterations (mg_levels(), mg_stats(); damping: set_option("mg_omega", thousandths)).
        set_option("mg_smoother", 1): every sweep of the cycle but the first on each level is a forward multicolour Gauss-Seidel
        sweep, undamped (mg_colours(); default 0 = damped block Jacobi; not on a ghosted context, not in solve_dist;
        set_option("mg_gs_fuse", 0): one launch per colour on the small levels too, same bytes).
        precond=PRECOND_ILU0: block Jacobi's system with a multicolour block ILU(0) of D^-1 A applied from the right, factored
        anew by every solve (ilu_stats(); not on a ghosted context, not in solve_dist; the factor is FP64, so not with mixed=True --
        unless set_option("ilu_factor_bits", 32): the sweeps then stream an fp32 copy of the FP64 factor, with or without
        mixed=True, and ilu_factor_bits() tells what they streamed).
        precond=PRECOND_ILU0_LOCAL: the rank-local form of solve_dist; without ghosts it returns the bytes of PRECOND_ILU0.
        precond=PRECOND_MULTIGRID_GS_LOCAL: the multigrid of solve_dist with the rank-local Gauss-Seidel smoother; without ghosts
        it returns the bytes of PRECOND_MULTIGRID under set_option("mg_smoother", 1), whatever that option says.
        set_option("solve_method", 1): right-preconditioned restarted GMRES(m) in place of BiCGStab, on the same system with the
        same preconditioners and stopping test (m: set_option("gmres_restart", 1 .. 128), default 30; set_option("gmres_refine", 1):
        a second Gram-Schmidt pass per step).  info.iterations then counts Arnoldi steps, info.restarts the cycles after the first;
        gmres_stats() tells what the basis costs.  Default 0 = BiCGStab; not in solve_dist."""
        if (x is None) == (field is None):
            raise ValueError("give either a device address or field=")
        if field is not None:
            x = self.field_device_ptr(int(field), self.n_node * self.nvar)
        p = SolveParams(float(rel_tol), float(abs_tol), float(rhs_scale), int(max_its), int(precond))
        info = SolveInfo()
        fn = self._lib.rdc_solve_mixed if mixed else self._lib.rdc_solve
        self._ck(fn(self._h, C.byref(p), C.c_void_p(int(x)), C.byref(info)))
        return info

    def solve_dist_plan(self, send_nodes):
        """rdc_solve_dist_plan: the send list (owned local node ids, send order) of the uploaded mesh; reads the option
        "interior_nodes" as it stands (set it before mesh_upload) and checks that no row below it has a ghost column"""
        ids = np.ascontiguousarray(send_nodes, dtype=np.int32).reshape(-1)
        self._dist_plan = None
        self._ck(self._lib.rdc_solve_dist_plan(self._h, ids.size, ids.ctypes.data_as(C.POINTER(C.c_int32))))

    def solve_dist(self, comm, x=None, *, field=None, rel_tol=1e-8, abs_tol=0.0, max_its=10000, precond=PRECOND_BLOCK_JACOBI,
                   rhs_scale=1.0, mixed=False):
        """rdc_solve_dist: the solve of `solve`, across the ranks of comm (halo.SolveComm), every rank calling with its own
        context.  x: device address of n_node*nvar doubles in local numbering (owned rows: initial guess in, solution out; ghost
        rows: ignored in, the owners' values out), or field=FIELD_*.  The returned SolveInfo is the same on every rank.  The send
        list of comm is uploaded once per mesh.  An exception raised inside a callback of comm is re-raised here.
        precond=PRECOND_MULTIGRID needs a communicator with the sized exchange (SolveComm(..., sized=True)) and goes to
        rdc_solve_dist_mg; its peer counts are uploaded with the plan.  precond=PRECOND_MULTIGRID_GS_LOCAL goes the same way: that
        cycle with the multicolour Gauss-Seidel sweep inside every rank and Jacobi between the ranks, the same callbacks, fewer
        iterations; "mg_smoother" is not consulted, and mg_colours() then reports this rank's colours.
        precond=PRECOND_ILU0_LOCAL: block Jacobi between the ranks, the block ILU(0) of every rank's owned square inside it, applied
        from the right; the exchanges and all-reduces of block Jacobi, fewer iterations (not with mixed=True, unless set_option("ilu_factor_bits", 32): an fp32 copy
        of every rank's factor)."""
        if (x is None) == (field is None):
            raise ValueError("give either a device address or field=")
        if field is not None:
            x = self.field_device_ptr(int(field), self.n_node * self.nvar)
        sized = getattr(comm, "sized_struct", None)
        if self._dist_plan is not comm:
            self.solve_dist_plan(comm.send_nodes)
            if sized is not None:
                sc, gc = (np.ascontiguousarray(a, dtype=np.int64) for a in comm.peer_counts)
                i64p = C.POINTER(C.c_int64)
                self._ck(self._lib.rdc_solve_dist_plan_peers(self._h, sc.size, sc.ctypes.data_as(i64p), gc.ctypes.data_as(i64p)))
            self._dist_plan = comm
        p = SolveParams(float(rel_tol), float(abs_tol), float(rhs_scale), int(max_its), int(precond))
        info = SolveInfo()
        comm.error = None
        if sized is not None and int(precond) in (PRECOND_MULTIGRID, PRECOND_MULTIGRID_GS_LOCAL):
            rc = self._lib.rdc_solve_dist_mg(self._h, C.byref(p), C.byref(sized), 1 if mixed else 0, C.c_void_p(int(x)), C.byref(info))
        else:
            rc = self._lib.rdc_solve_dist(self._h, C.byref(p), C.byref(comm.struct), 1 if mixed else 0, C.c_void_p(int(x)), C.byref(info))
        if comm.error is not None:
            err, comm.error = comm.error, None
            raise err
        self._ck(rc)
        return info

    def _dist_plan_for(self, comm):
        """the send list of comm, and its peer counts if it has the sized exchange, uploaded once per mesh and communicator"""
        if self._dist_plan is comm:
            return
        self.solve_dist_plan(comm.send_nodes)
        if getattr(comm, "sized_struct", None) is not None:
            sc, gc = (np.ascontiguousarray(a, dtype=np.int64) for a in comm.peer_counts)
            i64p = C.POINTER(C.c_int64)
            self._ck(self._lib.rdc_solve_dist_plan_peers(self._h, sc.size, sc.ctypes.data_as(i64p), gc.ctypes.data_as(i64p)))
        self._dist_plan = comm

    def solve_dist_gmres(self, comm, x=None, *, field=None, rel_tol=1e-8, abs_tol=0.0, max_its=10000, precond=PRECOND_BLOCK_JACOBI,
                         rhs_scale=1.0, mixed=False):
        """rdc_solve_dist_gmres: right-preconditioned restarted GMRES(m) across the ranks of comm, which must be a
        halo.SolveComm(..., wide=True).  Arguments, x and the returned SolveInfo as solve_dist; iterations counts Arnoldi steps and
        restarts the cycles after the first, as in solve under set_option("solve_method", 1).  GMRES runs whatever "solve_method"
        is; "gmres_restart" and "gmres_refine" are honoured.  precond: PRECOND_NONE, _JACOBI, _BLOCK_JACOBI, PRECOND_ILU0_LOCAL
        (block Jacobi between the ranks, ILU(0) inside each: PETSc's default under mpirun) and PRECOND_MULTIGRID or PRECOND_MULTIGRID_GS_LOCAL (the rank-local
        hierarchy of solve_dist).  An exception raised inside a callback of comm is re-raised here."""
        wide = getattr(comm, "wide_struct", None)
        if wide is None:
            raise ValueError("solve_dist_gmres needs a communicator with the wide all-reduce: SolveComm(..., wide=True)")
        if (x is None) == (field is None):
            raise ValueError("give either a device address or field=")
        if field is not None:
            x = self.field_device_ptr(int(field), self.n_node * self.nvar)
        self._dist_plan_for(comm)
        p = SolveParams(float(rel_tol), float(abs_tol), float(rhs_scale), int(max_its), int(precond))
        info = SolveInfo()
        comm.error = None
        rc = self._lib.rdc_solve_dist_gmres(self._h, C.byref(p), C.byref(wide), 1 if mixed else 0, C.c_void_p(int(x)), C.byref(info))
        if comm.error is not None:
            err, comm.error = comm.error, None
            raise err
        self._ck(rc)
        return info

    def gmres_arnoldi_dist(self, comm, v0, steps, precond, mixed=False):
        """rdc_solve_dist_gmres_arnoldi, numpy in, numpy out (tests; collective): v0 = this rank's owned rows (n_owned * nvar) ->
        (V [steps_done + 1][n_owned * nvar], this rank's owned rows of the basis; H [restart + 1][restart], the same on every
        rank).  comm: SolveComm(..., wide=True); restart as in gmres_arnoldi."""
        import torch
        wide = getattr(comm, "wide_struct", None)
        if wide is None:
            raise ValueError("gmres_arnoldi_dist needs a communicator with the wide all-reduce: SolveComm(..., wide=True)")
        v0 = np.ascontiguousarray(v0, dtype=np.float64).reshape(-1)
        n = self.n_owned * self.nvar
        if v0.size != n:
            raise ValueError("v0 must have n_owned * nvar entries")
        self._dist_plan_for(comm)
        restart = getattr(self, "_gmres_restart", 30)
        dev = torch.device("cuda", self.device)
        vd = torch.from_numpy(v0).to(dev)
        Vd = torch.zeros(max((int(steps) + 1) * n, 1), dtype=torch.float64, device=dev)
        H = np.zeros((restart, restart + 1), dtype=np.float64)   # column-major (restart + 1) x restart
        done = C.c_int32()
        torch.cuda.synchronize(dev)
        comm.error = None
        rc = self._lib.rdc_solve_dist_gmres_arnoldi(self._h, C.byref(wide), int(precond), 1 if mixed else 0, C.c_void_p(vd.data_ptr()),
                                                    int(steps), C.c_void_p(Vd.data_ptr()), _dp(H), C.byref(done))
        if comm.error is not None:
            err, comm.error = comm.error, None
            raise err
        self._ck(rc)
        return Vd.cpu().numpy()[:(int(steps) + 1) * n].reshape(int(steps) + 1, n)[:done.value + 1], H.T.copy()

    def mg_levels(self):
        """[(nodes, node blocks)] of every level of the hierarchy of the last multigrid solve on this mesh, level 0 = the matrix"""
        n = C.c_int32()
        self._ck(self._lib.rdc_solve_mg_levels(self._h, C.byref(n), None, None, 0))
        nodes, blocks = (C.c_int64 * n.value)(), (C.c_int64 * n.value)()
        self._ck(self._lib.rdc_solve_mg_levels(self._h, C.byref(n), nodes, blocks, n.value))
        return [(int(nodes[i]), int(blocks[i])) for i in range(n.value)]

    def mg_stats(self):
        """(device ms the last multigrid solve spent building the coarse matrices and their D^-1, device bytes the levels hold)"""
        ms, nbytes = C.c_float(), C.c_int64()
        self._ck(self._lib.rdc_solve_mg_stats(self._h, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value

    def mg_colours(self):
        """[colours] of every level of that hierarchy, as the Gauss-Seidel smoother (set_option("mg_smoother", 1)) sweeps them"""
        n = C.c_int32()
        self._ck(self._lib.rdc_solve_mg_levels(self._h, C.byref(n), None, None, 0))
        colours = (C.c_int32 * n.value)()
        self._ck(self._lib.rdc_solve_mg_colours(self._h, colours, n.value))
        return [int(k) for k in colours]

    def mg_apply_device(self, in_ptr, out_ptr, mixed=False):
        """rdc_solve_mg_apply on device addresses (n_owned*nvar doubles each): out = M in, one multigrid cycle as the next
        solve(precond=PRECOND_MULTIGRID, mixed=mixed) would apply it.  A test hook."""
        self._ck(self._lib.rdc_solve_mg_apply(self._h, 1 if mixed else 0, C.c_void_p(int(in_ptr)), C.c_void_p(int(out_ptr))))

    def mg_apply(self, x, mixed=False):
        """numpy in, numpy out (tests): M x"""
        import torch
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != self.n_owned * self.nvar:
            raise ValueError("x must have n_owned * nvar entries")
        dev = torch.device("cuda", self.device)
        xd = torch.from_numpy(x).to(dev)
        yd = torch.empty_like(xd)
        torch.cuda.synchronize(dev)
        self.mg_apply_device(xd.data_ptr(), yd.data_ptr(), mixed)
        return yd.cpu().numpy()

    def mg_level(self, level):
        """rdc_solve_mg_level_download -> (val, dinv) of a level as the last mg_apply or multigrid solve built them: val
        [blocks * nvar^2] in the node-block layout over the level's pattern (None for level 0, the matrix itself), dinv
        [nodes][nvar][nvar].  A test hook."""
        levels = self.mg_levels()
        if not 0 <= int(level) < len(levels):
            self._ck(self._lib.rdc_solve_mg_level_download(self._h, int(level), None, None))
        n, blocks = levels[int(level)]
        nv = self.nvar
        val = np.empty(blocks * nv * nv, dtype=np.float64) if level else None
        dinv = np.empty((n, nv, nv), dtype=np.float64)
        self._ck(self._lib.rdc_solve_mg_level_download(self._h, int(level), _dp(val) if level else None, _dp(dinv)))
        return val, dinv

    def gmres_stats(self):
        """rdc_solve_gmres_stats -> (restart length, device bytes of the basis, cycles) of the last GMRES solve on this mesh"""
        m, nbytes, cycles = C.c_int32(), C.c_int64(), C.c_int32()
        self._ck(self._lib.rdc_solve_gmres_stats(self._h, C.byref(m), C.byref(nbytes), C.byref(cycles)))
        return m.value, nbytes.value, cycles.value

    def gmres_arnoldi_device(self, v0_ptr, steps, precond, V_ptr, H, mixed=False):
        """rdc_solve_gmres_arnoldi on device addresses: v0 (n_owned*nvar doubles) in, the basis vectors into V (room for steps + 1),
        the raw Hessenberg matrix into the host array H ((restart + 1) x restart, column-major).  Returns the steps done.  A test hook."""
        done = C.c_int32()
        self._ck(self._lib.rdc_solve_gmres_arnoldi(self._h, int(precond), 1 if mixed else 0, C.c_void_p(int(v0_ptr)), int(steps),
                                                   C.c_void_p(int(V_ptr)), _dp(H), C.byref(done)))
        return done.value

    def gmres_arnoldi(self, v0, steps, precond, mixed=False):
        """numpy in, numpy out (tests): (V [steps_done + 1][n], H [restart + 1][restart]) of `steps` Arnoldi steps from v0 / ||v0||
        as a GMRES solve with `precond` would take them; restart = the option "gmres_restart" as this wrapper last set it"""
        import torch
        v0 = np.ascontiguousarray(v0, dtype=np.float64).reshape(-1)
        n = self.n_owned * self.nvar
        if v0.size != n:
            raise ValueError("v0 must have n_owned * nvar entries")
        restart = getattr(self, "_gmres_restart", 30)
        dev = torch.device("cuda", self.device)
        vd = torch.from_numpy(v0).to(dev)
        Vd = torch.zeros((int(steps) + 1) * n, dtype=torch.float64, device=dev)
        H = np.zeros((restart, restart + 1), dtype=np.float64)   # column-major (restart + 1) x restart
        torch.cuda.synchronize(dev)
        done = self.gmres_arnoldi_device(vd.data_ptr(), steps, precond, Vd.data_ptr(), H, mixed)
        return Vd.cpu().numpy().reshape(int(steps) + 1, n)[:done + 1], H.T.copy()

    def ilu_stats(self):
        """(device ms the last ILU(0) solve spent on the copy of D^-1 A and its factorisation, device bytes the factor holds, colours)"""
        ms, nbytes, ncol = C.c_float(), C.c_int64(), C.c_int32()
        self._ck(self._lib.rdc_solve_ilu_stats(self._h, C.byref(ms), C.byref(nbytes), C.byref(ncol)))
        return ms.value, nbytes.value, ncol.value

    def ilu_factor_bits(self):
        """rdc_solve_ilu_factor_bits: what the sweeps of the last ILU(0) solve or apply hook streamed, 32 (the fp32 copy of the
        factor, set_option("ilu_factor_bits", 32)) or 64 (the default, or the fall-back of a factor that does not fit fp32)"""
        bits = C.c_int32()
        self._ck(self._lib.rdc_solve_ilu_factor_bits(self._h, C.byref(bits)))
        return bits.value

    def ilu_apply_device(self, in_ptr, out_ptr):
        """rdc_solve_ilu_apply on device addresses (n_owned*nvar doubles each): out = (LU)^-1 in, as the next
        solve(precond=PRECOND_ILU0) would apply it.  A test hook."""
        self._ck(self._lib.rdc_solve_ilu_apply(self._h, C.c_void_p(int(in_ptr)), C.c_void_p(int(out_ptr))))

    def ilu_apply(self, x):
        """numpy in, numpy out (tests): M x"""
        import torch
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != self.n_owned * self.nvar:
            raise ValueError("x must have n_owned * nvar entries")
        dev = torch.device("cuda", self.device)
        xd = torch.from_numpy(x).to(dev)
        yd = torch.empty_like(xd)
        torch.cuda.synchronize(dev)
        self.ilu_apply_device(xd.data_ptr(), yd.data_ptr())
        return yd.cpu().numpy()

    def ilu_factor(self):
        """rdc_solve_ilu_download -> (val, uinv) as the last ilu_apply or ILU(0) solve built them: val [nnz] in the node-block layout
        of the CSR values, L and U blocks in the positions of the blocks they replace (L's identity not stored); uinv
        [n_owned][nvar][nvar] = U_ii^-1.  A test hook."""
        nv = self.nvar
        val = np.empty(self.csr_dims()[1], dtype=np.float64)
        uinv = np.empty((self.n_owned, nv, nv), dtype=np.float64)
        self._ck(self._lib.rdc_solve_ilu_download(self._h, _dp(val), _dp(uinv)))
        return val, uinv

    def ilu_local_apply_device(self, in_ptr, out_ptr):
        """rdc_solve_ilu_local_apply on device addresses (n_owned*nvar doubles each): out = (LU)^-1 in with the ILU(0) of this
        rank's owned square, as the next solve_dist(precond=PRECOND_ILU0_LOCAL) would apply it; takes a ghosted context.  A test hook."""
        self._ck(self._lib.rdc_solve_ilu_local_apply(self._h, C.c_void_p(int(in_ptr)), C.c_void_p(int(out_ptr))))

    def ilu_local_apply(self, x):
        """numpy in, numpy out (tests): M x, n_owned*nvar entries each"""
        import torch
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != self.n_owned * self.nvar:
            raise ValueError("x must have n_owned * nvar entries")
        dev = torch.device("cuda", self.device)
        xd = torch.from_numpy(x).to(dev)
        yd = torch.empty_like(xd)
        torch.cuda.synchronize(dev)
        self.ilu_local_apply_device(xd.data_ptr(), yd.data_ptr())
        return yd.cpu().numpy()

    def ilu_local_factor(self):
        """rdc_solve_ilu_local_download -> (val, uinv) as the last ilu_local_apply or solve with PRECOND_ILU0_LOCAL built them: val
        in the layout of a node-block CSR restricted to the owned columns (per node [var a][owned block k][var b], the nodes one
        behind the other; no position for a ghost block), uinv [n_owned][nvar][nvar] = U_ii^-1.  A test hook."""
        nv = self.nvar
        rp, col = self.csr_pattern()
        val = np.empty(int(np.count_nonzero(col[:rp[self.n_owned * nv]] < self.n_owned * nv)), dtype=np.float64)
        uinv = np.empty((self.n_owned, nv, nv), dtype=np.float64)
        self._ck(self._lib.rdc_solve_ilu_local_download(self._h, _dp(val), _dp(uinv)))
        return val, uinv

    def part1_nodes(self):
        n = C.c_int64()
        self._ck(self._lib.rdc_part1_nodes(self._h, C.byref(n)))
        return n.value

    # -- instrumentation
    def timing_enable(self, on=True):
        self._ck(self._lib.rdc_timing_enable(self._h, 1 if on else 0))

    def timing_last_ms(self):
        ms = C.c_float()
        self._ck(self._lib.rdc_timing_last_ms(self._h, C.byref(ms)))
        return ms.value

    def timing_sum_ms(self):
        """(total device ms, number of assemble calls) since the last enable / sum; resets the pool."""
        ms, n = C.c_float(), C.c_int()
        self._ck(self._lib.rdc_timing_sum_ms(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timing_samples_ms(self, capacity=4096):
        """device ms of every assemble call since the last enable / sum / samples (oldest first); resets the pool."""
        buf = (C.c_float * capacity)()
        n = C.c_int()
        self._ck(self._lib.rdc_timing_samples_ms(self._h, buf, capacity, C.byref(n)))
        return [buf[i] for i in range(min(n.value, capacity))]
