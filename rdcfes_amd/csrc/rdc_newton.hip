// rdc_newton.hip — rdc_solid_newton and rdc_solid_newton_dist (include/rdc_assembly.h): the Newton loop of the solid system around
// the entries the library already has.  The decisions are newton_next (rdc_newton.h); this file executes its actions:
// rdc_solid_assemble, a linear entry with everything it brings (protocol, preconditioners, settings, failure handling) -- rdc_solve or
// rdc_solve_mixed, across ranks the partitioned entry newton_linear_dispatch names -- and three small kernels for what lies between
// them.  No matrix, rhs or vector crosses the bus; what the host reads is stated in rdc_newton.h.
//
// Across ranks the loop adds two things of its own: one exchange of the coordinates on entry, and one allreduce_sum of the whole
// record (NEWTON_REC_DOUBLES doubles) before each host read.  Every sum runs over the owned entries, in the fixed chunk order; the
// coordinates move over all local entries, from a delta whose ghost tail the partitioned linear entry filled with the owners' values.
#include <cmath>

#include "rdc_capi_internal.h"

using namespace rdc;

namespace {

// the sums of a workgroup of 256 in a fixed order: thread 0 writes them to partials[block * NC + c]
template <int NC>
__device__ __forceinline__ void newton_block_partials(const double (&c)[NC], double* __restrict__ partials) {
  __shared__ double sh[NC][256];
#pragma unroll
  for (int k = 0; k < NC; k++) sh[k][threadIdx.x] = c[k];
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off)
#pragma unroll
      for (int k = 0; k < NC; k++) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < NC; k++) partials[(int64_t)blockIdx.x * NC + k] = sh[k][0];
}

// partials of ||r||^2: workgroup b sums the entries [b * NEWTON_CHUNK, (b + 1) * NEWTON_CHUNK) of r, every thread its four in order
__global__ __launch_bounds__(256) void k_newton_norm(const double* __restrict__ r, int64_t n, double* __restrict__ partials) {
  const int64_t i0 = (int64_t)blockIdx.x * NEWTON_CHUNK + threadIdx.x;
  double c[1] = {0.0};
#pragma unroll
  for (int q = 0; q < NEWTON_CHUNK / 256; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) c[0] = fma(r[i], r[i], c[0]);
  }
  newton_block_partials<1>(c, partials);
}

// One entry of the update, for owned and ghost entries alike: a ghost coordinate stays bit for bit its owner's because both ranks
// run this on the same three numbers.  step == 0 is the restore: u = u0 whatever delta holds.
struct NewtonMove { double d, u; };
__device__ __forceinline__ NewtonMove newton_move(double u0, double delta, double step) {
  NewtonMove m;
  m.d = step == 0.0 ? 0.0 : step * delta;
  m.u = u0 + m.d;
  return m;
}

// xyz = u0 + step * delta over the n entries of the coordinate array, whose layout [node][3] is the dof layout; partials of
// ||step delta||^2 and ||xyz||^2 over the entries below n_sum (the owned ones) in the same pass, in the chunk order of n.
__global__ __launch_bounds__(256) void k_newton_step(const double* __restrict__ u0, const double* __restrict__ delta, double step,
                                                     double* __restrict__ xyz, int64_t n, int64_t n_sum, double* __restrict__ partials) {
  const int64_t i0 = (int64_t)blockIdx.x * NEWTON_CHUNK + threadIdx.x;
  double c[2] = {0.0, 0.0};
#pragma unroll
  for (int q = 0; q < NEWTON_CHUNK / 256; q++) {
    const int64_t i = i0 + q * 256;
    if (i < n) {
      const NewtonMove m = newton_move(u0[i], delta[i], step);
      xyz[i] = m.u;
      if (i < n_sum) {
        c[0] = fma(m.d, m.d, c[0]);
        c[1] = fma(m.u, m.u, c[1]);
      }
    }
  }
  newton_block_partials<2>(c, partials);
}

// u0 = xyz
__global__ __launch_bounds__(256) void k_newton_save(const double* __restrict__ xyz, double* __restrict__ u0, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) u0[i] = xyz[i];
}

// one workgroup adds the partials of the previous kernel in a fixed order: rec->sum[first + c] = sum over b of partials[b * ncomp + c].
// clear: every other double of the record becomes 0 first -- the first sum behind a host read clears, so that an all-reduce of the
// whole record never adds up what an earlier one left.
__global__ __launch_bounds__(1024) void k_newton_sum(const double* __restrict__ partials, int64_t nparts, int ncomp, int first, int clear,
                                                     NewtonRec* __restrict__ rec) {
  __shared__ double sh[2][1024];
  double s[2] = {0.0, 0.0};
  for (int64_t i = threadIdx.x; i < nparts; i += 1024)
    for (int c = 0; c < ncomp; c++) s[c] += partials[i * ncomp + c];
  sh[0][threadIdx.x] = s[0];
  sh[1][threadIdx.x] = s[1];
  __syncthreads();
  for (int off = 512; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + off];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (clear) {
      for (int k = 0; k < 3; k++) rec->sum[k] = 0.0;
      for (int k = 0; k < NEWTON_REC_DOUBLES - 3; k++) rec->pad[k] = 0.0;
    }
    for (int c = 0; c < ncomp; c++) rec->sum[first + c] = sh[c][0];
  }
}

// the device side of one call: the carved work memory and the arrays of the context it reads and writes
struct NewtonDev {
  NewtonWork w;
  double *u0, *delta, *partials, *send, *xyz;
  const double* rhs;
  NewtonRec* rec;
  hipStream_t stream;
};

// ||rhs||^2 over the owned rows -> rec->sum[NEWTON_SUM_RESIDUAL].  A rank without owned rows launches only the sum, which gives 0.
hipError_t enqueue_norm(const NewtonDev& d, bool clear) {
  const int64_t blocks = (d.w.n_owned + NEWTON_CHUNK - 1) / NEWTON_CHUNK;
  if (blocks > 0) hipLaunchKernelGGL(k_newton_norm, dim3((unsigned)blocks), dim3(256), 0, d.stream, d.rhs, d.w.n_owned, d.partials);
  hipLaunchKernelGGL(k_newton_sum, dim3(1), dim3(1024), 0, d.stream, (const double*)d.partials, blocks, 1, (int)NEWTON_SUM_RESIDUAL, clear ? 1 : 0, d.rec);
  return hipGetLastError();
}

// coordinates = u0 + step delta over all local entries; ||step delta||^2, ||u||^2 over the owned ones -> rec->sum[NEWTON_SUM_STEP],
// [NEWTON_SUM_SOLUTION].  Always the first sum behind a host read: it clears the record.
hipError_t enqueue_step(const NewtonDev& d, double step) {
  if (d.w.blocks > 0)
    hipLaunchKernelGGL(k_newton_step, dim3((unsigned)d.w.blocks), dim3(256), 0, d.stream, (const double*)d.u0, (const double*)d.delta, step, d.xyz,
                       d.w.n, d.w.n_owned, d.partials);
  hipLaunchKernelGGL(k_newton_sum, dim3(1), dim3(1024), 0, d.stream, (const double*)d.partials, d.w.blocks, 2, (int)NEWTON_SUM_STEP, 1, d.rec);
  return hipGetLastError();
}

// Both entries.  comm == nullptr: rdc_solid_newton, single partition.  Otherwise rdc_solid_newton_dist: the norms are global, the
// linear solve is the partitioned entry of `how`, and *comm_rc takes the first non-zero return of a callback the loop itself made
// (a linear entry reports its own through RDC_ERR_COMM).
int newton_run(rdc_ctx* c, const rdc_solid_params* p, const rdc_solid_newton_params* np, const rdc_solve_comm_wide* comm, NewtonDispatch how,
               rdc_solid_newton_info* info, const char* name) {
  const HostPrep& P = c->ms.prep;
  int rc = set_device(c);
  if (rc) return rc;

  NewtonDev d;
  const SolveState& S = c->ms.solve;
  const int64_t n_send = comm && S.plan_ready ? S.dist.n_send : 0;
  d.w = comm ? newton_carve_dist(P.n_node, P.n_owned, n_send) : newton_carve(P.n_node, P.n_owned);
  if (c->buf.solve.newton.bytes != d.w.bytes && (rc = dev_alloc(c, c->buf.solve.newton, d.w.bytes))) return rc;
  if (!c->newton_rec) RDC_HIP(c, hipHostMalloc((void**)&c->newton_rec, sizeof(NewtonRec), hipHostMallocDefault));
  double* base = (double*)c->buf.solve.newton.p;
  d.u0 = base + d.w.u0; d.delta = base + d.w.delta; d.partials = base + d.w.partials; d.rec = (NewtonRec*)(base + d.w.rec);
  d.send = base + d.w.send;
  d.xyz = (double*)c->buf.mesh.xyz.p;
  d.rhs = (const double*)c->buf.out.rhs.p;
  d.stream = c->stream;

  hipEvent_t ev[2] = {nullptr, nullptr};
  RDC_HIP(c, hipEventCreate(&ev[0]));
  if (hipEventCreate(&ev[1]) != hipSuccess) { (void)hipEventDestroy(ev[0]); return fail(c, RDC_ERR_HIP, "hipEventCreate failed"); }
  (void)hipEventRecord(ev[0], c->stream);

  rdc_solve_params lin = np->linear;
  lin.rhs_scale = -1.0;   // J delta = -R
  NewtonState s;
  NewtonNorms m;
  hipError_t e = hipSuccess;
  rc = RDC_OK;
  int comm_rc = 0;   // the first non-zero return of a callback of the loop: nothing is called after it
  const rdc_solve_comm* cb = comm ? &comm->sized.base : nullptr;
  // the record of sums of what has been enqueued: the one host read behind an assembly or a step; across ranks summed over them first
  auto read_rec = [&]() {
    if (cb && e == hipSuccess && (comm_rc = cb->allreduce_sum(cb->user, (double*)d.rec, NEWTON_REC_DOUBLES, (void*)c->stream))) return;
    if (e == hipSuccess) e = hipMemcpyAsync(c->newton_rec, d.rec, sizeof(NewtonRec), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  };
  auto assemble = [&](int jacobian, bool clear) {
    if ((rc = rdc_solid_assemble(c, p, jacobian))) return;
    e = enqueue_norm(d, clear);
  };
  // On entry across ranks: the ghost coordinates become the owners'.  From here on every rank moves them itself (k_newton_step).
  if (cb) {
    e = solve_halo_pack(3, (const int32_t*)c->buf.solve.send.p, n_send, (const double*)d.xyz, d.send, c->stream);
    if (e == hipSuccess) comm_rc = cb->exchange_begin(cb->user, d.send, d.xyz + d.w.n_owned, (void*)c->stream);
    if (e == hipSuccess && !comm_rc) comm_rc = cb->exchange_end(cb->user, (void*)c->stream);
    c->const_rows.coords_update();
  }
  // bounded: newton_next hands out at most 1000 iterations of at most 10 halvings, a handful of actions each
  for (int guard = 0; guard < 16 * 1000 + 16 && e == hipSuccess && !comm_rc; guard++) {
    const NewtonAction a = newton_next(*np, s, m);
    m = NewtonNorms();
    if (a == NEWTON_FINISH) break;
    if (a == NEWTON_ASSEMBLE_FULL) {
      assemble(1, true);
      if (rc == RDC_OK) read_rec();
      m.residual = std::sqrt(c->newton_rec->sum[NEWTON_SUM_RESIDUAL]);
    } else if (a == NEWTON_SOLVE) {
      if (d.w.n > 0) hipLaunchKernelGGL(k_newton_save, dim3((unsigned)((d.w.n + 255) / 256)), dim3(256), 0, c->stream, (const double*)d.xyz, d.u0, d.w.n);
      e = hipGetLastError();
      // delta = 0: the start of the linear solve on the owned rows; the ghost tail too, so that no entry of it is ever undefined
      if (e == hipSuccess && d.w.n_delta > 0) e = hipMemsetAsync(d.delta, 0, (size_t)d.w.n_delta * sizeof(double), c->stream);
      if (e != hipSuccess) break;
      rdc_solve_info li = rdc_solve_info();
      if (!comm) rc = np->mixed ? rdc_solve_mixed(c, &lin, d.delta, &li) : rdc_solve(c, &lin, d.delta, &li);
      else if (how.entry == NEWTON_LINEAR_DIST_GMRES) rc = rdc_solve_dist_gmres(c, &lin, comm, np->mixed, d.delta, &li);
      else if (how.entry == NEWTON_LINEAR_DIST_MG) rc = rdc_solve_dist_mg(c, &lin, &comm->sized, np->mixed, d.delta, &li);
      else rc = rdc_solve_dist(c, &lin, cb, np->mixed, d.delta, &li);
      m.linear_reason = li.reason;
      m.linear_iterations = li.iterations;
    } else if (a == NEWTON_TRY_STEP || a == NEWTON_HALVE) {
      c->const_rows.coords_update();
      e = enqueue_step(d, s.step);
      if (e == hipSuccess && s.measure) assemble(0, false);
      if (rc == RDC_OK) read_rec();
      m.step_norm = std::sqrt(c->newton_rec->sum[NEWTON_SUM_STEP]);
      m.solution_norm = std::sqrt(c->newton_rec->sum[NEWTON_SUM_SOLUTION]);
      m.residual = std::sqrt(c->newton_rec->sum[NEWTON_SUM_RESIDUAL]);
    } else {   // NEWTON_ACCEPT
      c->newton_history.add(s.rn, s.step, s.lin_its, s.lin_reason);
      if (s.measure) {
        assemble(0, true);
        if (rc == RDC_OK) read_rec();
        m.residual = std::sqrt(c->newton_rec->sum[NEWTON_SUM_RESIDUAL]);
      }
    }
    if (rc != RDC_OK) break;
  }
  if (rc == RDC_OK && e == hipSuccess && !comm_rc && s.last == NEWTON_FINISH) {
    if (s.info.reason == RDC_NEWTON_LINEAR_FAILED) c->newton_history.add(s.rn, 0.0, s.lin_its, s.lin_reason);
    if (s.restore) {   // the saved iterate, by a step of length 0: ghost entries included, so no message
      c->const_rows.coords_update();
      e = enqueue_step(d, 0.0);
    }
  }
  if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  if (rc != RDC_OK) {   // an entry of the loop refused or failed; its message stands.  The coordinates move only behind a solve that returned RDC_OK
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  if (comm_rc) {   // the coordinates are as the last executed action left them
    (void)hipStreamSynchronize(c->stream);
    return fail(c, RDC_ERR_COMM, "a communication callback returned %d; %s was abandoned", comm_rc, name);
  }
  if (e != hipSuccess) return fail(c, RDC_ERR_HIP, "%s failed: %s", name, hipGetErrorString(e));
  if (s.last != NEWTON_FINISH) return fail(c, RDC_ERR_STATE, "%s: the loop did not end within its bound", name);
  *info = s.info;
  info->device_ms = ms;
  return RDC_OK;
}

// what both entries refuse before anything is launched or called, up to the point where they differ (ghost nodes)
int newton_refuse_setup(rdc_ctx* c, const char* name) {
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "%s called before rdc_mesh_upload", name);
  // what rdc_solid_assemble refuses
  if (c->ms.prep.nvar != 3) return fail(c, RDC_ERR_INVALID, "solid system needs nvar=3");
  if (!c->buf.field[RDC_FIELD_UNDEFORMED_XYZ].p) return fail(c, RDC_ERR_STATE, "undeformed coordinates not set");
  if (!c->buf.field[RDC_FIELD_ELEM_FIBRE].p) return fail(c, RDC_ERR_STATE, "fibre field not set");
  if (c->ms.n_materials <= 0) return fail(c, RDC_ERR_STATE, "materials not set");
  return RDC_OK;
}

}  // namespace

extern "C" {

int rdc_solid_newton(rdc_ctx* c, const rdc_solid_params* p, const rdc_solid_newton_params* np, rdc_solid_newton_info* info) {
  if (!c) return RDC_ERR_INVALID;
  if (!p || !np || !info) return fail(c, RDC_ERR_INVALID, "null argument");
  if (int rc = newton_refuse_setup(c, "rdc_solid_newton")) return rc;
  const HostPrep& P = c->ms.prep;
  if (P.n_owned < P.n_node)
    return fail(c, RDC_ERR_UNSUPPORTED, "the context has ghost nodes (%lld owned of %lld): a Newton solve across partitions needs global norms "
                "and a partitioned linear solve inside the loop: rdc_solid_newton_dist", (long long)P.n_owned, (long long)P.n_node);
  if (const char* bad = newton_check_params(*np)) return fail(c, RDC_ERR_INVALID, "%s", bad);
  if (c->opt.part != 0) return fail(c, RDC_ERR_STATE, "rdc_solid_newton assembles whole: not inside a two-part call");
  *info = rdc_solid_newton_info();
  c->newton_history.clear();
  if (P.n_owned == 0) return RDC_OK;   // no unknowns: converged, nothing to launch
  return newton_run(c, p, np, nullptr, NewtonDispatch(), info, "rdc_solid_newton");
}

int rdc_solid_newton_dist(rdc_ctx* c, const rdc_solid_params* p, const rdc_solid_newton_params* np, const rdc_solve_comm_wide* comm,
                          rdc_solid_newton_info* info) {
  if (!c) return RDC_ERR_INVALID;
  if (!p || !np || !comm || !info) return fail(c, RDC_ERR_INVALID, "null argument");
  if (int rc = newton_refuse_setup(c, "rdc_solid_newton_dist")) return rc;
  const HostPrep& P = c->ms.prep;
  if (P.n_owned < P.n_node && !c->ms.solve.plan_ready)
    return fail(c, RDC_ERR_STATE, "the context has ghost nodes (%lld owned of %lld) and no send list: call rdc_solve_dist_plan first",
                (long long)P.n_owned, (long long)P.n_node);
  if (const char* bad = newton_check_params(*np)) return fail(c, RDC_ERR_INVALID, "%s", bad);
  if (c->opt.part != 0) return fail(c, RDC_ERR_STATE, "rdc_solid_newton_dist assembles whole: not inside a two-part call");
  const NewtonDispatch how = newton_linear_dispatch(np->linear.precond, c->sopt.solve_method);
  if (!newton_comm_complete(*comm, how))
    return fail(c, RDC_ERR_INVALID, "the communicator lacks a callback: exchange_begin, exchange_end and allreduce_sum always, the sized pair for "
                "precond %d and %d, allreduce_sum_wide under \"solve_method\" = 1", (int)RDC_PRECOND_MULTIGRID, (int)RDC_PRECOND_MULTIGRID_GS_LOCAL);
  *info = rdc_solid_newton_info();
  c->newton_history.clear();
  // a rank without owned nodes does not return early: it takes part in every callback with zero sums
  return newton_run(c, p, np, comm, how, info, "rdc_solid_newton_dist");
}

int rdc_solid_newton_history(rdc_ctx* c, int cap, double* residual, double* step, int32_t* lin_its, int32_t* lin_reason, int32_t* n) {
  if (!c || !n || cap < 0) return RDC_ERR_INVALID;
  const NewtonHistory& h = c->newton_history;
  *n = (int32_t)h.residual.size();
  for (int i = 0; i < *n && i < cap; i++) {
    if (residual) residual[i] = h.residual[(size_t)i];
    if (step) step[i] = h.step[(size_t)i];
    if (lin_its) lin_its[i] = h.lin_its[(size_t)i];
    if (lin_reason) lin_reason[i] = h.lin_reason[(size_t)i];
  }
  return RDC_OK;
}

}  // extern "C"
