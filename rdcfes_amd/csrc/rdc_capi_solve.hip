// rdc_capi_solve.hip — the linear-solve part of the C-ABI (include/rdc_assembly.h) over rdc_solve.hip.  Every entry that runs a solve
// follows one protocol: solve_enter | its own refusals (check_solve_params where it takes rdc_solve_params) | solve_do, which builds
// the device view, runs and leaves.  What the cached artefacts are worth afterwards is decided by rdc_solve_state.h alone.
#include <algorithm>
#include <cmath>
#include <utility>

#include "rdc_capi_internal.h"

using namespace rdc;

namespace {

// what rdc_solve.hip needs of the context; uploads the block column list the first time (4 bytes per node block).
// dist: the work buffer is that of a partitioned solve, laid out for these dimensions
int solve_view(rdc_ctx* c, bool want_work, bool want_f32, SolveDev* d, const DistDims* dist = nullptr) {
  int rc = set_device(c);
  if (rc) return rc;
  const HostPrep& P = c->ms.prep;
  if (P.nvar != 3 && P.nvar != 5) return fail(c, RDC_ERR_UNSUPPORTED, "the linear solve kernels exist for 3 and 5 unknowns per node, not %d", P.nvar);
  if (!c->ms.solve.bcol_ready) {
    if ((rc = dev_upload(c, c->buf.solve.bcol, P.bcol))) return rc;
    RDC_HIP(c, hipStreamSynchronize(c->stream));
    c->ms.solve.bcol_ready = true;
  }
  d->nvar = P.nvar; d->n_owned = P.n_owned; d->n_nodes = P.n_node;
  d->bptr = (const int64_t*)c->buf.mesh.bptr.p; d->bcol = (const int32_t*)c->buf.solve.bcol.p;
  d->val = (const double*)c->buf.out.val.p; d->rhs = (const double*)c->buf.out.rhs.p;
  d->stream = c->stream;
  if (want_work) {
    if ((rc = dev_alloc(c, c->buf.solve.work, solve_work_bytes(P.nvar, P.n_owned, dist)))) return rc;
    if (!c->solve_rec) RDC_HIP(c, hipHostMalloc((void**)&c->solve_rec, sizeof(SolveScal), hipHostMallocDefault));
    d->work = (double*)c->buf.solve.work.p;
    d->host_rec = c->solve_rec;
  }
  if (want_f32) {
    if (!c->ms.solve.voff_ready) {   // float offset of every owned node's padded rows (rdc_solve.h, f32_row_stride)
      std::vector<int64_t> voff((size_t)P.n_owned + 1, 0);
      for (int64_t n = 0; n < P.n_owned; n++) voff[(size_t)n + 1] = voff[(size_t)n] + P.nvar * f32_row_stride(P.nvar, P.bptr[(size_t)n + 1] - P.bptr[(size_t)n]);
      if ((rc = dev_upload(c, c->buf.solve.voff, voff))) return rc;
      RDC_HIP(c, hipStreamSynchronize(c->stream));
      if ((rc = dev_alloc(c, c->buf.solve.val32, (size_t)voff.back() * sizeof(float)))) return rc;
      c->ms.solve.voff_ready = true;
    }
    d->voff = (const int64_t*)c->buf.solve.voff.p;
    d->val32 = (float*)c->buf.solve.val32.p;
  }
  return RDC_OK;
}

// The lists that rdc_solve.h lays out in arenas (mg_place, mg_gs_place, ilu_place, ilu_place_f32) reach the device in one way:
// place(arenas, copy) runs on arenas without a base and a copy that does nothing, which measures; b0 and b1 (may be null) are
// allocated to the measured sizes; place runs again on them with a copy that uploads and stops at the first error; the stream is
// synchronised, so the host lists may go out of scope.  what: the noun of the message.
template <class Place>
int arena_upload(rdc_ctx* c, DevBuf* b0, DevBuf* b1, const char* what, Place&& place) {
  MgArena a[2];
  DevBuf* const b[2] = {b0, b1};
  place(a, [](void*, const void*, size_t) {});
  for (int i = 0; i < 2 && b[i]; i++) {
    int rc = dev_alloc(c, *b[i], a[i].used);
    if (rc) return rc;
    a[i] = MgArena{(char*)b[i]->p};
  }
  hipError_t e = hipSuccess;
  place(a, [&](void* at, const void* list, size_t bytes) {
    if (e == hipSuccess) e = hipMemcpyAsync(at, list, bytes, hipMemcpyHostToDevice, c->stream);
  });
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, RDC_ERR_HIP, "upload of %s failed: %s", what, hipGetErrorString(e));
  return RDC_OK;
}

// A mesh holds one hierarchy: that of the single-partition solves, or that of rdc_solve_dist_mg with its ghost layers.  A call
// that needs the other kind drops it, and so does what a distributed one was built on going away (a new plan, new peers).
// A mesh also holds one set of colour lists.  Those of the single-partition hierarchy outlive it, since that hierarchy is always
// the same; those of a partitioned one (gs_dist: RDC_PRECOND_MULTIGRID_GS_LOCAL) depend on the plan as it does -- the ghost
// columns they ignore, the interior split of colour 0 -- and go whenever it goes or would go.
void mg_drop_unless(SolveState& S, bool dist) {
  if (S.mg_ready && S.mg_dist != dist) S.mg_ready = S.mg_dist = false;
  if (!dist && S.gs_ready && S.gs_dist) S.gs_ready = S.gs_dist = false;
}

// the two arenas of a hierarchy (mg_build or, with halos, the levels of mg_view_dist), carved by mg_place
int mg_upload(rdc_ctx* c, const std::vector<MgLevelHost>& steps, const std::vector<MgHalo>* halos) {
  const HostPrep& P = c->ms.prep;
  return arena_upload(c, &c->buf.solve.mg_idx, &c->buf.solve.mg_val, "the multigrid lists", [&](MgArena* a, auto&& copy) {
    mg_place(steps, P.nvar, P.n_owned, P.bptr[(size_t)P.n_owned], a[0], a[1], c->ms.solve.mg, copy, halos);
  });
}

// The colour lists of the Gauss-Seidel smoother, one per level of the hierarchy `steps` describes: coloured on the host, validated,
// and uploaded into one arena that mg_gs_place carves (first solve with "mg_smoother" = 1 on a mesh).  dist: the hierarchy is a
// partitioned one (RDC_PRECOND_MULTIGRID_GS_LOCAL): mg_colour ignores the ghost columns, so the lists are those of the owned square
// of every level, and the nodes of colour 0 below "interior_nodes" are counted for the launch inside the exchange.
int gs_upload(rdc_ctx* c, const std::vector<MgLevelHost>& steps, bool dist) {
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  std::vector<MgColours> cols(steps.size() + 1);
  for (size_t l = 0; l < cols.size(); l++) {
    const bool ok = l == 0 ? mg_colour(P.n_owned, P.bptr.data(), P.bcol.data(), cols[0])
                           : mg_colour(steps[l - 1].n, steps[l - 1].bptr.data(), steps[l - 1].bcol.data(), cols[l]);
    if (!ok)
      return fail(c, RDC_ERR_UNSUPPORTED, "the block pattern of %smultigrid level %d is not structurally symmetric: two coupled nodes share "
                  "a colour, and a Gauss-Seidel sweep (%s) over such colours would race", dist ? "this rank's owned square of " : "", (int)l,
                  dist ? "precond 6" : "\"mg_smoother\" = 1");
  }
  S.gs_cols = std::move(cols);   // MgGsLevel::cptr_host points into them
  int rc = arena_upload(c, &c->buf.solve.mg_gs, nullptr, "the colour lists", [&](MgArena* a, auto&& copy) { mg_gs_place(S.gs_cols, a[0], S.gs, copy); });
  S.gs_ready = rc == RDC_OK;
  S.gs_dist = S.gs_ready && dist;
  if (S.gs_dist) S.gs.int0 = mg_gs_interior(S.gs_cols[0], S.plan_ready ? S.dist.n_int : 0);
  return rc;
}

// The multigrid hierarchy of the mesh: built on the host and uploaded at the first multigrid solve (rdc_solve.h, mg_build).
// d must come from solve_view(want_work).
// gs_local: RDC_PRECOND_MULTIGRID_GS_LOCAL, which sweeps with Gauss-Seidel whatever "mg_smoother" says
int mg_view(rdc_ctx* c, SolveDev* d, bool gs_local) {
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  MgDev& g = S.mg;
  mg_drop_unless(S, false);
  const bool gs = gs_local || c->sopt.mg_smoother == 1;
  const bool want_gs = gs && !S.gs_ready;   // the hierarchy of a mesh is always the same: its colours outlive a rebuild
  if (!S.mg_ready || want_gs) {
    std::vector<MgLevelHost> steps;
    if (!mg_build(P.n_owned, P.bptr.data(), P.bcol.data(), steps))
      return fail(c, RDC_ERR_UNSUPPORTED, "a multigrid level would have 2^31 node blocks or more");
    int rc;
    if (want_gs && (rc = gs_upload(c, steps, false))) return rc;   // first: a refusal leaves the context as it was
    if (!S.mg_ready && (rc = mg_upload(c, steps, nullptr))) return rc;
    S.mg_ready = true;
  }
  g.lv[0].bptr = d->bptr; g.lv[0].bcol = d->bcol;
  g.omega = 1e-3 * c->sopt.mg_omega;
  d->mg = &g;
  if (gs) {
    S.gs.fuse = c->sopt.mg_gs_fuse != 0;
    d->gs = &S.gs;
  }
  return RDC_OK;
}

// The lists of the block ILU(0) of the mesh (rdc_solve.h, ilu_build: colours, rows in elimination order), built on the host and
// uploaded at the first solve with RDC_PRECOND_ILU0 or RDC_PRECOND_ILU0_LOCAL, into the two arenas ilu_place carves.  One set per
// mesh serves both values: on a context with ghost nodes -- only the callers of the rank-local factor get here with one -- the lists
// are those of the owned square and M p and M s have a ghost tail; without ghosts they are what they always were.  d must come
// from solve_view.
int ilu_view(rdc_ctx* c, SolveDev* d) {
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  int rc;
  if (!S.ilu_ready) {
    IluHost H;
    int64_t where = -1;
    const int bad = ilu_build(P.n_owned, P.bptr.data(), P.bcol.data(), H, &where, P.n_owned < P.n_node);
    if (bad == 1)
      return fail(c, RDC_ERR_UNSUPPORTED, "the block pattern is not structurally symmetric: two coupled nodes share a colour, and the "
                  "block ILU(0) (precond %d) eliminates colour by colour", (int)RDC_PRECOND_ILU0);
    if (bad) return fail(c, RDC_ERR_UNSUPPORTED, "node %lld has no diagonal block in the pattern: no block ILU(0)", (long long)where);
    S.ilu_host = std::move(H);   // IluDev::cptr_host points into it
    rc = arena_upload(c, &c->buf.solve.ilu_idx, &c->buf.solve.ilu_val, "the ILU(0) lists", [&](MgArena* a, auto&& copy) {
      ilu_place(S.ilu_host, P.nvar, P.n_owned, P.bptr[(size_t)P.n_owned], a[0], a[1], S.ilu, copy, P.n_node);
    });
    if (rc) return rc;
    S.ilu_ready = true;
  }
  S.ilu.want32 = c->sopt.ilu_factor_bits == 32;
  if (S.ilu.want32 && !S.ilu.val32) {   // the third allocation: the fp32 copy of the factor, from the first call that wants it
    const std::vector<int64_t> foff = ilu_f32_offsets(P.n_owned, P.bptr.data(), S.ilu_host, P.nvar);
    rc = arena_upload(c, &c->buf.solve.ilu_f32, nullptr, "the offsets of the fp32 ILU(0) factor", [&](MgArena* a, auto&& copy) { ilu_place_f32(foff, a[0], S.ilu, copy); });
    if (rc) { S.ilu.foff = nullptr; S.ilu.val32 = nullptr; return rc; }   // nothing half uploaded is kept
  }
  d->ilu = &S.ilu;
  return RDC_OK;
}

// The state of restarted GMRES for the option "gmres_restart" as it stands: one allocation that gmres_carve (rdc_solve.h) measures
// and then carves, made at the first call that needs it on a mesh and remade when the restart length has grown.  d must come from
// solve_view(want_work).  dist: the partitioned form, whose slots have ghost tails and which has the buffer of the wide all-reduce;
// it is a little larger than the other for the same restart length, so the bytes at hand decide as well.
int gmres_view(rdc_ctx* c, SolveDev* d, bool dist) {
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  const int m = c->sopt.gmres_restart;
  const int64_t n_nodes = dist ? P.n_node : -1;
  const size_t bytes = gmres_carve(P.nvar, P.n_owned, m, nullptr, n_nodes).bytes;
  if (m > S.gmres_cap || bytes > c->buf.solve.gmres.bytes) {
    S.gmres_cap = 0;
    int rc = dev_alloc(c, c->buf.solve.gmres, bytes);
    if (rc) return rc;   // the message gives the byte count
    S.gmres_cap = m;
  }
  if (!c->gmres_rec) RDC_HIP(c, hipHostMalloc((void**)&c->gmres_rec, sizeof(GmresRec), hipHostMallocDefault));
  S.gmres = gmres_carve(P.nvar, P.n_owned, m, (double*)c->buf.solve.gmres.p, n_nodes);
  d->gmres = &S.gmres;
  d->gmres_rec = c->gmres_rec;
  d->gmres_refine = c->sopt.gmres_refine != 0;
  return RDC_OK;
}

// what a partitioned entry adds to a call; sized: the levels below the matrix exchange (rdc_solve_dist_mg, and rdc_solve_dist_gmres
// with the multigrid; null otherwise); wide: rdc_solve_dist_gmres and its hook; rc: a callback's non-zero return
struct DistCall { const rdc_solve_comm* comm; const rdc_solve_comm_sized* sized; const rdc_solve_comm_wide* wide; int rc; };

// The hierarchy of rdc_solve_dist_mg: built collectively at the first such solve after a plan (rdc_solve.h: mg_dist_aggregate, the
// exchange of aggregate numbers, mg_dist_coarsen; mg_dist_goes_on decides on all-reduced sums) and placed by mg_place with its
// ghost layers.  The two collective calls of a step go through the communicator on a small device buffer.  d must carry the
// work buffer.  gs_local (RDC_PRECOND_MULTIGRID_GS_LOCAL): the colour lists of the levels too, from the steps the build keeps on the
// host (mg_dist_steps), at the first such solve on the hierarchy; a refusal by the colouring comes before anything is uploaded.
int mg_view_dist(rdc_ctx* c, SolveDev* d, const rdc_solve_comm_sized* comm, int* comm_rc, bool gs_local) {
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  MgDev& g = S.mg;
  mg_drop_unless(S, true);
  if (!S.mg_ready) {
    if (S.gs_dist) S.gs_ready = S.gs_dist = false;   // (of a hierarchy whose upload failed)
    if (P.bptr[(size_t)P.n_owned] >= ((int64_t)1 << 31)) return fail(c, RDC_ERR_UNSUPPORTED, "a multigrid level would have 2^31 node blocks or more");
    std::vector<MgLevelHost> steps;
    std::vector<MgHalo> halos(1, S.halo0);
    const int peers = halos[0].peers();
    // staging: [send ids | received ids | 2 sums], sized for level 0 (no level below has more to send or receive)
    const int64_t ns0 = halos[0].n_send(), ng0 = halos[0].n_ghost;
    int rc = dev_alloc(c, c->buf.solve.mg_stage, (size_t)(ns0 + ng0 + 8) * sizeof(double));
    if (rc) return rc;
    double* d_send = (double*)c->buf.solve.mg_stage.p; double* d_recv = d_send + ns0; double* d_sum = d_recv + ng0;
    std::vector<double> ids_out, ids_in;
    hipError_t e = hipSuccess;
    const int64_t* bptr = P.bptr.data();
    const int32_t* bcol = P.bcol.data();
    const char* refused = nullptr;
    for (;;) {
      const MgHalo& F = halos.back();
      MgLevelHost L;
      ids_out.assign((size_t)F.n_send() + 1, 0.0);
      mg_dist_aggregate(F, bptr, bcol, L, ids_out.data());
      double sums[2] = {(double)F.n_owned, L.n < F.n_owned ? 1.0 : 0.0};
      if ((e = hipMemcpyAsync(d_sum, sums, sizeof(sums), hipMemcpyHostToDevice, c->stream)) != hipSuccess) break;
      if ((*comm_rc = comm->base.allreduce_sum(comm->base.user, d_sum, 2, (void*)c->stream))) break;
      if ((e = hipMemcpyAsync(sums, d_sum, sizeof(sums), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) break;
      if (!mg_dist_goes_on((int)halos.size(), sums[0], sums[1])) break;
      // the owners' aggregate numbers of this rank's ghosts: one exchange of width 1
      std::vector<int64_t> so(F.send_off), go(F.ghost_off);
      ids_in.assign((size_t)F.n_ghost + 1, -1.0);
      if (F.n_send() && (e = hipMemcpyAsync(d_send, ids_out.data(), (size_t)F.n_send() * sizeof(double), hipMemcpyHostToDevice, c->stream)) != hipSuccess) break;
      if ((*comm_rc = comm->exchange_sized_begin(comm->base.user, d_send, d_recv, peers, so.data(), go.data(), (void*)c->stream))) break;
      if ((*comm_rc = comm->exchange_sized_end(comm->base.user, (void*)c->stream))) break;
      if (F.n_ghost && (e = hipMemcpyAsync(ids_in.data(), d_recv, (size_t)F.n_ghost * sizeof(double), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
      if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) break;
      MgHalo C;
      if (!mg_dist_coarsen(F, bptr, bcol, ids_in.data(), L, C)) { refused = "a multigrid level would have 2^31 node blocks or more, or a peer sent no aggregate number"; break; }
      steps.push_back(std::move(L));
      halos.push_back(std::move(C));
      bptr = steps.back().bptr.data();
      bcol = steps.back().bcol.data();
    }
    (void)hipStreamSynchronize(c->stream);
    if (*comm_rc) return fail(c, RDC_ERR_COMM, "a communication callback returned %d while the multigrid levels were built", *comm_rc);
    if (e != hipSuccess) return fail(c, RDC_ERR_HIP, "building the multigrid levels failed: %s", hipGetErrorString(e));
    if (refused) return fail(c, RDC_ERR_UNSUPPORTED, "%s", refused);
    S.mg_off.assign(halos.size(), std::vector<int64_t>());
    for (size_t l = 1; l < halos.size(); l++) {
      for (int64_t o : halos[l].send_off) S.mg_off[l].push_back(o * P.nvar);
      for (int64_t o : halos[l].ghost_off) S.mg_off[l].push_back(o * P.nvar);
    }
    if (gs_local && (rc = gs_upload(c, steps, true))) return rc;
    if ((rc = mg_upload(c, steps, &halos))) return rc;
    S.mg_dist_steps = std::move(steps);
    for (size_t l = 1; l < halos.size(); l++) {
      g.lv[l].send_off = S.mg_off[l].data();
      g.lv[l].ghost_off = S.mg_off[l].data() + peers + 1;
    }
    S.mg_ready = S.mg_dist = true;
  } else if (gs_local && !(S.gs_ready && S.gs_dist)) {
    int rc = gs_upload(c, S.mg_dist_steps, true);
    if (rc) return rc;
  }
  g.lv[0].bptr = d->bptr; g.lv[0].bcol = d->bcol;
  g.omega = 1e-3 * c->sopt.mg_omega;
  d->mg = &g;
  if (gs_local) {
    S.gs.fuse = c->sopt.mg_gs_fuse != 0;
    d->gs = &S.gs;
  }
  d->peers = S.halo0.peers();
  return RDC_OK;
}

// The first lines of every entry that runs or plans a solve: the context, its mesh, and what entering invalidates.
int solve_enter(rdc_ctx* c, SolveEntry entry) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  solve_valid_enter(c->ms.solve.valid, entry);
  return RDC_OK;
}

// Behind the last refusal of an entry.  What the call is about to rebuild stops being valid; the one SolveDev of the call is filled,
// always in this order -- the work buffer and record (those of a partitioned solve if dist), the fp32 copy if the call is mixed, the
// hierarchy, the ILU(0) lists, the state of GMRES; run(d) does the device work and notes in *o what it found; the flags follow
// from the outcome.  *precond: RDC_PRECOND_ILU0_LOCAL becomes RDC_PRECOND_ILU0 on a context without ghost nodes, where the owned
// square is the matrix; RDC_PRECOND_MULTIGRID_GS_LOCAL becomes RDC_PRECOND_MULTIGRID once the view carries the colour lists, which
// are what tells rdc_solve.hip the smoother.
template <class Run>
int solve_do(rdc_ctx* c, const SolveCall& call, int32_t* precond, DistCall* dist, SolveOutcome* o, Run&& run) {
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  solve_valid_begin(S.valid, call);
  SolveDev d;
  if (dist) {
    d.dist = S.plan_ready ? S.dist : DistDims{P.n_node, 0, 0};
    d.send_nodes = (const int32_t*)c->buf.solve.send.p;
    d.comm = dist->comm; d.sized = dist->sized; d.wide = dist->wide; d.comm_rc = &dist->rc;
  }
  int rc = solve_view(c, true, call.mixed, &d, dist ? &d.dist : nullptr);
  if (rc) return rc;
  const bool gs_local = call.precond == RDC_PRECOND_MULTIGRID_GS_LOCAL;
  if (call.multigrid() && (rc = dist ? mg_view_dist(c, &d, dist->sized, &dist->rc, gs_local) : mg_view(c, &d, gs_local))) return rc;
  if (precond && gs_local) *precond = RDC_PRECOND_MULTIGRID;
  if (precond && *precond == RDC_PRECOND_ILU0_LOCAL && P.n_owned == P.n_node) *precond = RDC_PRECOND_ILU0;
  if (call.ilu() && (rc = ilu_view(c, &d))) return rc;
  if (call.gmres && (rc = gmres_view(c, &d, dist != nullptr))) return rc;
  const hipError_t e = run(d);
  o->ran = e == hipSuccess;
  o->comm_failed = dist && dist->rc;
  solve_valid_leave(S.valid, call, *o);
  if (o->comm_failed) {
    (void)hipStreamSynchronize(c->stream);   // x holds the last iterate
    return fail(c, RDC_ERR_COMM, "a communication callback returned %d; the solve was abandoned", dist->rc);
  }
  RDC_HIP(c, e);
  return RDC_OK;
}

// y = A x on the FP64 values or, f32, on the fp32 copy of D^-1 A that the last rdc_csr_scale_f32 or mixed call left
int matvec_call(rdc_ctx* c, const double* d_x, double* d_y, bool f32) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (!d_x || !d_y) return fail(c, RDC_ERR_INVALID, "null vector");
  if (f32 && !c->ms.solve.valid.f32_copy) return fail(c, RDC_ERR_INVALID, "this mesh has no fp32 copy: call rdc_csr_scale_f32 or rdc_solve_mixed first");
  if (c->ms.prep.n_owned == 0) return RDC_OK;   // no rows
  SolveDev d;
  int rc = solve_view(c, false, f32, &d);
  if (rc) return rc;
  if (f32) RDC_HIP(c, solve_matvec_f32(d, d_x, d_y));
  else RDC_HIP(c, solve_matvec(d, d_x, d_y));
  return RDC_OK;
}

// with_right: the preconditioners applied from the right on top of block Jacobi's system count (the solve entries)
bool known_precond(int precond, bool with_right) {
  return precond == RDC_PRECOND_NONE || precond == RDC_PRECOND_JACOBI || precond == RDC_PRECOND_BLOCK_JACOBI ||
         (with_right && (precond == RDC_PRECOND_MULTIGRID || precond == RDC_PRECOND_ILU0 || precond == RDC_PRECOND_ILU0_LOCAL ||
                        precond == RDC_PRECOND_MULTIGRID_GS_LOCAL));
}

// what every entry that takes rdc_solve_params refuses of them
int check_solve_params(rdc_ctx* c, const rdc_solve_params* p) {
  if (p->max_its < 1) return fail(c, RDC_ERR_INVALID, "max_its must be at least 1");
  if (!(p->rel_tol >= 0.0) || !(p->abs_tol >= 0.0) || !std::isfinite(p->rel_tol) || !std::isfinite(p->abs_tol))
    return fail(c, RDC_ERR_INVALID, "tolerances must be finite and not negative");
  if (!std::isfinite(p->rhs_scale)) return fail(c, RDC_ERR_INVALID, "rhs_scale must be finite");
  if (!known_precond(p->precond, true)) return fail(c, RDC_ERR_INVALID, "unknown preconditioner %d", (int)p->precond);
  return RDC_OK;
}

// the single-partition entries on a context with ghost nodes (multigrid: the cycle is asked for)
int refuse_ghosted(rdc_ctx* c, bool multigrid) {
  if (multigrid && c->sopt.mg_smoother == 1)
    return fail(c, RDC_ERR_UNSUPPORTED, "the context has ghost nodes (%lld owned of %lld): a Gauss-Seidel sweep (\"mg_smoother\" = 1) across "
                "partitions needs a rule for the ghost values and is not implemented", (long long)c->ms.prep.n_owned, (long long)c->ms.prep.n_node);
  return fail(c, RDC_ERR_UNSUPPORTED, "the context has ghost nodes (%lld owned of %lld): a solve across partitions needs a halo "
              "exchange inside every iteration and is not implemented; rdc_csr_matvec works on such a context",
              (long long)c->ms.prep.n_owned, (long long)c->ms.prep.n_node);
}

// behind the refusals of the four solve entries: solve_run under the protocol
int solve_run_call(rdc_ctx* c, const SolveCall& call, const rdc_solve_params* p, double* d_x, rdc_solve_info* info, DistCall* dist) {
  rdc_solve_params q = *p;
  SolveOutcome o;
  return solve_do(c, call, &q.precond, dist, &o, [&](const SolveDev& d) {
    const hipError_t e = solve_run(d, q, d_x, info, call.mixed);
    o.matrix_bits = info->matrix_bits; o.reason = info->reason;
    if (d.gmres) { o.gmres_restart = d.gmres->restart; o.gmres_cycles = d.gmres->cycles; }
    return e;
  });
}

int solve_call(rdc_ctx* c, const rdc_solve_params* p, double* d_x, rdc_solve_info* info, bool mixed) {
  int rc = solve_enter(c, SolveEntry::SOLVE);
  if (rc) return rc;
  if (!p || !d_x || !info) return fail(c, RDC_ERR_INVALID, "null argument");
  if ((rc = check_solve_params(c, p))) return rc;
  if (mixed && p->precond == RDC_PRECOND_ILU0 && c->sopt.ilu_factor_bits != 32)
    return fail(c, RDC_ERR_UNSUPPORTED, "the block ILU(0) preconditioner (precond %d) has an FP64 factor only: rdc_solve, not rdc_solve_mixed", (int)RDC_PRECOND_ILU0);
  if (mixed && p->precond == RDC_PRECOND_ILU0_LOCAL && c->sopt.ilu_factor_bits != 32)
    return fail(c, RDC_ERR_UNSUPPORTED, "the rank-local block ILU(0) preconditioner (precond %d) has an FP64 factor only: rdc_solve or rdc_solve_dist, "
                "not rdc_solve_mixed", (int)RDC_PRECOND_ILU0_LOCAL);
  if (c->ms.prep.n_owned < c->ms.prep.n_node) return refuse_ghosted(c, p->precond == RDC_PRECOND_MULTIGRID);
  if (c->ms.prep.n_owned == 0) {   // no rows, no unknowns: nothing to launch
    *info = rdc_solve_info();
    info->matrix_bits = 64;
    return RDC_OK;
  }
  return solve_run_call(c, SolveCall{SolveEntry::SOLVE, p->precond, mixed, c->sopt.solve_method == 1}, p, d_x, info, nullptr);
}

// The hooks of one application of a right preconditioner: rdc_solve_mg_apply (entry MG_APPLY), rdc_solve_ilu_apply and, local,
// rdc_solve_ilu_local_apply, which takes a context with ghost nodes (the factor of its owned square).
int apply_call(rdc_ctx* c, SolveEntry entry, bool mixed, const double* d_in, double* d_out, bool local) {
  const bool mg = entry == SolveEntry::MG_APPLY;
  int rc = solve_enter(c, entry);
  if (rc) return rc;
  if (!d_in || !d_out) return fail(c, RDC_ERR_INVALID, "null vector");
  if (!local && c->ms.prep.n_owned < c->ms.prep.n_node) return refuse_ghosted(c, mg);
  if (c->ms.prep.n_owned == 0) return RDC_OK;   // no rows
  SolveOutcome o;
  rc = solve_do(c, SolveCall{entry, RDC_PRECOND_NONE, mixed}, nullptr, nullptr, &o, [&](const SolveDev& d) {
    return mg ? solve_mg_apply(d, mixed, d_in, d_out, &o.bad_blocks, &o.matrix_bits) : solve_ilu_apply(d, d_in, d_out, &o.bad_blocks);
  });
  if (rc || o.bad_blocks == 0) return rc;
  return mg ? fail(c, RDC_ERR_INVALID, "%d diagonal blocks of the multigrid levels are not invertible: no cycle was applied", o.bad_blocks)
            : fail(c, RDC_ERR_INVALID, "%d diagonal blocks or ILU(0) pivots are not invertible: nothing was applied", o.bad_blocks);
}

// the two downloads.  Both write a node-block CSR over the columns the factor has: private position p of a node goes to the block of the
// same column in the CSR row (bcol ascends, and the owned columns of a row are its leading ones), rows of own = the node's owned
// blocks, nodes one behind the other.  Without ghosts own is the whole row, and this is the layout of the CSR values.
int ilu_download_call(rdc_ctx* c, double* val, double* uinv, bool local) {
  if (!c) return RDC_ERR_INVALID;
  const SolveState& S = c->ms.solve;
  if (!c->ms.have_mesh || !S.ilu_ready || !S.valid.ilu_factored)
    return fail(c, RDC_ERR_STATE, "no rdc_solve_ilu_apply or solve with the block ILU(0) preconditioner has run on this mesh");
  const HostPrep& P = c->ms.prep;
  if (!local && P.n_owned < P.n_node) return refuse_ghosted(c, false);
  int rc = set_device(c);
  if (rc) return rc;
  const int nv = P.nvar;
  const int64_t n = P.n_owned, blocks = P.bptr[(size_t)n];
  std::vector<double> priv(val ? (size_t)blocks * nv * nv : 0);
  if (val && blocks) RDC_HIP(c, hipMemcpyAsync(priv.data(), S.ilu.val, priv.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (uinv && n) RDC_HIP(c, hipMemcpyAsync(uinv, S.ilu.uinv, (size_t)n * nv * nv * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  if (val) {
    int64_t o0 = 0;   // owned blocks of the nodes before i
    for (int64_t i = 0; i < n; i++) {
      const int64_t b0 = P.bptr[(size_t)i], nl = S.ilu_host.nlow[(size_t)i];
      const int64_t own = S.ilu_host.nown.empty() ? P.bptr[(size_t)i + 1] - b0 : S.ilu_host.nown[(size_t)i];
      for (int64_t p = 0; p < own; p++) {
        const int64_t k = std::lower_bound(P.bcol.begin() + b0, P.bcol.begin() + b0 + own, S.ilu_host.pcol[(size_t)(b0 + p)]) - (P.bcol.begin() + b0);
        for (int a = 0; a < nv; a++)
          for (int b = 0; b < nv; b++)
            val[(int64_t)nv * nv * o0 + ((int64_t)a * own + k) * nv + b] = priv[(size_t)ilu_value_offset(b0, nv, own, nl, a, p, b)];
      }
      o0 += own;
    }
  }
  return RDC_OK;
}

// What every partitioned entry refuses of a preconditioner and of the state of the context, behind its own argument checks.
// sized: the call exchanges on the levels below the matrix (it runs the multigrid); mg_entry: it is rdc_solve_dist_mg, which runs
// nothing else; any_precond: the entry takes the multigrid beside the others (rdc_solve_dist_gmres).  A context without ghosts and
// without peer counts gets the halo of no peers.
int dist_ready(rdc_ctx* c, int precond, bool sized, bool mg_entry, bool any_precond, int mixed) {
  if (precond == RDC_PRECOND_ILU0)
    return fail(c, RDC_ERR_UNSUPPORTED, "the block ILU(0) preconditioner (precond %d) across partitions needs a ghost exchange per colour and is "
                "not implemented: rdc_solve on a context without ghost nodes, or the rank-local factor (precond %d)", (int)RDC_PRECOND_ILU0,
                (int)RDC_PRECOND_ILU0_LOCAL);
  const bool mg = precond == RDC_PRECOND_MULTIGRID || precond == RDC_PRECOND_MULTIGRID_GS_LOCAL;
  if (!any_precond && mg_entry && !mg)
    return fail(c, RDC_ERR_INVALID, "rdc_solve_dist_mg is the multigrid solve (precond %d or %d); rdc_solve_dist has the others, not %d",
                (int)RDC_PRECOND_MULTIGRID, (int)RDC_PRECOND_MULTIGRID_GS_LOCAL, precond);
  if (!any_precond && !mg_entry && mg)
    return fail(c, RDC_ERR_UNSUPPORTED, "the multigrid preconditioner across partitions exchanges on every level: rdc_solve_dist_mg");
  if (precond == RDC_PRECOND_ILU0_LOCAL && mixed && c->sopt.ilu_factor_bits != 32)
    return fail(c, RDC_ERR_UNSUPPORTED, "the rank-local block ILU(0) preconditioner (precond %d) has an FP64 factor only: rdc_solve_dist with mixed = 0",
                (int)RDC_PRECOND_ILU0_LOCAL);
  if (sized && precond == RDC_PRECOND_MULTIGRID && c->sopt.mg_smoother == 1)   // (precond 6 has its rule and does not consult the option)
    return fail(c, RDC_ERR_UNSUPPORTED, "rdc_solve_dist_mg smooths with damped Jacobi only: a Gauss-Seidel sweep (\"mg_smoother\" = 1) across "
                "partitions needs a rule for the ghost values and is not implemented");
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  if (P.n_owned < P.n_node && !S.plan_ready)
    return fail(c, RDC_ERR_STATE, "the context has ghost nodes (%lld owned of %lld) and no send list: call rdc_solve_dist_plan first",
                (long long)P.n_owned, (long long)P.n_node);
  if (sized && P.n_owned < P.n_node && !S.peers_ready)
    return fail(c, RDC_ERR_STATE, "the context has ghost nodes (%lld owned of %lld) and no peer counts: call rdc_solve_dist_plan_peers first",
                (long long)P.n_owned, (long long)P.n_node);
  if (sized && !S.peers_ready && S.halo0.send_off.empty()) {   // no ghosts and no peer counts: no peers
    mg_drop_unless(S, false);
    S.halo0 = MgHalo();
    S.halo0.n_owned = P.n_owned; S.halo0.send_off.assign(1, 0); S.halo0.ghost_off.assign(1, 0);
    mg_halo_slots(S.halo0);
  }
  return RDC_OK;
}

// the callbacks a partitioned call will use: the three of the base, the sized pair if it exchanges below the matrix, the wide all-reduce
bool comm_complete(const rdc_solve_comm* comm, const rdc_solve_comm_sized* sized, const rdc_solve_comm_wide* wide) {
  return comm->exchange_begin && comm->exchange_end && comm->allreduce_sum && (!sized || (sized->exchange_sized_begin && sized->exchange_sized_end)) &&
         (!wide || wide->allreduce_sum_wide);
}

// the three partitioned solves.  sized: rdc_solve_dist_mg, the multigrid preconditioner and nothing else; wide: rdc_solve_dist_gmres,
// GMRES whatever "solve_method" says, with every preconditioner of the other two; neither: rdc_solve_dist
int solve_dist_call(rdc_ctx* c, const rdc_solve_params* p, const rdc_solve_comm* comm, const rdc_solve_comm_sized* sized,
                    const rdc_solve_comm_wide* wide, int mixed, double* d_x, rdc_solve_info* info) {
  int rc = solve_enter(c, SolveEntry::DIST);   // the work buffer takes the layout of a partitioned solve
  if (rc) return rc;
  if (!p || !d_x || !info || !comm) return fail(c, RDC_ERR_INVALID, "null argument");
  if (!wide && c->sopt.solve_method == 1)
    return fail(c, RDC_ERR_UNSUPPORTED, "GMRES across partitions is not implemented (\"solve_method\" = 1): allreduce_sum carries at most %d doubles "
                "and a GMRES step sums up to \"gmres_restart\" + 1; set \"solve_method\" to 0 for %s", DIST_RECORD, sized ? "rdc_solve_dist_mg" : "rdc_solve_dist");
  const bool mg_entry = sized != nullptr;
  if (wide) sized = p->precond == RDC_PRECOND_MULTIGRID || p->precond == RDC_PRECOND_MULTIGRID_GS_LOCAL ? &wide->sized : nullptr;
  if (!comm_complete(comm, sized, wide)) return fail(c, RDC_ERR_INVALID, "the communicator lacks a callback");
  if ((rc = check_solve_params(c, p))) return rc;
  if ((rc = dist_ready(c, p->precond, sized != nullptr, mg_entry, wide != nullptr, mixed))) return rc;
  DistCall dc{comm, sized, wide, 0};
  return solve_run_call(c, SolveCall{SolveEntry::DIST, p->precond, mixed != 0, wide != nullptr}, p, d_x, info, &dc);
}

}  // namespace

extern "C" {

int rdc_solve_gmres_stats(rdc_ctx* c, int32_t* restart, int64_t* basis_bytes, int32_t* cycles) {
  if (!c) return RDC_ERR_INVALID;
  const SolveValid& valid = c->ms.solve.valid;
  if (!c->ms.have_mesh || !valid.gmres_solved) return fail(c, RDC_ERR_STATE, "no GMRES solve (\"solve_method\" = 1) has run on this mesh");
  if (restart) *restart = valid.gmres_restart;
  if (basis_bytes)   // (gmres_carve: a partitioned solve's slots have ghost tails)
    *basis_bytes = (int64_t)(valid.gmres_restart + 1) * (valid.gmres_dist ? c->ms.prep.n_node : c->ms.prep.n_owned) * c->ms.prep.nvar * (int64_t)sizeof(double);
  if (cycles) *cycles = valid.gmres_cycles;
  return RDC_OK;
}

int rdc_solve_ilu_stats(rdc_ctx* c, float* setup_ms, int64_t* bytes, int32_t* n_colours) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh || !c->ms.solve.ilu_ready) return fail(c, RDC_ERR_STATE, "no solve with the block ILU(0) preconditioner has run on this mesh");
  if (setup_ms) *setup_ms = c->ms.solve.ilu.setup_ms;
  if (bytes) *bytes = (int64_t)(c->buf.solve.ilu_idx.bytes + c->buf.solve.ilu_val.bytes + c->buf.solve.ilu_f32.bytes);
  if (n_colours) *n_colours = c->ms.solve.ilu.n_colours;
  return RDC_OK;
}

int rdc_solve_ilu_factor_bits(rdc_ctx* c, int32_t* bits) {
  if (!c || !bits) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh || !c->ms.solve.ilu_ready || !c->ms.solve.ilu.bits)
    return fail(c, RDC_ERR_STATE, "no solve or apply hook with the block ILU(0) preconditioner has run on this mesh");
  *bits = c->ms.solve.ilu.bits;
  return RDC_OK;
}

int rdc_solve_mg_levels(rdc_ctx* c, int32_t* n_levels, int64_t* nodes, int64_t* blocks, int cap) {
  if (!c || !n_levels || cap < 0 || (cap > 0 && (!nodes || !blocks))) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh || !c->ms.solve.mg_ready) return fail(c, RDC_ERR_STATE, "no multigrid solve has run on this mesh");
  *n_levels = c->ms.solve.mg.n_levels;
  for (int l = 0; l < c->ms.solve.mg.n_levels && l < cap; l++) { nodes[l] = c->ms.solve.mg.lv[l].n; blocks[l] = c->ms.solve.mg.lv[l].blocks; }
  return RDC_OK;
}

int rdc_solve_mg_stats(rdc_ctx* c, float* setup_ms, int64_t* level_bytes) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh || !c->ms.solve.mg_ready) return fail(c, RDC_ERR_STATE, "no multigrid solve has run on this mesh");
  if (setup_ms) *setup_ms = c->ms.solve.mg.setup_ms;
  if (level_bytes) *level_bytes = (int64_t)(c->buf.solve.mg_idx.bytes + c->buf.solve.mg_val.bytes);
  return RDC_OK;
}

int rdc_solve_mg_colours(rdc_ctx* c, int32_t* n_colours, int cap) {
  if (!c || cap < 0 || (cap > 0 && !n_colours)) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh || !c->ms.solve.gs_ready) return fail(c, RDC_ERR_STATE, "no multigrid solve with the Gauss-Seidel smoother has run on this mesh");
  for (int l = 0; l < c->ms.solve.gs.n_levels && l < cap; l++) n_colours[l] = c->ms.solve.gs.lv[l].n_colours;
  return RDC_OK;
}

int rdc_csr_scale_f32(rdc_ctx* c, int precond) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (!known_precond(precond, false)) return fail(c, RDC_ERR_INVALID, "unknown preconditioner %d", precond);
  solve_valid_enter(c->ms.solve.valid, SolveEntry::SCALE_F32);   // D^-1 in the work buffer is rebuilt, for `precond`
  int overflow = 0;
  SolveOutcome o;
  int rc = solve_do(c, SolveCall{SolveEntry::SCALE_F32, precond, true}, nullptr, nullptr, &o, [&](const SolveDev& d) {
    const hipError_t e = c->ms.prep.n_owned > 0 ? solve_scale_f32(d, precond, &o.bad_blocks, &overflow) : hipSuccess;
    o.matrix_bits = overflow > 0 ? 64 : 32;
    return e;
  });
  if (rc) return rc;
  if (o.bad_blocks > 0) return fail(c, RDC_ERR_INVALID, "%d diagonal blocks are not invertible: no fp32 copy", o.bad_blocks);
  if (overflow > 0) return fail(c, RDC_ERR_INVALID, "%d blocks of D^-1 A hold an entry that is not finite in fp32: no fp32 copy", overflow);
  return RDC_OK;
}

int rdc_csr_matvec(rdc_ctx* c, const double* d_x, double* d_y) { return matvec_call(c, d_x, d_y, false); }
int rdc_csr_matvec_f32(rdc_ctx* c, const double* d_x, double* d_y) { return matvec_call(c, d_x, d_y, true); }

int rdc_solve(rdc_ctx* c, const rdc_solve_params* p, double* d_x, rdc_solve_info* info) { return solve_call(c, p, d_x, info, false); }
int rdc_solve_mixed(rdc_ctx* c, const rdc_solve_params* p, double* d_x, rdc_solve_info* info) { return solve_call(c, p, d_x, info, true); }

int rdc_solve_gmres_arnoldi(rdc_ctx* c, int precond, int mixed, const double* d_v0, int steps, double* d_V, double* H, int32_t* steps_done) {
  int rc = solve_enter(c, SolveEntry::ARNOLDI);   // D^-1 in the work buffer is rebuilt
  if (rc) return rc;
  if (!d_v0 || !d_V || !H || !steps_done) return fail(c, RDC_ERR_INVALID, "null argument");
  if (!known_precond(precond, true)) return fail(c, RDC_ERR_INVALID, "unknown preconditioner %d", precond);
  if (steps < 1 || steps > c->sopt.gmres_restart)
    return fail(c, RDC_ERR_INVALID, "steps must be 1 .. \"gmres_restart\" = %d, not %d", c->sopt.gmres_restart, steps);
  if (mixed && (precond == RDC_PRECOND_ILU0 || precond == RDC_PRECOND_ILU0_LOCAL) && c->sopt.ilu_factor_bits != 32)
    return fail(c, RDC_ERR_UNSUPPORTED, "the block ILU(0) preconditioner (precond %d) has an FP64 factor only: mixed = 0, or \"ilu_factor_bits\" = 32", precond);
  if (c->ms.prep.n_owned < c->ms.prep.n_node) return refuse_ghosted(c, precond == RDC_PRECOND_MULTIGRID);
  *steps_done = 0;
  if (c->ms.prep.n_owned == 0) return RDC_OK;   // no rows
  int done = 0;
  SolveOutcome o;
  rc = solve_do(c, SolveCall{SolveEntry::ARNOLDI, precond, mixed != 0, true}, &precond, nullptr, &o, [&](const SolveDev& d) {
    return solve_gmres_arnoldi(d, precond, mixed != 0, d_v0, steps, d_V, H, &done, &o.bad_blocks, &o.matrix_bits);
  });
  if (rc) return rc;
  if (o.bad_blocks > 0) return fail(c, RDC_ERR_INVALID, "%d diagonal blocks or pivots are not invertible: nothing was run", o.bad_blocks);
  *steps_done = done;
  return RDC_OK;
}

int rdc_solve_mg_apply(rdc_ctx* c, int mixed, const double* d_in, double* d_out) { return apply_call(c, SolveEntry::MG_APPLY, mixed != 0, d_in, d_out, false); }
int rdc_solve_ilu_apply(rdc_ctx* c, const double* d_in, double* d_out) { return apply_call(c, SolveEntry::ILU_APPLY, false, d_in, d_out, false); }
int rdc_solve_ilu_local_apply(rdc_ctx* c, const double* d_in, double* d_out) { return apply_call(c, SolveEntry::ILU_APPLY, false, d_in, d_out, true); }

int rdc_solve_ilu_download(rdc_ctx* c, double* val, double* uinv) { return ilu_download_call(c, val, uinv, false); }
int rdc_solve_ilu_local_download(rdc_ctx* c, double* val, double* uinv) { return ilu_download_call(c, val, uinv, true); }

int rdc_solve_mg_level_download(rdc_ctx* c, int level, double* val, double* dinv) {
  if (!c) return RDC_ERR_INVALID;
  const SolveState& S = c->ms.solve;
  if (!c->ms.have_mesh || !S.mg_ready || !S.valid.mg_values)
    return fail(c, RDC_ERR_STATE, "no rdc_solve_mg_apply or multigrid solve has run on this mesh, or a later call has overwritten what it built");
  if (level < 0 || level >= S.mg.n_levels) return fail(c, RDC_ERR_INVALID, "level %d: the hierarchy has the levels 0 .. %d", level, S.mg.n_levels - 1);
  if (level == 0 && val) return fail(c, RDC_ERR_INVALID, "level 0 is the matrix itself (rdc_csr_download): val must be NULL");
  int rc = set_device(c);
  if (rc) return rc;
  const MgLevelDev& L = S.mg.lv[level];
  const size_t nv2 = (size_t)c->ms.prep.nvar * c->ms.prep.nvar;
  const double* d_dinv = L.dinv;
  if (level == 0) {
    SolveDev d;
    if ((rc = solve_view(c, true, false, &d))) return rc;
    d_dinv = solve_dinv(d);
  }
  if (val && L.blocks) RDC_HIP(c, hipMemcpyAsync(val, L.val, (size_t)L.blocks * nv2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (dinv && L.n) RDC_HIP(c, hipMemcpyAsync(dinv, d_dinv, (size_t)L.n * nv2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  return RDC_OK;
}

int rdc_solve_dist_plan(rdc_ctx* c, int64_t n_send, const int32_t* send_nodes) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (n_send < 0 || (n_send > 0 && !send_nodes)) return fail(c, RDC_ERR_INVALID, "bad send list");
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  S.plan_ready = S.peers_ready = false;
  solve_valid_enter(S.valid, SolveEntry::DIST_PLAN);
  mg_drop_unless(S, false);   // a new plan drops the hierarchy built on the old one
  S.halo0 = MgHalo();
  const int64_t n_int = c->opt.interior_nodes > 0 ? c->opt.interior_nodes : 0;
  int64_t where = 0;
  switch (dist_plan_check(P.n_owned, P.bptr.data(), P.bcol.data(), n_int, n_send, send_nodes, &where)) {
    case 1: return fail(c, RDC_ERR_INVALID, "send entry %lld is node %d, which is not one of the %lld owned nodes", (long long)where,
                        (int)send_nodes[where], (long long)P.n_owned);
    case 2: return fail(c, RDC_ERR_INVALID, "\"interior_nodes\" = %lld exceeds the %lld owned nodes", (long long)n_int, (long long)P.n_owned);
    case 3: return fail(c, RDC_ERR_INVALID, "node %lld lies below \"interior_nodes\" = %lld but its row has a ghost column", (long long)where, (long long)n_int);
    default: break;
  }
  int rc = set_device(c);
  if (rc) return rc;
  S.send_nodes.assign(send_nodes, send_nodes + n_send);
  if ((rc = dev_upload(c, c->buf.solve.send, S.send_nodes))) return rc;
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  S.dist.n_nodes = P.n_node; S.dist.n_int = n_int; S.dist.n_send = n_send;
  S.plan_ready = true;
  return RDC_OK;
}

int rdc_solve_dist_plan_peers(rdc_ctx* c, int32_t n_peers, const int64_t* send_count, const int64_t* ghost_count) {
  int rc = solve_enter(c, SolveEntry::DIST_PLAN);
  if (rc) return rc;
  const HostPrep& P = c->ms.prep;
  SolveState& S = c->ms.solve;
  if (!S.plan_ready) return fail(c, RDC_ERR_STATE, "no send list: call rdc_solve_dist_plan first");
  if (n_peers < 0 || (n_peers > 0 && (!send_count || !ghost_count))) return fail(c, RDC_ERR_INVALID, "bad peer counts");
  MgHalo plan;
  switch (mg_halo_plan(P.n_owned, P.n_node - P.n_owned, S.dist.n_send, S.send_nodes.data(), n_peers, send_count, ghost_count, plan)) {
    case 0: break;
    case 1: return fail(c, RDC_ERR_INVALID, "a peer count is negative");
    case 2: return fail(c, RDC_ERR_INVALID, "the send counts of the %d peers do not add up to the %lld entries of the send list", (int)n_peers, (long long)S.dist.n_send);
    case 3: return fail(c, RDC_ERR_INVALID, "the ghost counts of the %d peers do not add up to the %lld ghost nodes", (int)n_peers, (long long)(P.n_node - P.n_owned));
    default: return fail(c, RDC_ERR_INVALID, "bad send list");
  }
  mg_drop_unless(S, false);   // new peers drop the hierarchy built on the old ones
  S.halo0 = std::move(plan);
  S.peers_ready = true;
  return RDC_OK;
}

int rdc_solve_dist(rdc_ctx* c, const rdc_solve_params* p, const rdc_solve_comm* comm, int mixed, double* d_x, rdc_solve_info* info) { return solve_dist_call(c, p, comm, nullptr, nullptr, mixed, d_x, info); }
int rdc_solve_dist_mg(rdc_ctx* c, const rdc_solve_params* p, const rdc_solve_comm_sized* comm, int mixed, double* d_x, rdc_solve_info* info) { return solve_dist_call(c, p, comm ? &comm->base : nullptr, comm, nullptr, mixed, d_x, info); }
int rdc_solve_dist_gmres(rdc_ctx* c, const rdc_solve_params* p, const rdc_solve_comm_wide* comm, int mixed, double* d_x, rdc_solve_info* info) { return solve_dist_call(c, p, comm ? &comm->sized.base : nullptr, nullptr, comm, mixed, d_x, info); }

int rdc_solve_dist_gmres_arnoldi(rdc_ctx* c, const rdc_solve_comm_wide* comm, int precond, int mixed, const double* d_v0, int steps, double* d_V,
                                 double* H, int32_t* steps_done) {
  int rc = solve_enter(c, SolveEntry::ARNOLDI);   // D^-1 in the work buffer is rebuilt, and the buffer takes the layout of a partitioned solve
  if (rc) return rc;
  if (!comm || !d_v0 || !d_V || !H || !steps_done) return fail(c, RDC_ERR_INVALID, "null argument");
  const rdc_solve_comm_sized* sized = precond == RDC_PRECOND_MULTIGRID || precond == RDC_PRECOND_MULTIGRID_GS_LOCAL ? &comm->sized : nullptr;
  if (!comm_complete(&comm->sized.base, sized, comm)) return fail(c, RDC_ERR_INVALID, "the communicator lacks a callback");
  if (!known_precond(precond, true)) return fail(c, RDC_ERR_INVALID, "unknown preconditioner %d", precond);
  if (steps < 1 || steps > c->sopt.gmres_restart)
    return fail(c, RDC_ERR_INVALID, "steps must be 1 .. \"gmres_restart\" = %d, not %d", c->sopt.gmres_restart, steps);
  if ((rc = dist_ready(c, precond, sized != nullptr, false, true, mixed))) return rc;
  *steps_done = 0;
  int done = 0;
  SolveOutcome o;
  DistCall dc{&comm->sized.base, sized, comm, 0};
  SolveCall call{SolveEntry::ARNOLDI, precond, mixed != 0, true};
  call.dist = true;
  rc = solve_do(c, call, &precond, &dc, &o, [&](const SolveDev& d) {
    return solve_gmres_arnoldi(d, precond, mixed != 0, d_v0, steps, d_V, H, &done, &o.bad_blocks, &o.matrix_bits);
  });
  if (rc) return rc;
  if (o.bad_blocks > 0) return fail(c, RDC_ERR_INVALID, "%d diagonal blocks or pivots are not invertible: nothing was run", o.bad_blocks);
  *steps_done = done;
  return RDC_OK;
}

}  // extern "C"
