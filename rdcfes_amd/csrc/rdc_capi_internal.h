// rdc_capi_internal.h — the context behind the C-ABI and its device-memory helpers: what rdc_capi.hip (context, mesh, fields,
// assembly, post-processing, timing) and rdc_capi_solve.hip (the linear solve) share.  The helpers are defined in rdc_capi.hip.
#ifndef RDC_CAPI_INTERNAL_H
#define RDC_CAPI_INTERNAL_H

#include <vector>

#include "rdc_internal.h"
#include "rdc_const_rows.h"
#include "rdc_parts.h"
#include "rdc_newton.h"
#include "rdc_solve.h"
#include "rdc_solve_state.h"

namespace rdc {

static_assert(SOLVE_OPT_MG_OMEGA == MG_OMEGA_PERMILLE && SOLVE_OPT_GMRES_RESTART == GMRES_DEFAULT_RESTART &&
              SOLVE_OPT_GMRES_MAX_RESTART == GMRES_MAX_RESTART, "the literals of RDC_SOLVE_OPTIONS (rdc_options.h) follow rdc_solve.h");

struct DevBuf { void* p = nullptr; size_t bytes = 0; bool owned = true; };   // owned = false: bound by the caller (rdc_field_bind_device)

// Device buffers, in groups that follow the device views (MeshDev, Rg2Dev, EvDev, ClDev ...).  A group holds DevBufs and
// nothing else, so it can be walked as an array (free_group): a new buffer is one more name in its group.
struct Buffers {
  struct { DevBuf conn, xyz, bptr, eslot, elem_order, first_mask, first_rhs, pair_elem, pair_local, node_pair_ptr, wg_node_ptr; } mesh;
  // TET4 pair lists; nlist and ploc are read by k_tet4_rg5 only, eid (pair -> element) is uploaded at the first assembly of a model with per-element inputs
  struct { DevBuf desc, pair, chunk, sdesc, contrib, aux, ntab, nlist, ploc, eid; } rg2;
  struct { DevBuf nl_ptr, nlist, ploc; } hx;   // node-staged generic row gather (HEX8)
  // element-visit lists; perm = workgroup order of the two-part assembly, ticket = cluster counters of the resident kernel
  struct { DevBuf desc, nlist, vloc, vslot, ntab, bpart, perm, ticket; } ev;
  struct { DevBuf desc, ntab, eid, pair, pslot; } cl;        // cluster lists of the producer / consumer HEX8 kernels
  struct { DevBuf ke, fe, gptr, gsrc, brow; } two_pass;      // solid two-pass assembly: element matrices + gather lists
  struct { DevBuf elem_material, materials, side_elem, side_id, side_disp; } solid_in;
  // linear solve (rdc_solve.hip): block column list (first matvec / solve), work vectors (first solve); fp32 copy of D^-1 A
  // and the offsets of its padded rows (first mixed solve / rdc_csr_scale_f32)
  // mg_idx / mg_val: every list, and every matrix / D_l^-1 / vector, of the multigrid levels (first multigrid solve)
  // send: the send list of a partitioned solve (rdc_solve_dist_plan)
  // mg_gs: the colour lists of every level (first multigrid solve with the Gauss-Seidel smoother)
  // ilu_f32: the offsets and the floats of the fp32 copy of that factor (first ILU solve or hook with "ilu_factor_bits" = 32; ilu_place_f32)
  // ilu_idx / ilu_val: the lists, and the factor / U_ii^-1 / vectors, of the block ILU(0) (first solve with RDC_PRECOND_ILU0; rdc_solve.h, ilu_place)
  // gmres: the state of restarted GMRES (first solve with "solve_method" = 1, or the Arnoldi hook; rdc_solve.h, gmres_carve)
  // newton: the saved iterate, the update and the sums of the Newton loop of the solid system (first rdc_solid_newton; rdc_newton.h, newton_carve)
  struct { DevBuf bcol, work, voff, val32, mg_idx, mg_val, send, mg_stage, mg_gs, ilu_idx, ilu_val, ilu_f32, gmres, newton; } solve;   // mg_stage: what the collective calls of the set-up of rdc_solve_dist_mg move
  struct { DevBuf val, rhs, packed; } out;
  // sized by the call that uses them: partial results of the reductions, ...; stamps = diagnostic phase stamps, allocated = armed (rdc_debug_stamps)
  struct { DevBuf wg_max, adpm_slot, solid_post, stamps; } scratch;
  DevBuf field[RDC_FIELD_COUNT];
};

// Linear solve (rdc_solve.hip): what buf.solve holds for the uploaded mesh.  The *_ready flags say that lists are laid out for
// this mesh and belong to the builders that set them; valid says what the values behind the lists are still worth, by the rule
// of rdc_solve_state.h and by nothing else.
struct SolveState {
  bool bcol_ready = false;   // bcol holds this mesh's block column list
  bool voff_ready = false;   // voff / val32 are laid out for this mesh
  bool mg_ready = false;     // mg_idx / mg_val hold this mesh's hierarchy, mg describes it
  bool mg_dist = false;      // ... and it is the one of rdc_solve_dist_mg (ghost layers; mg_off holds the offsets of its exchanges)
  MgDev mg;
  bool gs_ready = false;     // mg_gs holds the colour lists of this mesh's (single-partition) hierarchy, gs describes them
  bool gs_dist = false;      // ... no: of its partitioned hierarchy, per rank (RDC_PRECOND_MULTIGRID_GS_LOCAL); dropped with it
  MgGsDev gs;
  std::vector<MgColours> gs_cols;   // their host copy (MgGsLevel::cptr_host points into it)
  bool ilu_ready = false;    // ilu_idx / ilu_val hold this mesh's lists, ilu describes them, ilu_host is their host copy
  IluDev ilu;
  IluHost ilu_host;          // (IluDev::cptr_host points into it; rdc_solve_ilu_download permutes with it)
  bool plan_ready = false;   // send holds this mesh's send list, dist its checked dimensions (rdc_solve_dist_plan)
  DistDims dist;
  bool peers_ready = false;  // halo0 is the plan with its per-peer segments (rdc_solve_dist_plan_peers)
  std::vector<int32_t> send_nodes;   // host copy of the plan's send list
  MgHalo halo0;
  std::vector<MgLevelHost> mg_dist_steps;   // the steps of the partitioned hierarchy, kept for the colouring of its levels
  std::vector<std::vector<int64_t>> mg_off;   // per level >= 1: send and ghost offsets in doubles, what MgLevelDev::send_off / ghost_off point at
  int gmres_cap = 0;         // the restart length buf.solve.gmres was allocated for (0: not allocated)
  GmresState gmres = GmresState();   // ... and its layout for the restart length of the call at hand
  SolveValid valid;
};

// What is only meaningful for the uploaded mesh; rdc_mesh_upload starts from MeshState().
struct MeshState {
  bool have_mesh = false;
  HostPrep prep;
  HostPrepEv prep_ev;              // element-visit lists (PIHNA TET4, shipped pattern); .ok = available
  bool ev_tried = false;           // the element-visit lists of this mesh have been built (or found impossible)
  int64_t ev_perm_interior = -2;   // "interior_nodes" value the uploaded workgroup order was built for
  PartSplit ev_part1;              // the split of that order: its leading interior workgroups, the rows complete after them
  struct ClusterLists {            // cluster lists of the HEX8 producer / consumer kernels or of k_tet4_cl (ensure_cluster_lists)
    int state = 0;                 // 0 = not built yet, 1 = ready, -1 = not available for this mesh (two-pass / the pair kernels are used)
    int waves = 31, order = 1, interior = -1;   // the options "solid_cl_waves", pair order and "interior_nodes" they were built with
    int n_wg = 0;                  // all clusters
    PartSplit part1;               // their leading clusters of interior nodes, the rows complete after those
    size_t max_row_doubles = 0;
    int64_t n_pairs = 0, n_elem_visits = 0;   // statistics (rdc_tet4_cluster_info)
  } cl;
  bool solid_gather_ready = false, rg5_eid_ready = false;   // buf.two_pass, buf.rg2.eid hold this mesh's lists
  SolveState solve;
  int64_t part1_nodes = -1;          // rows [0, part1_nodes) were complete after the LAST part-1 call (-1: none since the upload)
  bool part1_packed = false;         // part 1 of the current step has packed the owned records (consumed by part 2)
  bool solid_part1_pending = false;
  int32_t n_materials = 0;   // what rdc_solid_set_materials / rdc_solid_set_sides left in buf.solid_in
  int64_t n_sides = 0;
  int64_t field_count[RDC_FIELD_COUNT] = {};
};

}  // namespace rdc

// Four kinds of state: what lives as long as the context (below), the tuning options (opt), the settings of the linear solve
// (sopt), and what belongs to the uploaded mesh (ms, with the device buffers in buf).
struct rdc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  char err[512] = "";
  int strategy = RDC_SCATTER_AUTO;
  int variant = RDC_VARIANT_AUTO;
  int tet4_cl_mode = 0;         // rdc_tet4_cluster_mode
  int tet4_cl_active = 0;       // the last assembly call launched k_tet4_cl
  size_t tet4_cl_lds = 0;       // dynamic LDS of that launch
  rdc::Options opt;
  rdc::SolveOptions sopt;
  rdc::MeshState ms;
  rdc::Buffers buf;
  rdc::ConstRows const_rows;    // the a rows of the value array that PIHNA element-visit launches may leave (rdc_const_rows.h); coords_out outlives the mesh
  hipEvent_t pack_event = nullptr;  // two-part assembly: recorded behind part 1's pack of the owned node records
  // chunked hand-back (rdc_csr_download_rows_async): a copy stream of the context's own and a small pool of completion events
  hipStream_t copy_stream = nullptr;
  hipEvent_t copy_fence = nullptr;            // recorded on the context's stream at call time: the copy starts behind the work enqueued so far
  static constexpr int N_TICKETS = 16;
  hipEvent_t ticket[N_TICKETS] = {};
  int next_ticket = 0;
  hipEvent_t solid_part1_event = nullptr;   // recorded behind part 1 of a two-part solid assembly (the sides of part 2 wait for it)
  rdc::SolveScal* solve_rec = nullptr;   // pinned: the one record the host reads per iteration of the linear solve
  rdc::GmresRec* gmres_rec = nullptr;    // pinned: the record the host reads per Arnoldi step
  rdc::NewtonRec* newton_rec = nullptr;  // pinned: the record the host reads behind an assembly or a step of rdc_solid_newton
  rdc::NewtonHistory newton_history;     // per Newton iteration of the last rdc_solid_newton
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;   // pairs (start, stop), one pair per timed assemble call
  size_t ev_used = 0;           // events handed out since the last rdc_timing_sum_ms / enable
  size_t max_lds = 64 * 1024;
  int n_cu = 256;
};

namespace rdc {

// records the message (c null: for rdc_ctx_create's caller) and returns code
int fail(rdc_ctx* c, int code, const char* fmt, ...);

#define RDC_HIP(ctx, call)                                                                       \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) return fail(ctx, RDC_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

int dev_free(rdc_ctx* c, DevBuf& b);
int dev_alloc(rdc_ctx* c, DevBuf& b, size_t bytes);
int set_device(rdc_ctx* c);

template <class T>
int dev_upload(rdc_ctx* c, DevBuf& b, const std::vector<T>& v) {
  int rc = dev_alloc(c, b, v.size() * sizeof(T));
  if (rc) return rc;
  if (!v.empty()) RDC_HIP(c, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return RDC_OK;
}

}  // namespace rdc
#endif
