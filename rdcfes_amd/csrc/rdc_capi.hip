// rdc_capi.hip — implementation of the C-ABI declared in include/rdc_assembly.h.
// No CPU fallback lives here: every assemble call launches HIP kernels or fails.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>
#include <utility>

#include "rdc_capi_internal.h"
#include "rdc_parts.h"
#include "rdc_tet4_ev.h"
#include "rdc_tet4_cl.h"
#include "rdc_solid.h"

using namespace rdc;

namespace {

thread_local char g_create_error[512] = "";

}  // namespace

// the helpers rdc_capi_solve.hip shares (rdc_capi_internal.h)
namespace rdc {

int fail(rdc_ctx* c, int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (c) vsnprintf(c->err, sizeof(c->err), fmt, ap);
  else vsnprintf(g_create_error, sizeof(g_create_error), fmt, ap);
  va_end(ap);
  return code;
}

int dev_free(rdc_ctx* c, DevBuf& b) {
  if (b.p && b.owned) {
    hipError_t e = hipFree(b.p);
    if (e != hipSuccess) return fail(c, RDC_ERR_HIP, "hipFree failed: %s", hipGetErrorString(e));
  }
  b = DevBuf();
  return RDC_OK;
}

int dev_alloc(rdc_ctx* c, DevBuf& b, size_t bytes) {
  if (b.p && b.owned && b.bytes >= bytes && bytes > 0) return RDC_OK;
  int rc = dev_free(c, b);
  if (rc) return rc;
  if (bytes == 0) bytes = 8;
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) {
    b = DevBuf();
    return fail(c, RDC_ERR_ALLOC, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  b.bytes = bytes;
  b.owned = true;
  return RDC_OK;
}

int set_device(rdc_ctx* c) {
  RDC_HIP(c, hipSetDevice(c->device));
  return RDC_OK;
}

}  // namespace rdc

namespace {

// ---- device views of the buffer groups (cluster_view: behind ensure_cluster_lists) ----
MeshDev mesh_view(const rdc_ctx* c) {
  MeshDev m;
  m.n_elem = c->ms.prep.n_elem; m.n_node = c->ms.prep.n_node; m.n_owned = c->ms.prep.n_owned;
  m.conn = (const uint32_t*)c->buf.mesh.conn.p;
  m.xyz = (const double*)c->buf.mesh.xyz.p;
  m.bptr = (const int64_t*)c->buf.mesh.bptr.p;
  m.eslot = (const uint16_t*)c->buf.mesh.eslot.p;
  m.elem_order = (const uint32_t*)c->buf.mesh.elem_order.p;
  m.first_mask = (const uint64_t*)c->buf.mesh.first_mask.p;
  m.first_rhs = (const uint8_t*)c->buf.mesh.first_rhs.p;
  m.pair_elem = (const uint32_t*)c->buf.mesh.pair_elem.p;
  m.pair_local = (const uint8_t*)c->buf.mesh.pair_local.p;
  m.node_pair_ptr = (const int64_t*)c->buf.mesh.node_pair_ptr.p;
  m.wg_node_ptr = (const int32_t*)c->buf.mesh.wg_node_ptr.p;
  return m;
}

// TET4 pair lists (empty view: not available for this mesh); pair_eid is filled in by the models that read it (assemble_rd)
Rg2Dev rg2_view(const rdc_ctx* c) {
  Rg2Dev r;
  const HostPrep& P = c->ms.prep;
  const auto& b = c->buf.rg2;
  if (!P.rg2_ok || P.nen != 4) return r;
  r.n_wg = (int)P.wg2.size();
  r.desc = (const HostPrep::WgDesc*)b.desc.p;
  r.pair_rec = (const uint32_t*)b.pair.p;
  r.chunk = (const HostPrep::Chunk*)b.chunk.p;
  r.sdesc = (const HostPrep::StoreDesc*)b.sdesc.p;
  r.contrib = (const uint16_t*)b.contrib.p;
  r.pair_aux = (const uint16_t*)b.aux.p;
  r.node_tab = (const uint16_t*)b.ntab.p;
  if (P.nl_stride > 0) {
    r.nlist = (const uint32_t*)b.nlist.p;
    r.pair_loc = (const uint32_t*)b.ploc.p;
    r.nl_stride = P.nl_stride;
  }
  r.lds_bytes = P.rg2_lds_bytes;
  r.block = P.rg2_block;
  return r;
}

// element-visit lists of the whole mesh (the two-part calls add the workgroup order and their sub-range)
EvDev ev_view(const rdc_ctx* c) {
  EvDev v;
  const auto& b = c->buf.ev;
  v.n_wg = (int)c->ms.prep_ev.desc.size();
  v.desc = (const HostPrepEv::Desc*)b.desc.p;
  v.nlist = (const uint32_t*)b.nlist.p;
  v.vloc = (const uint32_t*)b.vloc.p;
  v.vslot = (const uint32_t*)b.vslot.p;
  v.ntab = (const HostPrepEv::Node*)b.ntab.p;
  v.bpart = (const uint8_t*)b.bpart.p;
  v.nls = c->ms.prep_ev.nls;
  v.max_out_doubles = c->ms.prep_ev.max_out_doubles;
  return v;
}

// frees every buffer of a group (a struct or array of DevBufs and nothing else)
template <class G>
void free_group(rdc_ctx* c, G& g) {
  static_assert(std::is_standard_layout<G>::value && sizeof(G) % sizeof(DevBuf) == 0, "a buffer group holds DevBufs only");
  DevBuf* b = reinterpret_cast<DevBuf*>(&g);
  for (size_t i = 0; i < sizeof(G) / sizeof(DevBuf); i++) dev_free(c, b[i]);
}
template <class G, class... Rest>
void free_group(rdc_ctx* c, G& g, Rest&... rest) { free_group(c, g); free_group(c, rest...); }

int64_t field_width(const rdc_ctx* c, int field) {
  switch (field) {
    case RDC_FIELD_OLD_SOLUTION: return c->ms.prep.nvar;
    case RDC_FIELD_AUX_NODAL: return 3;
    case RDC_FIELD_UNDEFORMED_XYZ: return 3;
    case RDC_FIELD_ELEM_FIBRE: return 3;
    case RDC_FIELD_PREV_SOLUTION: return c->ms.prep.nvar;
    case RDC_FIELD_TIME_DERIV: return c->ms.prep.nvar;
    case RDC_FIELD_RT_DOSE: return 3;
  }
  return 0;
}

int64_t field_expected(const rdc_ctx* c, int field) {
  const int64_t rows = (field == RDC_FIELD_ELEM_FIBRE) ? c->ms.prep.n_elem : c->ms.prep.n_node;
  return rows * field_width(c, field);
}

bool rowgather_available(const rdc_ctx* c) {
  return c->ms.prep.rowgather_ok || (c->ms.prep.rg2_ok && c->ms.prep.nen == 4 && c->variant != RDC_VARIANT_GENERIC);
}

// the scatter strategy with AUTO resolved
int strategy_of(const rdc_ctx* c) {
  if (c->strategy != RDC_SCATTER_AUTO) return c->strategy;
  return rowgather_available(c) ? RDC_SCATTER_ROWGATHER : RDC_SCATTER_COLOURED;
}

int resolve_strategy(rdc_ctx* c, int* out) {
  *out = strategy_of(c);
  if (*out == RDC_SCATTER_ROWGATHER && !rowgather_available(c))
    return fail(c, RDC_ERR_UNSUPPORTED, "row-gather scatter unavailable: a node row exceeds the LDS budget");
  return RDC_OK;
}

// What the kernel-path decision (rdc_path.h) reads of the context and the lists its mesh has at this moment.  The two facts that
// depend on the model are the caller's: pattern, and cl_fits (the LDS image of k_tet4_cl)
Facts path_facts(const rdc_ctx* c, int strategy) {
  const MeshState::ClusterLists& L = c->ms.cl;
  Facts f;
  f.strategy = strategy; f.variant = c->variant; f.opt = c->opt; f.tet4_cl_mode = c->tet4_cl_mode;
  f.stamps = c->buf.scratch.stamps.p != nullptr;
  list_facts(c->ms.prep, c->ms.prep_ev, f);
  f.ev_tried = c->ms.ev_tried;
  f.cl_ready = L.state == 1 && L.waves == c->opt.solid_cl_waves && L.interior == c->opt.interior_nodes &&
               (c->opt.solid_cl_order < 0 || L.order == c->opt.solid_cl_order);   // what ensure_cluster_lists would keep
  return f;
}

// hands out the next (start, stop) event pair of the timing pool, growing it on demand
int next_event_pair(rdc_ctx* c, hipEvent_t* start, hipEvent_t* stop) {
  if (c->ev_used + 2 > c->ev.size()) {
    for (int x = 0; x < 2; x++) {
      hipEvent_t e = nullptr;
      RDC_HIP(c, hipEventCreate(&e));
      c->ev.push_back(e);
    }
  }
  *start = c->ev[c->ev_used];
  *stop = c->ev[c->ev_used + 1];
  c->ev_used += 2;
  return RDC_OK;
}

// instantiation I of model M on the path of the plan
template <class M, class I>
hipError_t launch_path(const LaunchArgs& a, const typename M::K& k) {
  switch (a.plan.path) {
    case Path::TET4_CL: return launch_tet4_cl<I>(a, k);
    case Path::TET4_EV:
      if constexpr (std::is_same<M, Pihna>::value) return launch_tet4_ev(a, k);
      break;
    case Path::TET4_EVC: case Path::TET4_RG5: case Path::TET4_RG3: case Path::TET4_RG2: case Path::TET4_ROWGATHER: case Path::TET4_COLOURED:
      return launch_tet4_fast<I>(a, k);
    case Path::HEX8_CL: case Path::HEX8_CL_ROWS: case Path::GENERIC_ROWGATHER: case Path::GENERIC_COLOURED:
      if constexpr (std::is_same<M, I>::value || !Forms<M>::TET4_ONLY) return launch_rd<I>(a, k);
      break;
  }
  return hipErrorInvalidValue;   // a path this instantiation does not have
}

template <class M>
hipError_t launch_specialised(const LaunchArgs& a, const typename M::K& k) {
  switch (a.plan.inst) {
    case Inst::SPARSE: return launch_path<M, typename Forms<M>::Sparse>(a, k);
    case Inst::MOMENTS:
      if constexpr (std::is_same<M, Pihna>::value) return launch_path<M, PihnaNoCellTransportMoments>(a, k);
      return hipErrorInvalidValue;
    case Inst::FULL: break;
  }
  return launch_path<M, M>(a, k);
}

// two-part assembly on the element-visit lists: (re)builds the workgroup order for the current "interior_nodes":
// clusters all of whose nodes are below it first (the split itself: rdc_parts.h)
int ev_order_for_interior(rdc_ctx* c) {
  if (c->ms.ev_perm_interior == c->opt.interior_nodes && c->buf.ev.perm.p) return RDC_OK;
  std::vector<uint32_t> perm;
  c->ms.ev_part1 = split_ev(c->ms.prep_ev.desc, c->opt.interior_nodes, &perm);
  int rc = dev_upload(c, c->buf.ev.perm, perm);
  if (rc) return rc;
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  c->ms.ev_perm_interior = c->opt.interior_nodes;
  return RDC_OK;
}

// two-part assembly: the leading row-gather workgroups that part 1 launches and the rows complete after them
PartSplit part1_pairs(const rdc_ctx* c) { return split_pairs(c->ms.prep.wg2, c->opt.interior_nodes); }

// the context keeps the connectivity on the device only: the list builders of the first assembly read a host copy
int download_conn(rdc_ctx* c, std::vector<uint32_t>& conn_h) {
  conn_h.resize((size_t)c->ms.prep.n_elem * c->ms.prep.nen);
  RDC_HIP(c, hipMemcpyAsync(conn_h.data(), c->buf.mesh.conn.p, conn_h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  return RDC_OK;
}

// element-visit lists (rdc_prep_ev.cpp) of the current mesh: at the upload for five unknowns (PIHNA), on the first
// assembly for three (RIPF / HCC).  A mesh they cannot describe simply keeps the pair kernels (prep_ev.ok stays false).
int build_ev_lists(rdc_ctx* c, const uint32_t* conn) {
  int rc;
  c->ms.ev_tried = true;
  const HostPrep& P = c->ms.prep;
  const std::string ev_err = prep_build_ev(P, conn, (size_t)c->opt.ev_lds, c->ms.prep_ev, c->opt.interior_nodes <= P.n_owned ? c->opt.interior_nodes : -1);
  if (!ev_err.empty()) { c->ms.prep_ev = HostPrepEv(); return RDC_OK; }
  if ((rc = dev_upload(c, c->buf.ev.desc, c->ms.prep_ev.desc))) return rc;
  if ((rc = dev_upload(c, c->buf.ev.nlist, c->ms.prep_ev.nlist))) return rc;
  if ((rc = dev_upload(c, c->buf.ev.vloc, c->ms.prep_ev.vloc))) return rc;
  if ((rc = dev_upload(c, c->buf.ev.vslot, c->ms.prep_ev.vslot))) return rc;
  if ((rc = dev_upload(c, c->buf.ev.ntab, c->ms.prep_ev.ntab))) return rc;
  if ((rc = dev_upload(c, c->buf.ev.bpart, c->ms.prep_ev.bpart))) return rc;
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  // the big host copies are not needed again (the descriptors are: two-part order)
  std::vector<uint32_t>().swap(c->ms.prep_ev.nlist); std::vector<uint32_t>().swap(c->ms.prep_ev.vloc);
  std::vector<uint32_t>().swap(c->ms.prep_ev.vslot);
  return RDC_OK;
}

// cluster lists of the producer / consumer HEX8 kernels (three unknowns: solid system and reaction-diffusion models share
// them) or, on a TET4 mesh, of k_tet4_cl (cll::tet4_limits), built on first use.  ms.cl.state: 1 = ready, -1 = not available
// for this mesh (c->err says why).
int ensure_cluster_lists(rdc_ctx* c, int order_of_caller) {
  int rc;
  MeshState::ClusterLists& L = c->ms.cl;
  const int want_order = c->opt.solid_cl_order < 0 ? (L.state == 1 ? L.order : order_of_caller) : c->opt.solid_cl_order;
  if (L.state != 0 && (L.waves != c->opt.solid_cl_waves || L.order != want_order || L.interior != c->opt.interior_nodes)) L.state = 0;
  if (L.state != 0) return RDC_OK;
  const int nen = c->ms.prep.nen;   // 4: the lists of k_tet4_cl (rdc_tet4_cluster_mode)
  HostPrepCl::Limits lim = nen == 4 ? cll::tet4_limits(c->ms.prep.nvar) : cll::limits(c->opt.solid_cl_waves / 10, c->opt.solid_cl_waves % 10, c->ms.prep.nvar);
  lim.pair_order = want_order;
  HostPrepCl cl;
  std::vector<uint32_t> conn_h;
  if ((rc = download_conn(c, conn_h))) return rc;
  const std::string err = prep_build_cl(c->ms.prep, conn_h.data(), lim, cl, c->opt.interior_nodes);
  L = MeshState::ClusterLists();
  L.interior = c->opt.interior_nodes; L.waves = c->opt.solid_cl_waves; L.order = want_order;
  if (!err.empty()) {
    L.state = -1;
    std::snprintf(c->err, sizeof(c->err), "%s", err.c_str());
    return RDC_OK;
  }
  if ((rc = dev_upload(c, c->buf.cl.desc, cl.desc))) return rc;
  if ((rc = dev_upload(c, c->buf.cl.ntab, cl.ntab))) return rc;
  if ((rc = dev_upload(c, c->buf.cl.eid, cl.eid))) return rc;
  if ((rc = dev_upload(c, c->buf.cl.pair, cl.pair))) return rc;
  if ((rc = dev_upload(c, c->buf.cl.pslot, cl.pslot))) return rc;
  RDC_HIP(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
  L.max_row_doubles = cl.max_row_doubles;
  L.n_wg = (int)cl.desc.size();
  L.n_pairs = cl.n_pairs; L.n_elem_visits = cl.n_elem_visits;
  if (L.interior >= 0) L.part1 = PartSplit{(int)cl.n_wg_interior, cl.part1_nodes};
  L.state = 1;
  return RDC_OK;
}

// part 0: every cluster; 1: the leading clusters of interior nodes; 2: the rest (the kernels index the lists by blockIdx.x)
ClDev cluster_view(const rdc_ctx* c, int part = 0) {
  const MeshState::ClusterLists& L = c->ms.cl;
  ClDev v;
  v.cw = L.waves / 10; v.pw = L.waves % 10;
  const size_t b = part == 2 ? (size_t)L.part1.wg : 0;
  v.n_wg = part == 1 ? L.part1.wg : (part == 2 ? L.n_wg - L.part1.wg : L.n_wg);
  const cll::Strides S = c->ms.prep.nen == 4 ? cll::strides(cll::tet4_limits(c->ms.prep.nvar), 4) : cll::strides(v.cw, v.pw, c->ms.prep.nen);
  v.desc = (const HostPrepCl::Desc*)c->buf.cl.desc.p + b;
  v.ntab = (const HostPrepCl::Node*)c->buf.cl.ntab.p + b * S.node;
  v.eid = (const uint32_t*)c->buf.cl.eid.p + b * S.elem;
  v.pair = (const uint32_t*)c->buf.cl.pair.p + b * S.pair;
  v.pslot = (const uint32_t*)c->buf.cl.pslot.p + b * S.pslot;
  v.max_row_doubles = L.max_row_doubles;
  return v;
}

template <class M, class P>
int assemble_rd(rdc_ctx* c, const P* p, int nvar_expected, bool need_aux) {
  if (!c) return RDC_ERR_INVALID;
  c->tet4_cl_active = 0;
  if (!p) return fail(c, RDC_ERR_INVALID, "null parameter struct");
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "assemble called before rdc_mesh_upload");
  if (c->ms.prep.nvar != nvar_expected)
    return fail(c, RDC_ERR_INVALID, "model needs nvar=%d, mesh was uploaded with nvar=%d", nvar_expected, c->ms.prep.nvar);
  if (!c->buf.field[RDC_FIELD_OLD_SOLUTION].p) return fail(c, RDC_ERR_STATE, "old solution field not set");
  if (need_aux && !c->buf.field[RDC_FIELD_AUX_NODAL].p) return fail(c, RDC_ERR_STATE, "aux nodal field not set");
  if (M::NELEM > 0 && (!c->buf.field[RDC_FIELD_ELEM_TRACTS].p || c->ms.field_count[RDC_FIELD_ELEM_TRACTS] != (int64_t)M::NELEM * c->ms.prep.n_elem))
    return fail(c, RDC_ERR_STATE, "per-element field (tracts) not set");
  int rc = set_device(c);
  if (rc) return rc;
  const typename M::K k = M::derive(*p);
  LaunchArgs a;
  a.m = mesh_view(c);
  a.nen = c->ms.prep.nen;
  a.exp_mode = exp_mode_of(M::exponent(k)) == M::FAST_EXP_MODE ? M::FAST_EXP_MODE : 0;
  int strategy;
  rc = resolve_strategy(c, &strategy);
  if (rc) return rc;
  a.u = (const double*)c->buf.field[RDC_FIELD_OLD_SOLUTION].p;
  a.aux = (const double*)c->buf.field[RDC_FIELD_AUX_NODAL].p;
  a.elem = (const double*)c->buf.field[RDC_FIELD_ELEM_TRACTS].p;
  if (c->ms.prep.hx_ok) {
    a.hx_nl_ptr = (const int64_t*)c->buf.hx.nl_ptr.p;
    a.hx_nlist = (const uint32_t*)c->buf.hx.nlist.p;
    a.hx_ploc = (const uint16_t*)c->buf.hx.ploc.p;
    a.hx_max_nodes = c->ms.prep.hx_max_nodes;
  }
  a.packed = (double*)c->buf.out.packed.p;
  a.opt = c->opt;
  a.stamps = (long long*)c->buf.scratch.stamps.p;
  a.rg2 = rg2_view(c);
  // Which kernel runs (rdc_path.h; DESIGN.md, "Which kernel runs"): the lists the call builds on first use, then the plan.  A refused
  // list build (c->err says why) leaves the call on the path it would have taken without the lists
  constexpr PathModel model = describe<M>();
  Facts f = path_facts(c, strategy);
  f.pattern = Forms<M>::pattern(*p);
  const Builds b = path_builds(model, f);
  if (b.pair_eid) {
    if (!c->ms.rg5_eid_ready) {
      if ((rc = dev_upload(c, c->buf.rg2.eid, c->ms.prep.pair_eid))) return rc;
      c->ms.rg5_eid_ready = true;
    }
    a.rg2.pair_eid = (const uint32_t*)c->buf.rg2.eid.p;
  }
  if (b.ev) {
    std::vector<uint32_t> conn_h;
    if ((rc = download_conn(c, conn_h))) return rc;
    if ((rc = build_ev_lists(c, conn_h.data()))) return rc;
    f.ev_ok = c->ms.prep_ev.ok;
  }
  if (b.tet4_cl || b.hex8_cl) {
    if ((rc = ensure_cluster_lists(c, b.tet4_cl ? 1 : 0))) return rc;
    f.cl_ready = c->ms.cl.state == 1;
    f.cl_fits = tet4_cl_lds_bytes<M>(c->ms.cl.max_row_doubles) <= c->max_lds;
  }
  const Plan plan = a.plan = path_decide(model, f);
  // the a rows of the value array (rdc_const_rows.h) are kept by the PIHNA element-visit launches alone: any other assembly of the
  // context -- another path, another model, a timing-only build ("ablate" 1-3: wrong results) -- forgets them
  const bool const_rows_path = std::is_same<M, Pihna>::value && plan.path == Path::TET4_EV && (c->opt.ablate == 0 || c->opt.ablate == 4);
  if (!const_rows_path) c->const_rows.other_assembly();
  if (c->opt.ev_resident) {   // cluster counter of the resident kernel
    if ((rc = dev_alloc(c, c->buf.ev.ticket, 256))) return rc;   // [0]: whole launches and part 1, [16]: part 2
    a.ev_ticket = (int*)c->buf.ev.ticket.p;
  }
  a.ev_grid = c->opt.grid > 0 ? c->opt.grid : 2 * c->n_cu;
  if (plan.path == Path::TET4_EV || plan.path == Path::TET4_EVC || plan.two_part == TwoPart::EV_SPLIT) a.ev = ev_view(c);
  // Two-part assembly (halo overlap): part 1 = the leading work items of the path's lists whose nodes are all interior, part 2 = the
  // rest.  A path that launches no sub-ranges assembles nothing in part 1 and everything in part 2
  const int part = c->opt.part;
  PartSplit split;   // the work items of part 1 and the rows complete after them
  switch (plan.two_part) {
    case TwoPart::WHOLE: c->ms.part1_packed = false; break;
    case TwoPart::CL_SPLIT:   // the cluster lists respect "interior_nodes" (interior clusters first)
      c->ms.part1_packed = false;
      if (part == 1) {
        c->ms.part1_nodes = c->ms.cl.part1.wg > 0 ? c->ms.cl.part1.nodes : 0;
        if (c->ms.cl.part1.wg == 0) return RDC_OK;
      }
      a.cl = cluster_view(c, c->ms.cl.interior >= 0 ? part : (part == 2 ? 0 : 1));
      if (a.cl.n_wg == 0) return RDC_OK;
      break;
    case TwoPart::EV_SPLIT:
      if (c->opt.interior_nodes < 0) return fail(c, RDC_ERR_STATE, "\"part\" needs \"interior_nodes\"");
      if ((rc = ev_order_for_interior(c))) return rc;
      a.ev.wg_perm = (const uint32_t*)c->buf.ev.perm.p;
      split = c->ms.ev_part1;
      break;
    case TwoPart::PAIR_SPLIT: split = part1_pairs(c); break;
    case TwoPart::ALL_IN_PART2: break;
  }
  if (plan.two_part == TwoPart::EV_SPLIT || plan.two_part == TwoPart::PAIR_SPLIT || plan.two_part == TwoPart::ALL_IN_PART2) {
    const bool ev = plan.two_part == TwoPart::EV_SPLIT;
    int& wg_begin = ev ? a.ev.wg_begin : a.rg2.wg_begin;
    int& wg_count = ev ? a.ev.wg_count : a.rg2.wg_count;
    if (part == 1) {
      c->ms.part1_packed = false;
      c->ms.part1_nodes = 0;
      if (split.wg == 0) return RDC_OK;
      c->ms.part1_nodes = split.nodes;
      wg_begin = 0; wg_count = split.wg;
      // part 1 packs the records of the owned nodes only and part 2 those of the ghosts, ordered by an event: the two
      // parts may run on different streams (rdc_assembly.h, stream contract of the two-part assembly)
      if (!c->pack_event) RDC_HIP(c, hipEventCreateWithFlags(&c->pack_event, hipEventDisableTiming));
      a.pack_part = 1; a.pack_event = c->pack_event;
      c->ms.part1_packed = true;
    } else {
      wg_begin = split.wg; wg_count = -1;
      if (plan.two_part != TwoPart::ALL_IN_PART2 && c->ms.part1_packed) { a.pack_part = 2; a.pack_event = c->pack_event; }
      c->ms.part1_packed = false;
    }
  }
  const bool hex8_cl = plan.path == Path::HEX8_CL || plan.path == Path::HEX8_CL_ROWS;
  if ((hex8_cl || plan.path == Path::TET4_CL) && part == 0) {
    a.cl = cluster_view(c);
    a.cl.grid = hex8_cl && c->opt.hex_kernel == 2 ? 2 * c->n_cu : 0;   // persistent form: the workgroups resident at once
  }
  if (plan.path == Path::TET4_CL) {   // what rdc_tet4_cluster_info reports (a part without clusters has returned above)
    c->tet4_cl_active = 1;
    c->tet4_cl_lds = tet4_cl_lds_bytes<M>(a.cl.max_row_doubles);
  }
  a.val = (double*)c->buf.out.val.p;
  a.rhs = (double*)c->buf.out.rhs.p;
  a.stream = c->stream;
  a.colour_ptr = c->ms.prep.colour_ptr.data();
  a.n_colours = c->ms.prep.n_colours;
  a.n_wg = c->ms.prep.rowgather_ok ? (int)c->ms.prep.wg_node_ptr.size() - 1 : 0;
  a.lds_bytes = c->ms.prep.rg_lds_bytes;
  a.ev_start = nullptr;
  hipEvent_t ev_stop = nullptr;
  if (c->timing) {
    if ((rc = next_event_pair(c, &a.ev_start, &ev_stop))) return rc;
  }
  ConstRowsKey rows_key;
  bool capturing = false;
  if constexpr (std::is_same<M, Pihna>::value) {
    if (const_rows_path) {
      rows_key = const_rows_key(k);
      // a launch recorded into a graph writes every row: a replay must not depend on what the host knew at capture time.  A
      // query that fails (another stream of the thread is capturing) counts as capturing
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess) { (void)hipGetLastError(); capturing = true; }
      else capturing = cs != hipStreamCaptureStatusNone;
      a.ev_rows = c->const_rows.rows(c->const_rows.mode, rows_key, plan.two_part == TwoPart::WHOLE ? 0 : part, c->opt.interior_nodes, capturing);
    }
  }
  hipError_t e = launch_specialised<M>(a, k);
  if (const_rows_path) c->const_rows.launched(a.ev_rows, rows_key, plan.two_part == TwoPart::WHOLE ? 0 : part, capturing, e == hipSuccess);
  if (e != hipSuccess) return fail(c, RDC_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
  if (c->timing) RDC_HIP(c, hipEventRecord(ev_stop, c->stream));
  return RDC_OK;
}

// one call per part of a two-part step: "part" and the stream for this call only (a step of the multi-GPU harness is then
// two C-ABI calls instead of six: set_option, assemble, set_stream, set_option, assemble, set_stream)
template <class F>
int with_part(rdc_ctx* c, int part, void* stream, F&& call) {
  if (!c) return RDC_ERR_INVALID;
  if (part < 0 || part > 2) return fail(c, RDC_ERR_INVALID, "part must be 0, 1 or 2");
  const int part0 = c->opt.part;
  const hipStream_t s0 = c->stream;
  c->opt.part = part;
  c->stream = (hipStream_t)stream;
  const int rc = call();
  c->opt.part = part0;
  c->stream = s0;
  return rc;
}
}  // namespace

extern "C" {

int rdc_abi_version(void) { return RDC_ABI_VERSION; }

const char* rdc_last_error(const rdc_ctx* ctx) { return ctx ? ctx->err : g_create_error; }

int rdc_device_count(int* n) {
  if (!n) return RDC_ERR_INVALID;
  int ndev = 0;
  const hipError_t e = hipGetDeviceCount(&ndev);
  *n = e == hipSuccess ? ndev : 0;
  return e == hipSuccess ? RDC_OK : fail(nullptr, RDC_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
}

int rdc_ctx_create(int device_ordinal, rdc_ctx** out) {
  if (!out) return fail(nullptr, RDC_ERR_INVALID, "null output pointer");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail(nullptr, RDC_ERR_HIP, "no HIP device available (%s); this library has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (device_ordinal < 0 || device_ordinal >= ndev)
    return fail(nullptr, RDC_ERR_INVALID, "device ordinal %d out of range [0,%d)", device_ordinal, ndev);
  rdc_ctx* c = new (std::nothrow) rdc_ctx();
  if (!c) return fail(nullptr, RDC_ERR_ALLOC, "out of host memory");
  c->device = device_ordinal;
  e = hipSetDevice(device_ordinal);
  if (e != hipSuccess) {
    delete c;
    return fail(nullptr, RDC_ERR_HIP, "device initialisation failed: %s", hipGetErrorString(e));
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) {
    if (prop.sharedMemPerBlock > 0) c->max_lds = prop.sharedMemPerBlock;
    if (prop.sharedMemPerBlockOptin > c->max_lds) c->max_lds = prop.sharedMemPerBlockOptin;   // what hipFuncSetAttribute may raise a kernel to
    if (prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
  }
  *out = c;
  return RDC_OK;
}

int rdc_ctx_destroy(rdc_ctx* c) {
  if (!c) return RDC_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  free_group(c, c->buf);
  if (c->solve_rec) (void)hipHostFree(c->solve_rec);
  if (c->gmres_rec) (void)hipHostFree(c->gmres_rec);
  if (c->newton_rec) (void)hipHostFree(c->newton_rec);
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  if (c->pack_event) (void)hipEventDestroy(c->pack_event);
  if (c->solid_part1_event) (void)hipEventDestroy(c->solid_part1_event);
  if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
  if (c->copy_fence) (void)hipEventDestroy(c->copy_fence);
  for (hipEvent_t e : c->ticket) if (e) (void)hipEventDestroy(e);
  delete c;
  return RDC_OK;
}

int rdc_set_stream(rdc_ctx* c, void* s) {
  if (!c) return RDC_ERR_INVALID;
  c->stream = (hipStream_t)s;
  return RDC_OK;
}

int rdc_synchronize(rdc_ctx* c) {
  if (!c) return RDC_ERR_INVALID;
  int rc = set_device(c);
  if (rc) return rc;
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  return RDC_OK;
}

int rdc_set_scatter(rdc_ctx* c, int s) {
  if (!c) return RDC_ERR_INVALID;
  if (s != RDC_SCATTER_AUTO && s != RDC_SCATTER_COLOURED && s != RDC_SCATTER_ROWGATHER)
    return fail(c, RDC_ERR_INVALID, "unknown scatter strategy %d", s);
  c->strategy = s;
  return RDC_OK;
}

int rdc_set_kernel_variant(rdc_ctx* c, int v) {
  if (!c) return RDC_ERR_INVALID;
  if (v != RDC_VARIANT_AUTO && v != RDC_VARIANT_GENERIC) return fail(c, RDC_ERR_INVALID, "unknown kernel variant %d", v);
  c->variant = v;
  return RDC_OK;
}

int rdc_set_option(rdc_ctx* c, const char* key, int value) {
  if (!c || !key) return RDC_ERR_INVALID;
  if (!std::strcmp(key, "const_rows")) {   // rdc_const_rows.h: a contract with the caller about the value array, not a tuning knob of a kernel
    if (!const_rows_mode_ok(value)) return fail(c, RDC_ERR_INVALID, "%s", CONST_ROWS_REFUSED);
    c->const_rows.mode = value;
    return RDC_OK;
  }
  if (solve_option_known(key)) return solve_options_set(c->sopt, key, value, c->err, sizeof(c->err));   // the two tables of rdc_options.h
  return options_set(c->opt, key, value, c->err, sizeof(c->err));
}

int rdc_get_scatter(const rdc_ctx* c, int* s) {
  if (!c || !s) return RDC_ERR_INVALID;
  int r = c->strategy;
  if (r == RDC_SCATTER_AUTO && c->ms.have_mesh) r = c->ms.prep.rowgather_ok ? RDC_SCATTER_ROWGATHER : RDC_SCATTER_COLOURED;
  *s = r;
  return RDC_OK;
}

int rdc_mesh_upload(rdc_ctx* c, int elem_type, int64_t n_elem, int64_t n_node, int64_t n_owned,
                    const uint32_t* conn, const double* xyz, int nvar) {
  if (!c) return RDC_ERR_INVALID;
  if (!conn || !xyz) return fail(c, RDC_ERR_INVALID, "null mesh arrays");
  int rc = set_device(c);
  if (rc) return rc;
  c->ms.have_mesh = false;
  c->const_rows.mesh_upload();
  // LDS budget of a row-gather workgroup: half the per-block limit keeps two workgroups per CU
  const size_t budget = c->max_lds >= 64 * 1024 ? 50 * 1024 : c->max_lds / 2;
  std::string err = prep_build(elem_type, n_elem, n_node, n_owned, conn, nvar, budget, c->opt.block, c->ms.prep, c->opt.schedule != 0);
  if (!err.empty()) return fail(c, RDC_ERR_INVALID, "%s", err.c_str());   // a refused mesh leaves the fields of the previous one as they are
  // from here on nothing of the previous mesh is left: its state (all but the lists just built), its fields and solid inputs
  // (sized by the mesh), the lists built on first use, the per-call scratch and armed stamps
  { MeshState fresh; fresh.prep = std::move(c->ms.prep); c->ms = std::move(fresh); }
  Buffers& b = c->buf;
  free_group(c, b.field, b.solid_in, b.ev, b.cl, b.two_pass, b.solve, b.scratch);
  const HostPrep& P = c->ms.prep;
  if (!P.hx_ok) free_group(c, b.hx);   // the lists this mesh does not have
  if (!(P.rg2_ok && elem_type == RDC_TET4)) free_group(c, b.rg2);
  std::vector<uint32_t> conn_v(conn, conn + n_elem * elem_type);
  std::vector<double> xyz_v(xyz, xyz + n_node * 3);
  if ((rc = dev_upload(c, c->buf.mesh.conn, conn_v))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.xyz, xyz_v))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.bptr, P.bptr))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.eslot, P.eslot))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.elem_order, P.elem_order))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.first_mask, P.first_mask))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.first_rhs, P.first_rhs))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.pair_elem, P.pair_elem))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.pair_local, P.pair_local))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.node_pair_ptr, P.node_pair_ptr))) return rc;
  if ((rc = dev_upload(c, c->buf.mesh.wg_node_ptr, P.wg_node_ptr))) return rc;
  if (P.hx_ok) {
    if ((rc = dev_upload(c, c->buf.hx.nl_ptr, P.hx_nl_ptr))) return rc;
    if ((rc = dev_upload(c, c->buf.hx.nlist, P.hx_nlist))) return rc;
    if ((rc = dev_upload(c, c->buf.hx.ploc, P.hx_ploc))) return rc;
  }
  if (P.rg2_ok && elem_type == RDC_TET4) {
    if ((rc = dev_upload(c, c->buf.rg2.desc, P.wg2))) return rc;
    if ((rc = dev_upload(c, c->buf.rg2.pair, P.pair_rec))) return rc;
    if ((rc = dev_upload(c, c->buf.rg2.chunk, P.chunk))) return rc;
    if ((rc = dev_upload(c, c->buf.rg2.sdesc, P.sdesc))) return rc;
    if ((rc = dev_upload(c, c->buf.rg2.contrib, P.contrib))) return rc;
    if ((rc = dev_upload(c, c->buf.rg2.aux, P.pair_aux))) return rc;
    if ((rc = dev_upload(c, c->buf.rg2.ntab, P.node_tab))) return rc;
    if (P.nl_stride > 0) {
      if ((rc = dev_upload(c, c->buf.rg2.nlist, P.nlist))) return rc;
      if ((rc = dev_upload(c, c->buf.rg2.ploc, P.pair_loc))) return rc;
    }
  }
  if (elem_type == RDC_TET4 && nvar == 5 && P.rg2_ok) {
    // element-visit lists of the PIHNA kernel; a mesh they cannot describe simply keeps the pair kernels
    // "interior_nodes" set BEFORE the upload lets the clusters respect the interior / near-ghost split (two-part assembly)
    if ((rc = build_ev_lists(c, conn))) return rc;
  }
  const size_t nnz = (size_t)nvar * nvar * P.bptr[n_owned];
  if ((rc = dev_alloc(c, c->buf.out.val, nnz * sizeof(double)))) return rc;
  if ((rc = dev_alloc(c, c->buf.out.rhs, (size_t)n_owned * nvar * sizeof(double)))) return rc;
  if (elem_type == RDC_TET4 && (rc = dev_alloc(c, c->buf.out.packed, (size_t)n_node * 12 * sizeof(double)))) return rc;
  RDC_HIP(c, hipMemsetAsync(c->buf.out.val.p, 0, c->buf.out.val.bytes, c->stream));
  RDC_HIP(c, hipMemsetAsync(c->buf.out.rhs.p, 0, c->buf.out.rhs.bytes, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  c->ms.have_mesh = true;
  return RDC_OK;
}

int rdc_mesh_update_coords(rdc_ctx* c, const double* xyz) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (!xyz) return fail(c, RDC_ERR_INVALID, "null coordinates");
  int rc = set_device(c);
  if (rc) return rc;
  c->const_rows.coords_update();
  RDC_HIP(c, hipMemcpyAsync(c->buf.mesh.xyz.p, xyz, (size_t)c->ms.prep.n_node * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  return RDC_OK;
}

int rdc_mesh_coords_device_ptr(rdc_ctx* c, double** d) {
  if (!c || !d) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  *d = (double*)c->buf.mesh.xyz.p;
  c->const_rows.coords_pointer();   // the caller may move nodes at any time from now on
  return RDC_OK;
}

int rdc_mesh_dims(const rdc_ctx* c, int64_t* n_elem, int64_t* n_node, int64_t* n_owned, int* elem_type,
                  int* nvar, int* n_colours) {
  if (!c || !c->ms.have_mesh) return RDC_ERR_STATE;
  if (n_elem) *n_elem = c->ms.prep.n_elem;
  if (n_node) *n_node = c->ms.prep.n_node;
  if (n_owned) *n_owned = c->ms.prep.n_owned;
  if (elem_type) *elem_type = c->ms.prep.nen;
  if (nvar) *nvar = c->ms.prep.nvar;
  if (n_colours) *n_colours = c->ms.prep.n_colours;
  return RDC_OK;
}

int rdc_csr_dims(const rdc_ctx* c, int64_t* n_rows, int64_t* nnz) {
  if (!c || !c->ms.have_mesh) return RDC_ERR_STATE;
  if (n_rows) *n_rows = c->ms.prep.n_owned * c->ms.prep.nvar;
  if (nnz) *nnz = (int64_t)c->ms.prep.nvar * c->ms.prep.nvar * c->ms.prep.bptr[c->ms.prep.n_owned];
  return RDC_OK;
}

int rdc_csr_pattern_download(const rdc_ctx* c, int64_t* row_ptr, int32_t* col_idx) {
  if (!c || !c->ms.have_mesh) return RDC_ERR_STATE;
  if (!row_ptr || !col_idx) return RDC_ERR_INVALID;
  const HostPrep& P = c->ms.prep;
  const int nv = P.nvar;
  row_ptr[0] = 0;
  for (int64_t n = 0; n < P.n_owned; n++) {
    const int64_t len = P.bptr[n + 1] - P.bptr[n];
    for (int a = 0; a < nv; a++) {
      const int64_t r = n * nv + a;
      row_ptr[r + 1] = row_ptr[r] + len * nv;
      int32_t* o = col_idx + row_ptr[r];
      for (int64_t k = 0; k < len; k++)
        for (int b = 0; b < nv; b++) *o++ = P.bcol[P.bptr[n] + k] * nv + b;
    }
  }
  return RDC_OK;
}

int rdc_mesh_colours_download(const rdc_ctx* c, int32_t* colour) {
  if (!c || !c->ms.have_mesh) return RDC_ERR_STATE;
  if (!colour) return RDC_ERR_INVALID;
  std::memcpy(colour, c->ms.prep.colour.data(), sizeof(int32_t) * (size_t)c->ms.prep.n_elem);
  return RDC_OK;
}

int rdc_field_device_ptr(rdc_ctx* c, int field, int64_t count, double** d_ptr) {
  if (!c || !d_ptr) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (field < 0 || field >= RDC_FIELD_COUNT) return fail(c, RDC_ERR_INVALID, "unknown field %d", field);
  if (count != field_expected(c, field))
    return fail(c, RDC_ERR_INVALID, "field %d needs %lld values, got %lld", field, (long long)field_expected(c, field), (long long)count);
  int rc = set_device(c);
  if (rc) return rc;
  DevBuf& b = c->buf.field[field];
  if (!b.p || !b.owned || c->ms.field_count[field] != count) {
    if (b.p && !b.owned) b = DevBuf();
    if ((rc = dev_alloc(c, b, (size_t)count * sizeof(double)))) return rc;
    c->ms.field_count[field] = count;
  }
  *d_ptr = (double*)b.p;
  return RDC_OK;
}

int rdc_field_upload(rdc_ctx* c, int field, const double* host, int64_t count) {
  if (!c) return RDC_ERR_INVALID;
  if (!host) return fail(c, RDC_ERR_INVALID, "null host pointer");
  double* d = nullptr;
  int rc = rdc_field_device_ptr(c, field, count, &d);
  if (rc) return rc;
  RDC_HIP(c, hipMemcpyAsync(d, host, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  return RDC_OK;
}

int rdc_field_download(rdc_ctx* c, int field, double* host, int64_t count) {
  if (!c) return RDC_ERR_INVALID;
  if (!host) return fail(c, RDC_ERR_INVALID, "null host pointer");
  if (field < 0 || field >= RDC_FIELD_COUNT || !c->buf.field[field].p) return fail(c, RDC_ERR_STATE, "field %d not set", field);
  if (count != c->ms.field_count[field]) return fail(c, RDC_ERR_INVALID, "field %d holds %lld values", field, (long long)c->ms.field_count[field]);
  int rc = set_device(c);
  if (rc) return rc;
  RDC_HIP(c, hipMemcpyAsync(host, c->buf.field[field].p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  return RDC_OK;
}

int rdc_field_bind_device(rdc_ctx* c, int field, double* d_ptr, int64_t count) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (field < 0 || field >= RDC_FIELD_COUNT) return fail(c, RDC_ERR_INVALID, "unknown field %d", field);
  if (!d_ptr) return fail(c, RDC_ERR_INVALID, "null device pointer");
  if (count != field_expected(c, field))
    return fail(c, RDC_ERR_INVALID, "field %d needs %lld values, got %lld", field, (long long)field_expected(c, field), (long long)count);
  int rc = dev_free(c, c->buf.field[field]);
  if (rc) return rc;
  c->buf.field[field].p = d_ptr;
  c->buf.field[field].bytes = (size_t)count * sizeof(double);
  c->buf.field[field].owned = false;
  c->ms.field_count[field] = count;
  return RDC_OK;
}

int rdc_solid_set_materials(rdc_ctx* c, const int32_t* elem_material, int32_t n_materials,
                            const rdc_solid_material* materials) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (!elem_material || !materials || n_materials <= 0) return fail(c, RDC_ERR_INVALID, "bad material table");
  for (int64_t e = 0; e < c->ms.prep.n_elem; e++)
    if (elem_material[e] < 0 || elem_material[e] >= n_materials) return fail(c, RDC_ERR_INVALID, "material index out of range at element %lld", (long long)e);
  int rc = set_device(c);
  if (rc) return rc;
  std::vector<int32_t> em(elem_material, elem_material + c->ms.prep.n_elem);
  std::vector<rdc_solid_material> mt(materials, materials + n_materials);
  if ((rc = dev_upload(c, c->buf.solid_in.elem_material, em))) return rc;
  if ((rc = dev_upload(c, c->buf.solid_in.materials, mt))) return rc;
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  c->ms.n_materials = n_materials;
  return RDC_OK;
}

int rdc_solid_set_sides(rdc_ctx* c, int64_t n_sides, const int64_t* side_elem, const int32_t* side_id,
                        const double* side_disp) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (n_sides < 0 || (n_sides > 0 && (!side_elem || !side_id || !side_disp))) return fail(c, RDC_ERR_INVALID, "bad side list");
  const int nsides_elem = c->ms.prep.nen == 4 ? 4 : 6;
  for (int64_t s = 0; s < n_sides; s++) {
    if (side_elem[s] < 0 || side_elem[s] >= c->ms.prep.n_elem) return fail(c, RDC_ERR_INVALID, "side %lld: element out of range", (long long)s);
    if (side_id[s] < 0 || side_id[s] >= nsides_elem) return fail(c, RDC_ERR_INVALID, "side %lld: side id out of range", (long long)s);
  }
  int rc = set_device(c);
  if (rc) return rc;
  std::vector<int64_t> se(side_elem, side_elem + n_sides);
  std::vector<int32_t> si(side_id, side_id + n_sides);
  std::vector<double> sd(side_disp, side_disp + 3 * n_sides);
  if ((rc = dev_upload(c, c->buf.solid_in.side_elem, se))) return rc;
  if ((rc = dev_upload(c, c->buf.solid_in.side_id, si))) return rc;
  if ((rc = dev_upload(c, c->buf.solid_in.side_disp, sd))) return rc;
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  c->ms.n_sides = n_sides;
  return RDC_OK;
}

int rdc_assemble_pihna(rdc_ctx* c, const rdc_pihna_params* p) { return assemble_rd<Pihna>(c, p, 5, false); }
int rdc_assemble_ripf(rdc_ctx* c, const rdc_ripf_params* p) { return assemble_rd<Ripf>(c, p, 3, true); }
int rdc_assemble_hcc(rdc_ctx* c, const rdc_hcc_params* p) { return assemble_rd<Hcc>(c, p, 3, false); }
int rdc_assemble_adpm(rdc_ctx* c, const rdc_adpm_params* p) { return assemble_rd<Adpm>(c, p, 3, false); }
int rdc_assemble_proteas(rdc_ctx* c, const rdc_proteas_params* p) { return assemble_rd<Proteas>(c, p, 5, true); }

int rdc_assemble_pihna_part(rdc_ctx* c, const rdc_pihna_params* p, int part, void* stream) {
  return with_part(c, part, stream, [&] { return assemble_rd<Pihna>(c, p, 5, false); });
}
int rdc_assemble_hcc_part(rdc_ctx* c, const rdc_hcc_params* p, int part, void* stream) {
  return with_part(c, part, stream, [&] { return assemble_rd<Hcc>(c, p, 3, false); });
}
int rdc_solid_assemble_part(rdc_ctx* c, const rdc_solid_params* p, int request_jacobian, int part, void* stream) {
  return with_part(c, part, stream, [&] { return rdc_solid_assemble(c, p, request_jacobian); });
}

int rdc_solid_assemble(rdc_ctx* c, const rdc_solid_params* p, int request_jacobian) {
  if (!c) return RDC_ERR_INVALID;
  if (!p) return fail(c, RDC_ERR_INVALID, "null parameter struct");
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "assemble called before rdc_mesh_upload");
  c->tet4_cl_active = 0;
  c->const_rows.other_assembly();
  if (c->ms.prep.nvar != 3) return fail(c, RDC_ERR_INVALID, "solid system needs nvar=3");
  if (!c->buf.field[RDC_FIELD_UNDEFORMED_XYZ].p) return fail(c, RDC_ERR_STATE, "undeformed coordinates not set");
  if (!c->buf.field[RDC_FIELD_ELEM_FIBRE].p) return fail(c, RDC_ERR_STATE, "fibre field not set");
  if (c->ms.n_materials <= 0) return fail(c, RDC_ERR_STATE, "materials not set");
  int rc = set_device(c);
  if (rc) return rc;
  SolidArgs a;
  a.m = mesh_view(c);
  a.nen = c->ms.prep.nen;
  a.Xu = (const double*)c->buf.field[RDC_FIELD_UNDEFORMED_XYZ].p;
  a.fibre = (const double*)c->buf.field[RDC_FIELD_ELEM_FIBRE].p;
  a.elem_material = (const int32_t*)c->buf.solid_in.elem_material.p;
  a.materials = (const rdc_solid_material*)c->buf.solid_in.materials.p;
  a.n_sides = c->ms.n_sides;
  a.side_elem = (const int64_t*)c->buf.solid_in.side_elem.p;
  a.side_id = (const int32_t*)c->buf.solid_in.side_id.p;
  a.side_disp = (const double*)c->buf.solid_in.side_disp.p;
  a.params = *p;
  a.request_jacobian = request_jacobian;
  a.val = (double*)c->buf.out.val.p;
  a.rhs = (double*)c->buf.out.rhs.p;
  a.stream = c->stream;
  a.colour_ptr = c->ms.prep.colour_ptr.data();
  a.n_colours = c->ms.prep.n_colours;
  a.opt = c->opt;
  a.nblocks = c->ms.prep.bptr[(size_t)c->ms.prep.n_owned];
  // kernel choice: the fused cluster kernel serves HEX8 tangent requests; everything else is two-pass (or coloured on request)
  int kernel = c->opt.solid_kernel == 1 ? 1 : 0;
  if ((c->opt.solid_kernel == 0 || c->opt.solid_kernel == 3) && c->ms.prep.nen == 8 && request_jacobian) {
    if ((rc = ensure_cluster_lists(c, 1))) return rc;
    if (c->ms.cl.state != 1 && c->opt.solid_kernel == 3) return fail(c, RDC_ERR_UNSUPPORTED, "fused solid kernel: %s", c->err);
    if (c->ms.cl.state == 1) {
      kernel = 3;
      a.cl = cluster_view(c, c->ms.cl.interior >= 0 ? c->opt.part : (c->opt.part == 1 ? 1 : 0));
    }
  } else if (c->opt.solid_kernel == 3) {
    return fail(c, RDC_ERR_UNSUPPORTED, "fused solid kernel: HEX8 tangent requests only");
  }
  // two-part assembly (halo overlap): the fused cluster kernel launches the clusters of interior nodes in part 1 and the rest
  // (+ the penalty sides, which add into rows of both kinds) in part 2; the two-pass and coloured forms assemble everything in part 2
  if (c->opt.part == 1) {
    c->ms.part1_nodes = 0;
    if (kernel != 3 || c->ms.cl.interior < 0 || a.cl.n_wg == 0) return RDC_OK;
    c->ms.part1_nodes = c->ms.cl.part1.nodes;
    a.n_sides = 0;
    if (!c->solid_part1_event) RDC_HIP(c, hipEventCreateWithFlags(&c->solid_part1_event, hipEventDisableTiming));
    a.done_record = c->solid_part1_event;
    c->ms.solid_part1_pending = true;
  } else if (c->opt.part == 2 && c->ms.solid_part1_pending) {
    a.sides_wait = c->solid_part1_event;
    c->ms.solid_part1_pending = false;
  } else {
    c->ms.solid_part1_pending = false;
  }
  a.kernel = kernel;
  if (a.kernel == 0) {
    if (!c->ms.solid_gather_ready) {  // one-time: gather lists and the element-matrix buffers
      SolidGather g;
      const std::string err = solid_gather_build(c->ms.prep, g);
      if (!err.empty()) return fail(c, RDC_ERR_UNSUPPORTED, "%s", err.c_str());
      if ((rc = dev_upload(c, c->buf.two_pass.gptr, g.gptr))) return rc;
      if ((rc = dev_upload(c, c->buf.two_pass.gsrc, g.gsrc))) return rc;
      if ((rc = dev_upload(c, c->buf.two_pass.brow, g.brow))) return rc;
      const size_t rows = (size_t)c->ms.prep.n_elem * c->ms.prep.nen;
      if ((rc = dev_alloc(c, c->buf.two_pass.ke, rows * c->ms.prep.nen * 9 * sizeof(double)))) return rc;
      if ((rc = dev_alloc(c, c->buf.two_pass.fe, rows * 3 * sizeof(double)))) return rc;
      RDC_HIP(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
      c->ms.solid_gather_ready = true;
    }
    a.ke = (double*)c->buf.two_pass.ke.p;
    a.fe = (double*)c->buf.two_pass.fe.p;
    a.gptr = (const uint32_t*)c->buf.two_pass.gptr.p;
    a.gsrc = (const uint32_t*)c->buf.two_pass.gsrc.p;
    a.brow = (const int32_t*)c->buf.two_pass.brow.p;
  } else {
    a.ke = a.fe = nullptr;
    a.gptr = a.gsrc = nullptr;
    a.brow = nullptr;
  }
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  if (a.sides_wait) {   // part 2 starts behind part 1 (its penalty sides add into rows of both parts); in a step it follows the halo exchange anyway
    RDC_HIP(c, hipStreamWaitEvent(c->stream, a.sides_wait, 0));
    a.sides_wait = nullptr;
  }
  if (c->timing) {
    if ((rc = next_event_pair(c, &ev_start, &ev_stop))) return rc;
    RDC_HIP(c, hipEventRecord(ev_start, c->stream));
  }
  hipError_t e = launch_solid(a);
  if (e != hipSuccess) return fail(c, RDC_ERR_HIP, "solid kernel launch failed: %s", hipGetErrorString(e));
  if (c->timing) RDC_HIP(c, hipEventRecord(ev_stop, c->stream));
  return RDC_OK;
}

int rdc_csr_values_device_ptr(rdc_ctx* c, double** d_val, double** d_rhs) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (d_val) { *d_val = (double*)c->buf.out.val.p; c->const_rows.values_pointer(); }   // ... or write the values
  if (d_rhs) *d_rhs = (double*)c->buf.out.rhs.p;
  return RDC_OK;
}

int rdc_csr_download(rdc_ctx* c, double* val, double* rhs) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  int rc = set_device(c);
  if (rc) return rc;
  const size_t nnz = (size_t)c->ms.prep.nvar * c->ms.prep.nvar * c->ms.prep.bptr[c->ms.prep.n_owned];
  if (val) RDC_HIP(c, hipMemcpyAsync(val, c->buf.out.val.p, nnz * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (rhs) RDC_HIP(c, hipMemcpyAsync(rhs, c->buf.out.rhs.p, (size_t)c->ms.prep.n_owned * c->ms.prep.nvar * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  return RDC_OK;
}

int rdc_csr_download_rows(rdc_ctx* c, int64_t node_begin, int64_t node_end, double* val, double* rhs, int async) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (node_begin < 0 || node_end < node_begin || node_end > c->ms.prep.n_owned) return fail(c, RDC_ERR_INVALID, "bad node range");
  int rc = set_device(c);
  if (rc) return rc;
  const int64_t nv = c->ms.prep.nvar;
  const int64_t v0 = nv * nv * c->ms.prep.bptr[(size_t)node_begin], v1 = nv * nv * c->ms.prep.bptr[(size_t)node_end];
  if (val && v1 > v0)
    RDC_HIP(c, hipMemcpyAsync(val + v0, (const double*)c->buf.out.val.p + v0, (size_t)(v1 - v0) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (rhs && node_end > node_begin)
    RDC_HIP(c, hipMemcpyAsync(rhs + node_begin * nv, (const double*)c->buf.out.rhs.p + node_begin * nv,
                              (size_t)((node_end - node_begin) * nv) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (!async) RDC_HIP(c, hipStreamSynchronize(c->stream));
  return RDC_OK;
}

int rdc_csr_download_rows_async(rdc_ctx* c, int64_t node_begin, int64_t node_end, double* val, double* rhs, int* ticket) {
  if (!c || !ticket) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (node_begin < 0 || node_end < node_begin || node_end > c->ms.prep.n_owned) return fail(c, RDC_ERR_INVALID, "bad node range");
  int rc = set_device(c);
  if (rc) return rc;
  if (!c->copy_stream) RDC_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  if (!c->copy_fence) RDC_HIP(c, hipEventCreateWithFlags(&c->copy_fence, hipEventDisableTiming));
  const int t = c->next_ticket;
  c->next_ticket = (t + 1) % rdc_ctx::N_TICKETS;
  if (!c->ticket[t]) RDC_HIP(c, hipEventCreateWithFlags(&c->ticket[t], hipEventDisableTiming | hipEventBlockingSync));
  else RDC_HIP(c, hipEventSynchronize(c->ticket[t]));   // the slot's previous copy (16 calls ago) has certainly been consumed
  // the rows must be complete in what has been enqueued on the context's stream so far; work enqueued later (part 2) is not waited for
  RDC_HIP(c, hipEventRecord(c->copy_fence, c->stream));
  RDC_HIP(c, hipStreamWaitEvent(c->copy_stream, c->copy_fence, 0));
  const int64_t nv = c->ms.prep.nvar;
  const int64_t v0 = nv * nv * c->ms.prep.bptr[(size_t)node_begin], v1 = nv * nv * c->ms.prep.bptr[(size_t)node_end];
  if (val && v1 > v0)
    RDC_HIP(c, hipMemcpyAsync(val + v0, (const double*)c->buf.out.val.p + v0, (size_t)(v1 - v0) * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
  if (rhs && node_end > node_begin)
    RDC_HIP(c, hipMemcpyAsync(rhs + node_begin * nv, (const double*)c->buf.out.rhs.p + node_begin * nv,
                              (size_t)((node_end - node_begin) * nv) * sizeof(double), hipMemcpyDeviceToHost, c->copy_stream));
  RDC_HIP(c, hipEventRecord(c->ticket[t], c->copy_stream));
  *ticket = t;
  return RDC_OK;
}

int rdc_ticket_wait(rdc_ctx* c, int ticket) {
  if (!c || ticket < 0 || ticket >= rdc_ctx::N_TICKETS || !c->ticket[ticket]) return c ? fail(c, RDC_ERR_INVALID, "no such ticket") : RDC_ERR_INVALID;
  int rc = set_device(c);
  if (rc) return rc;
  RDC_HIP(c, hipEventSynchronize(c->ticket[ticket]));
  return RDC_OK;
}

int rdc_host_pin(rdc_ctx* c, void* p, size_t bytes) {
  if (!c || !p) return RDC_ERR_INVALID;
  int rc = set_device(c);
  if (rc) return rc;
  RDC_HIP(c, hipHostRegister(p, bytes, hipHostRegisterDefault));
  return RDC_OK;
}

int rdc_host_unpin(rdc_ctx* c, void* p) {
  if (!c || !p) return RDC_ERR_INVALID;
  RDC_HIP(c, hipHostUnregister(p));
  return RDC_OK;
}

int rdc_part1_nodes(const rdc_ctx* c, int64_t* n_nodes) {
  if (!c || !n_nodes) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh) return RDC_ERR_STATE;
  *n_nodes = 0;
  // after a part-1 call: what THAT call completed (the kernel path depends on the model, the parameter values and the
  // tuning options, and the paths split the rows differently)
  if (c->ms.part1_nodes >= 0) { *n_nodes = c->ms.part1_nodes; return RDC_OK; }
  // before any part-1 call: what part 1 of a shipped-pattern PIHNA call would complete with the current options and the lists
  // that exist now (nothing is built here): the same decision as the call's
  if (c->opt.interior_nodes < 0) return RDC_OK;
  Facts f = path_facts(c, strategy_of(c));
  f.opt.part = 1;
  f.pattern = true;
  f.cl_fits = tet4_cl_lds_bytes<Pihna>(c->ms.cl.max_row_doubles) <= c->max_lds;
  PartSplit s;
  switch (path_decide(describe<Pihna>(), f).two_part) {
    case TwoPart::EV_SPLIT: s = split_ev(c->ms.prep_ev.desc, c->opt.interior_nodes); break;
    case TwoPart::CL_SPLIT: s = c->ms.cl.part1; break;
    case TwoPart::PAIR_SPLIT: s = part1_pairs(c); break;
    case TwoPart::WHOLE: case TwoPart::ALL_IN_PART2: break;
  }
  *n_nodes = s.wg > 0 ? s.nodes : 0;
  return RDC_OK;
}

int rdc_tet4_cluster_mode(rdc_ctx* c, int mode) {
  if (!c) return RDC_ERR_INVALID;
  if (mode < 0 || mode > 2) return fail(c, RDC_ERR_INVALID, "tet4 cluster mode must be 0 (off), 1 (meshes without pair lists) or 2 (every TET4 mesh), not %d", mode);
  c->tet4_cl_mode = mode;
  return RDC_OK;
}

int rdc_tet4_cluster_info(rdc_ctx* c, int32_t* mode, int32_t* active, int64_t* n_clusters, int64_t* n_pairs,
                          int64_t* n_elem_visits, int64_t* lds_bytes) {
  if (!c) return RDC_ERR_INVALID;
  const MeshState::ClusterLists& L = c->ms.cl;
  const bool lists = c->ms.have_mesh && c->ms.prep.nen == 4 && L.state == 1;
  if (mode) *mode = c->tet4_cl_mode;
  if (active) *active = c->tet4_cl_active;
  if (n_clusters) *n_clusters = lists ? L.n_wg : 0;
  if (n_pairs) *n_pairs = lists ? L.n_pairs : 0;
  if (n_elem_visits) *n_elem_visits = lists ? L.n_elem_visits : 0;
  if (lds_bytes) *lds_bytes = c->tet4_cl_active ? (int64_t)c->tet4_cl_lds : 0;
  return RDC_OK;
}

int rdc_clamp_nonnegative(rdc_ctx* c, int field) {
  if (!c) return RDC_ERR_INVALID;
  if (field < 0 || field >= RDC_FIELD_COUNT || !c->buf.field[field].p) return fail(c, RDC_ERR_STATE, "field %d not set", field);
  int rc = set_device(c);
  if (rc) return rc;
  const int64_t n = c->ms.field_count[field];
  if (n > 0) {
    int64_t grid = (n + 255) / 256;
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(k_clamp_nonnegative, dim3((unsigned)grid), dim3(256), 0, c->stream, (double*)c->buf.field[field].p, n);
    RDC_HIP(c, hipGetLastError());
  }
  return RDC_OK;
}

int rdc_pihna_volume_integrals(rdc_ctx* c, const rdc_pihna_ranges* r, int64_t n_elem, double* out4) {
  if (!c) return RDC_ERR_INVALID;
  if (!r || !out4) return fail(c, RDC_ERR_INVALID, "null argument");
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (c->ms.prep.nvar != 5) return fail(c, RDC_ERR_INVALID, "PIHNA volume integrals need nvar=5");
  if (!c->buf.field[RDC_FIELD_OLD_SOLUTION].p) return fail(c, RDC_ERR_STATE, "solution field not set");
  if (n_elem < 0) n_elem = c->ms.prep.n_elem;
  if (n_elem > c->ms.prep.n_elem) return fail(c, RDC_ERR_INVALID, "n_elem exceeds the mesh");
  int rc = set_device(c);
  if (rc) return rc;
  int64_t grid = (n_elem + 255) / 256;
  if (grid > 1024) grid = 1024;
  if (grid < 1) grid = 1;
  if ((rc = dev_alloc(c, c->buf.scratch.wg_max, (size_t)grid * 4 * sizeof(double)))) return rc;
  const MeshDev m = mesh_view(c);
  if (c->ms.prep.nen == 4)
    hipLaunchKernelGGL((k_pihna_volumes<4>), dim3((unsigned)grid), dim3(256), 0, c->stream, m, n_elem,
                       (const double*)c->buf.field[RDC_FIELD_OLD_SOLUTION].p, *r, (double*)c->buf.scratch.wg_max.p);
  else
    hipLaunchKernelGGL((k_pihna_volumes<8>), dim3((unsigned)grid), dim3(256), 0, c->stream, m, n_elem,
                       (const double*)c->buf.field[RDC_FIELD_OLD_SOLUTION].p, *r, (double*)c->buf.scratch.wg_max.p);
  RDC_HIP(c, hipGetLastError());
  std::vector<double> h((size_t)grid * 4);
  RDC_HIP(c, hipMemcpyAsync(h.data(), c->buf.scratch.wg_max.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  for (int x = 0; x < 4; x++) {
    double s = 0.0;
    for (int64_t g = 0; g < grid; g++) s += h[(size_t)g * 4 + x];
    out4[x] = s;
  }
  return RDC_OK;
}

int rdc_ripf_volume_integrals(rdc_ctx* c, const rdc_ripf_ranges* r, int64_t n_elem, double* out2) {
  if (!c) return RDC_ERR_INVALID;
  if (!r || !out2) return fail(c, RDC_ERR_INVALID, "null argument");
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (c->ms.prep.nvar != 3) return fail(c, RDC_ERR_INVALID, "RIPF volume integrals need nvar=3");
  if (!c->buf.field[RDC_FIELD_OLD_SOLUTION].p) return fail(c, RDC_ERR_STATE, "solution field not set");
  if (n_elem < 0) n_elem = c->ms.prep.n_elem;
  if (n_elem > c->ms.prep.n_elem) return fail(c, RDC_ERR_INVALID, "n_elem exceeds the mesh");
  int rc = set_device(c);
  if (rc) return rc;
  int64_t grid = (n_elem + 255) / 256;
  if (grid > 1024) grid = 1024;
  if (grid < 1) grid = 1;
  if ((rc = dev_alloc(c, c->buf.scratch.wg_max, (size_t)grid * 2 * sizeof(double)))) return rc;
  const MeshDev m = mesh_view(c);
  if (c->ms.prep.nen == 4)
    hipLaunchKernelGGL((k_ripf_volumes<4>), dim3((unsigned)grid), dim3(256), 0, c->stream, m, n_elem,
                       (const double*)c->buf.field[RDC_FIELD_OLD_SOLUTION].p, *r, (double*)c->buf.scratch.wg_max.p);
  else
    hipLaunchKernelGGL((k_ripf_volumes<8>), dim3((unsigned)grid), dim3(256), 0, c->stream, m, n_elem,
                       (const double*)c->buf.field[RDC_FIELD_OLD_SOLUTION].p, *r, (double*)c->buf.scratch.wg_max.p);
  RDC_HIP(c, hipGetLastError());
  std::vector<double> h((size_t)grid * 2);
  RDC_HIP(c, hipMemcpyAsync(h.data(), c->buf.scratch.wg_max.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  for (int x = 0; x < 2; x++) {
    double s = 0.0;
    for (int64_t g = 0; g < grid; g++) s += h[(size_t)g * 2 + x];
    out2[x] = s;
  }
  return RDC_OK;
}

int rdc_adpm_parcellation_integrals(rdc_ctx* c, const rdc_adpm_ranges* r, const int32_t* elem_subdomain,
                                    const int32_t* ids, int32_t n_ids, int64_t n_elem, double* out,
                                    int64_t* last_elem) {
  if (!c) return RDC_ERR_INVALID;
  if (!r || !elem_subdomain || !ids || !out) return fail(c, RDC_ERR_INVALID, "null argument");
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (c->ms.prep.nvar != 3) return fail(c, RDC_ERR_INVALID, "ADPM parcellation integrals need nvar=3");
  if (!c->buf.field[RDC_FIELD_OLD_SOLUTION].p) return fail(c, RDC_ERR_STATE, "solution field not set");
  if (n_ids <= 0 || n_ids > 2048) return fail(c, RDC_ERR_INVALID, "n_ids must be in [1, 2048]");
  for (int32_t i = 1; i < n_ids; i++)
    if (ids[i] <= ids[i - 1]) return fail(c, RDC_ERR_INVALID, "parcellation ids must be strictly ascending");
  if (n_elem < 0) n_elem = c->ms.prep.n_elem;
  if (n_elem > c->ms.prep.n_elem) return fail(c, RDC_ERR_INVALID, "n_elem exceeds the mesh");
  int rc = set_device(c);
  if (rc) return rc;
  // region slot of every element; the last element of each region carries bit 30
  std::vector<int32_t> slot((size_t)(n_elem > 0 ? n_elem : 1), -1);
  std::vector<int64_t> last((size_t)n_ids, -1);
  for (int64_t e = 0; e < n_elem; e++) {
    const int32_t* it = std::lower_bound(ids, ids + n_ids, elem_subdomain[e]);
    if (it == ids + n_ids || *it != elem_subdomain[e]) continue;
    slot[(size_t)e] = (int32_t)(it - ids);
    last[(size_t)(it - ids)] = e;
  }
  for (int32_t i = 0; i < n_ids; i++)
    if (last[(size_t)i] >= 0) slot[(size_t)last[(size_t)i]] |= 0x40000000;
  int64_t grid = (n_elem + 255) / 256;
  if (grid > 256) grid = 256;
  if (grid < 1) grid = 1;
  const size_t n_part = (size_t)grid * 2 * n_ids;
  if ((rc = dev_alloc(c, c->buf.scratch.wg_max, (n_part + 2 * (size_t)n_ids) * sizeof(double)))) return rc;
  if ((rc = dev_upload(c, c->buf.scratch.adpm_slot, slot))) return rc;
  double* part = (double*)c->buf.scratch.wg_max.p;
  double* conc = part + n_part;
  RDC_HIP(c, hipMemsetAsync(conc, 0, 2 * (size_t)n_ids * sizeof(double), c->stream));
  const MeshDev m = mesh_view(c);
  const size_t lds = 2 * (size_t)n_ids * sizeof(double);
  if (c->ms.prep.nen == 4)
    hipLaunchKernelGGL((k_adpm_parcellation<4>), dim3((unsigned)grid), dim3(256), lds, c->stream, m, n_elem,
                       (const double*)c->buf.field[RDC_FIELD_OLD_SOLUTION].p, *r, (const int32_t*)c->buf.scratch.adpm_slot.p, (int)n_ids, part, conc);
  else
    hipLaunchKernelGGL((k_adpm_parcellation<8>), dim3((unsigned)grid), dim3(256), lds, c->stream, m, n_elem,
                       (const double*)c->buf.field[RDC_FIELD_OLD_SOLUTION].p, *r, (const int32_t*)c->buf.scratch.adpm_slot.p, (int)n_ids, part, conc);
  RDC_HIP(c, hipGetLastError());
  std::vector<double> h(n_part + 2 * (size_t)n_ids);
  RDC_HIP(c, hipMemcpyAsync(h.data(), c->buf.scratch.wg_max.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  for (int32_t i = 0; i < n_ids; i++) {
    double sa = 0.0, st = 0.0;
    for (int64_t g = 0; g < grid; g++) {
      sa += h[(size_t)g * 2 * n_ids + 2 * i];
      st += h[(size_t)g * 2 * n_ids + 2 * i + 1];
    }
    out[4 * i] = h[n_part + 2 * i];
    out[4 * i + 1] = h[n_part + 2 * i + 1];
    out[4 * i + 2] = sa;
    out[4 * i + 3] = st;
    if (last_elem) last_elem[i] = last[(size_t)i];
  }
  return RDC_OK;
}

int rdc_solid_post_process(rdc_ctx* c, const rdc_solid_params* p, double* pressure, double* von_mises,
                           double* fibre_current) {
  if (!c) return RDC_ERR_INVALID;
  if (!p) return fail(c, RDC_ERR_INVALID, "null parameter struct");
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (c->ms.prep.nvar != 3) return fail(c, RDC_ERR_INVALID, "solid system needs nvar=3");
  if (!c->buf.field[RDC_FIELD_UNDEFORMED_XYZ].p) return fail(c, RDC_ERR_STATE, "undeformed coordinates not set");
  if (!c->buf.field[RDC_FIELD_ELEM_FIBRE].p) return fail(c, RDC_ERR_STATE, "fibre field not set");
  if (c->ms.n_materials <= 0) return fail(c, RDC_ERR_STATE, "materials not set");
  int rc = set_device(c);
  if (rc) return rc;
  const size_t ne = (size_t)c->ms.prep.n_elem;
  if ((rc = dev_alloc(c, c->buf.scratch.solid_post, ne * 5 * sizeof(double)))) return rc;
  SolidArgs a{};
  a.m = mesh_view(c);
  a.nen = c->ms.prep.nen;
  a.Xu = (const double*)c->buf.field[RDC_FIELD_UNDEFORMED_XYZ].p;
  a.fibre = (const double*)c->buf.field[RDC_FIELD_ELEM_FIBRE].p;
  a.elem_material = (const int32_t*)c->buf.solid_in.elem_material.p;
  a.materials = (const rdc_solid_material*)c->buf.solid_in.materials.p;
  a.params = *p;
  a.stream = c->stream;
  hipError_t e = launch_solid_post(a, (double*)c->buf.scratch.solid_post.p);
  if (e != hipSuccess) return fail(c, RDC_ERR_HIP, "solid post-process launch failed: %s", hipGetErrorString(e));
  std::vector<double> h(ne * 5);
  RDC_HIP(c, hipMemcpyAsync(h.data(), c->buf.scratch.solid_post.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  for (size_t e2 = 0; e2 < ne; e2++) {
    if (pressure) pressure[e2] = h[5 * e2];
    if (von_mises) von_mises[e2] = h[5 * e2 + 1];
    if (fibre_current) { fibre_current[3 * e2] = h[5 * e2 + 2]; fibre_current[3 * e2 + 1] = h[5 * e2 + 3]; fibre_current[3 * e2 + 2] = h[5 * e2 + 4]; }
  }
  return RDC_OK;
}

int rdc_ripf_check_solution(rdc_ctx* c, const rdc_ripf_check_params* p, double* rt_total_max) {
  if (!c) return RDC_ERR_INVALID;
  if (!p) return fail(c, RDC_ERR_INVALID, "null parameter struct");
  if (!c->ms.have_mesh) return fail(c, RDC_ERR_STATE, "no mesh uploaded");
  if (c->ms.prep.nvar != 3) return fail(c, RDC_ERR_INVALID, "RIPF check_solution needs nvar=3");
  if (!(p->time_step > 0.0)) return fail(c, RDC_ERR_INVALID, "time_step must be positive");
  if (p->RT_broad_fractions < 0 || p->RT_focus_fractions < 0) return fail(c, RDC_ERR_INVALID, "negative fraction count");
  const int need[] = {RDC_FIELD_OLD_SOLUTION, RDC_FIELD_PREV_SOLUTION, RDC_FIELD_RT_DOSE};
  const int64_t n = c->ms.prep.n_node;
  for (int f : need)
    if (!c->buf.field[f].p || c->ms.field_count[f] != 3 * n) return fail(c, RDC_ERR_STATE, "field %d not set", f);
  int rc = set_device(c);
  if (rc) return rc;
  for (int f : {RDC_FIELD_TIME_DERIV, RDC_FIELD_AUX_NODAL}) {
    if (c->buf.field[f].p && c->ms.field_count[f] == 3 * n) continue;
    if (c->buf.field[f].p && !c->buf.field[f].owned) return fail(c, RDC_ERR_STATE, "bound field %d has the wrong size", f);
    if ((rc = dev_alloc(c, c->buf.field[f], (size_t)(3 * n) * sizeof(double)))) return rc;
    c->ms.field_count[f] = 3 * n;
  }
  int64_t grid = (n + 255) / 256;
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  if ((rc = dev_alloc(c, c->buf.scratch.wg_max, (size_t)grid * sizeof(double)))) return rc;
  hipLaunchKernelGGL(k_ripf_check, dim3((unsigned)grid), dim3(256), 0, c->stream, n, 1.0 / p->time_step, p->HU_min, p->HU_max,
                     (double)p->RT_broad_fractions, (double)p->RT_focus_fractions, (int)p->day,
                     (double*)c->buf.field[RDC_FIELD_OLD_SOLUTION].p, (double*)c->buf.field[RDC_FIELD_PREV_SOLUTION].p,
                     (double*)c->buf.field[RDC_FIELD_TIME_DERIV].p, (double*)c->buf.field[RDC_FIELD_RT_DOSE].p,
                     (double*)c->buf.field[RDC_FIELD_AUX_NODAL].p, (double*)c->buf.scratch.wg_max.p);
  RDC_HIP(c, hipGetLastError());
  std::vector<double> h((size_t)grid);
  RDC_HIP(c, hipMemcpyAsync(h.data(), c->buf.scratch.wg_max.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  double mx = -1.0;
  for (double v : h) mx = v > mx ? v : mx;
  if (rt_total_max) *rt_total_max = mx;
  return RDC_OK;
}

int rdc_debug_stamps(rdc_ctx* c, long long* host_out, int64_t capacity, int64_t* n_written) {
  if (!c) return RDC_ERR_INVALID;
  if (!c->ms.have_mesh || !c->ms.prep.rg2_ok) return fail(c, RDC_ERR_STATE, "no row-gather work lists");
  int rc = set_device(c);
  if (rc) return rc;
  // "kernel" = 7 with "ablate" = 4: the stamped build of the element-visit kernel, [cluster][wave][12] (rdc_tet4_ev.hip, tools/ev_timeline.py)
  const bool ev_tl = c->opt.kernel == 7 && c->opt.ablate == 4 && c->ms.prep_ev.ok;
  const int64_t n = ev_tl ? (int64_t)c->ms.prep_ev.desc.size() * 4 * 12 : (int64_t)c->ms.prep.wg2.size() * 4 * 9;
  if (!host_out) {  // arm: the next PIHNA (shipped-parameter) assembly runs the stamped diagnostic kernel
    if ((rc = dev_alloc(c, c->buf.scratch.stamps, (size_t)n * sizeof(long long)))) return rc;
    RDC_HIP(c, hipMemsetAsync(c->buf.scratch.stamps.p, 0, (size_t)n * sizeof(long long), c->stream));
    if (n_written) *n_written = n;
    return RDC_OK;
  }
  if (!c->buf.scratch.stamps.p) return fail(c, RDC_ERR_STATE, "stamps not armed");
  const int64_t m = n < capacity ? n : capacity;
  RDC_HIP(c, hipMemcpyAsync(host_out, c->buf.scratch.stamps.p, (size_t)m * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  RDC_HIP(c, hipStreamSynchronize(c->stream));
  if (n_written) *n_written = m;
  dev_free(c, c->buf.scratch.stamps);
  return RDC_OK;
}

int rdc_timing_enable(rdc_ctx* c, int on) {
  if (!c) return RDC_ERR_INVALID;
  c->timing = on != 0;
  c->ev_used = 0;
  return RDC_OK;
}

int rdc_timing_last_ms(rdc_ctx* c, float* ms) {
  if (!c || !ms) return RDC_ERR_INVALID;
  if (c->ev_used < 2) return fail(c, RDC_ERR_STATE, "no timed assemble call recorded");
  int rc = set_device(c);
  if (rc) return rc;
  RDC_HIP(c, hipEventSynchronize(c->ev[c->ev_used - 1]));
  RDC_HIP(c, hipEventElapsedTime(ms, c->ev[c->ev_used - 2], c->ev[c->ev_used - 1]));
  return RDC_OK;
}

int rdc_timing_sum_ms(rdc_ctx* c, float* total_ms, int* n_calls) {
  if (!c || !total_ms || !n_calls) return RDC_ERR_INVALID;
  int rc = set_device(c);
  if (rc) return rc;
  float total = 0.0f;
  for (size_t x = 0; x + 1 < c->ev_used; x += 2) {
    float ms = 0.0f;
    RDC_HIP(c, hipEventSynchronize(c->ev[x + 1]));
    RDC_HIP(c, hipEventElapsedTime(&ms, c->ev[x], c->ev[x + 1]));
    total += ms;
  }
  *total_ms = total;
  *n_calls = (int)(c->ev_used / 2);
  c->ev_used = 0;
  return RDC_OK;
}

int rdc_timing_samples_ms(rdc_ctx* c, float* out, int capacity, int* n_calls) {
  if (!c || !out || !n_calls || capacity < 0) return RDC_ERR_INVALID;
  int rc = set_device(c);
  if (rc) return rc;
  int n = 0;
  for (size_t x = 0; x + 1 < c->ev_used; x += 2, n++) {
    float ms = 0.0f;
    RDC_HIP(c, hipEventSynchronize(c->ev[x + 1]));
    RDC_HIP(c, hipEventElapsedTime(&ms, c->ev[x], c->ev[x + 1]));
    if (n < capacity) out[n] = ms;
  }
  *n_calls = n;
  c->ev_used = 0;
  return RDC_OK;
}

}  // extern "C"
