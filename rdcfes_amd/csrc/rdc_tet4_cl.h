// rdc_tet4_cl.h — TET4 reaction-diffusion assembly on node clusters (all five models: PIHNA src/pihna.C:383-756, RIPF
// src/ripf.C:410-671, coupled HCC src/coupled_hcc.C:463-646, ADPM src/adpm.C:370-528, PROTEAS src/proteas.C:338-705) for
// the meshes whose rows are too long for the pair lists and the element-visit lists (more than 16 node blocks: every
// Gmsh / Delaunay mesh).
//
// k_tet4_rowgather and k_rowgather<M, 4> gather the four node records of every (node, element) pair from global memory
// through wg_node_ptr -> node_pair_ptr -> pair_elem -> conn -> records.  Here, on the cluster lists of rdc_prep_cl.cpp
// built with nen = 4 (cll::tet4_limits):
//   * a workgroup owns a cluster of <= 16 owned nodes grown over the mesh graph (locality does not depend on the numbering);
//   * STAGE: one lane per element touching the cluster gathers its four nodes once (tet4_cl_gather) into an ELEMENT
//     RECORD in LDS: the cluster's nodes are fetched once per element visit, not once per pair;
//   * ROWS: one lane per pair reads its element's record in the rotated order of the pair kernels (column j = local node
//     j ^ i), evaluates tet4_row0 and adds into an LDS image of the cluster's CSR rows (tet4_cl_pair);
//   * COPY-OUT: the image leaves in runs, every CSR value exactly once (cll::copy_out).
// The gather and the per-pair function are host + device so that the CPU suite replays the kernel from the same lists
// (tests/host_tet4_cl_shim.cpp).
#ifndef RDC_TET4_CL_H
#define RDC_TET4_CL_H
#include "rdc_prep.h"
#include "rdc_tet4_fast.h"

namespace rdc {

// element record: per local node n (original order) its coordinates, unknowns and aux values
template <class M>
struct Tet4ClRec {
  static constexpr int NA = (M::NAUX > 0 ? M::NAUX : 0);
  static constexpr int NODE = 3 + M::NV + NA, N = 4 * NODE;
  static constexpr int STRIDE = N | 1;   // odd: the records of 32 consecutive elements start in 32 different double-banks
};

// dynamic LDS of the kernel (doubles): [image + rhs entries of the largest cluster | max_elems element records]
template <class M>
constexpr size_t tet4_cl_rec_offset(size_t max_row_doubles) {
  return (size_t)cll::zero_doubles((int)max_row_doubles, M::NV * cll::tet4_limits(M::NV).max_nodes);
}
template <class M>
constexpr size_t tet4_cl_lds_bytes(size_t max_row_doubles) {
  return sizeof(double) * (tet4_cl_rec_offset<M>(max_row_doubles) + (size_t)cll::tet4_limits(M::NV).max_elems * Tet4ClRec<M>::STRIDE);
}

// block (a, b) of the model is structurally non-zero: the others stay the zeros of the image
template <class M>
RDC_HD constexpr bool tet4_cl_block(int a, int b) {
  bool nz = M::hasA(a, b) || M::hasD(a, b);
  for (int g = 0; g < M::NG; g++) nz = nz || M::hasB(a, b, g);
  return nz;
}

// record of element e from the mesh and the nodal fields (aux: read only when the model has aux values)
template <class M>
RDC_HD void tet4_cl_gather(const uint32_t* conn, uint32_t e, const double* xyz, const double* u, const double* aux,
                           double (&r)[Tet4ClRec<M>::N]) {
  using R = Tet4ClRec<M>;
#pragma unroll
  for (int n = 0; n < 4; n++) {
    const int64_t I = conn[(int64_t)e * 4 + n];
#pragma unroll
    for (int c = 0; c < 3; c++) r[n * R::NODE + c] = xyz[3 * I + c];
#pragma unroll
    for (int v = 0; v < M::NV; v++) r[n * R::NODE + 3 + v] = u[M::NV * I + v];
#pragma unroll
    for (int v = 0; v < R::NA; v++) r[n * R::NODE + 3 + M::NV + v] = aux[(int64_t)R::NA * I + v];
  }
}

// one addition into the image: the lanes of a workgroup on the device, one thread on the host
RDC_HD void tet4_cl_add(double* p, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  *p += v;
#endif
}

// sink of tet4_row0: j is the ROTATED column; off[j] = NV * slot of that column in the row of the pair's node
template <class M>
struct Tet4ClSink {
  double* row;    // image segment of the pair's node (HostPrepCl::Node::off)
  double* lrhs;   // rhs entries of the pair's node
  int stride;     // NV * len: doubles between equation rows
  int off[4];
  RDC_HD void ke(int a, int b, int j, double v) {
    if (!tet4_cl_block<M>(a, b)) return;
    tet4_cl_add(row + a * stride + off[j] + b, v);
  }
  RDC_HD void fe(int a, double v) { tet4_cl_add(lrhs + a, v); }
};

// The pair (element record `rec`, local row node li): its NV rows added into the image segment `seg` (len node blocks per
// row) at the column slots `slots` (cll::pslot_get, byte j = slot of ORIGINAL local node j), its rhs entries into lrhs.
// Models that read the aux values at one local node only (PROTEAS, AUX_LOCAL_NODE) see zeros in the other columns, as
// k_tet4_rg5 and k_tet4_coloured give them.  ED: the element's M::NELEM per-element inputs
template <class M, int EXP_MODE>
RDC_HD void tet4_cl_pair(const typename M::K& k, const double* rec, int li, uint32_t slots, double* seg, int len, double* lrhs,
                         const double* ED) {
  constexpr int NV = M::NV, NA = (M::NAUX > 0 ? M::NAUX : 1);
  using R = Tet4ClRec<M>;
  double X[4][3], U[4][NV], AX[4][NA];
  Tet4ClSink<M> sink;
  sink.row = seg;
  sink.lrhs = lrhs;
  sink.stride = NV * len;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int jo = j ^ li;   // original local index of rotated column j
    const double* r = rec + jo * R::NODE;
#pragma unroll
    for (int c = 0; c < 3; c++) X[j][c] = r[c];
#pragma unroll
    for (int v = 0; v < NV; v++) U[j][v] = r[3 + v];
#pragma unroll
    for (int v = 0; v < NA; v++)
      AX[j][v] = (M::NAUX > 0 && (M::AUX_LOCAL_NODE < 0 || jo == M::AUX_LOCAL_NODE)) ? r[3 + NV + (M::NAUX > 0 ? v : 0)] : 0.0;
    sink.off[j] = NV * cll::pslot_get(&slots, jo);
  }
  tet4_row0<M, EXP_MODE>(k, X, U, AX, sink, ED);
}

}  // namespace rdc
#endif
