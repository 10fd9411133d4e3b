// rdc_parts.h — two-part assembly ("part" = 1: the interior rows, 2: the rest): how the pair lists and the element-visit lists divide
// for a given "interior_nodes".  Host only (no HIP): the CPU suite compiles it with g++ (tests/host_shim.cpp).
#ifndef RDC_PARTS_H
#define RDC_PARTS_H
#include <algorithm>
#include "rdc_path.h"
#include "rdc_prep.h"

namespace rdc {

// The first wg work items of the family's launch order are interior; rows [0, nodes) are complete once they have run.
struct PartSplit { int wg = 0; int64_t nodes = 0; };

// Pair lists (HostPrep::wg2): a work item owns the nodes [n0, n0 + nnodes) and the ranges ascend, so the interior items are the
// leading ones that end at or below `interior`
inline PartSplit split_pairs(const std::vector<HostPrep::WgDesc>& wg2, int64_t interior) {
  auto end = [&](int w) { return (int64_t)wg2[(size_t)w].n0 + wg2[(size_t)w].nnodes; };
  int lo = 0, hi = (int)wg2.size();
  while (lo < hi) {
    const int mid = (lo + hi) / 2;
    if (end(mid) <= interior) lo = mid + 1; else hi = mid;
  }
  return {lo, lo > 0 ? end(lo - 1) : 0};
}

// Element-visit lists (HostPrepEv::desc): clusters are not node ranges.  Interior = every node of the cluster is below `interior`;
// the launch order (perm, if wanted) has those first, each kind in list order.  The rows of [0, n) are complete after them when
// no other cluster owns a node below n.
inline PartSplit split_ev(const std::vector<HostPrepEv::Desc>& desc, int64_t interior, std::vector<uint32_t>* perm = nullptr) {
  PartSplit s{0, std::max<int64_t>(interior, 0)};
  std::vector<uint32_t> rest;
  if (perm) perm->clear();
  for (size_t w = 0; w < desc.size(); w++) {
    const bool in = (int64_t)desc[w].max_node < interior;
    if (in) s.wg++; else s.nodes = std::min<int64_t>(s.nodes, (int64_t)desc[w].min_node);
    if (perm) (in ? *perm : rest).push_back((uint32_t)w);
  }
  if (perm) perm->insert(perm->end(), rest.begin(), rest.end());
  return s;
}

// What the kernel-path decision (rdc_path.h) reads of a mesh's lists as they stand: the element type and the pair, row-gather and
// element-visit lists.  The cluster-list facts are the caller's: they depend on the options the lists were built with
inline void list_facts(const HostPrep& P, const HostPrepEv& E, Facts& f) {
  f.nen = P.nen;
  f.rowgather_ok = P.rowgather_ok && P.wg_node_ptr.size() > 1;
  f.rg2_ok = P.rg2_ok && P.nen == 4;
  f.rg2_block = P.rg2_block;
  f.pair_aux = f.rg2_ok;
  f.nlist = f.rg2_ok && P.nl_stride > 0;
  f.pair_eid = !P.pair_eid.empty();
  f.ev_ok = E.ok;
}

}  // namespace rdc
#endif
