// CPU build of the TET4 cluster kernel's host + device parts (rdcfes_amd/csrc/rdc_tet4_cl.h) for tests/test_host_tet4_cl.py:
// the cluster lists built with cll::tet4_limits and checked against the mesh, and k_tet4_cl replayed from those lists with
// the SAME record gather and per-pair function the kernel compiles (tet4_cl_gather, tet4_cl_pair), into an image laid out as
// the kernel's (Node::off, rhs entries behind it) and copied out per node.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../rdcfes_amd/csrc/rdc_prep.h"
#include "../rdcfes_amd/csrc/rdc_tet4_cl.h"
#include "../rdcfes_amd/csrc/rdc_tet4_pihna_moments.h"

using namespace rdc;

namespace {
HostPrep g_prep;
HostPrepCl g_cl;
std::vector<uint32_t> g_conn;
std::string g_err;
int64_t g_interior = -1;

template <class M, class P>
int replay(const P* p, const double* xyz, const double* u, const double* aux, const double* elem, double* val, double* rhs) {
  constexpr int NV = M::NV;
  using R = Tet4ClRec<M>;
  if (!g_cl.ok || g_prep.nen != 4 || g_prep.nvar != NV) return 1;
  if ((M::NAUX > 0 && !aux) || (M::NELEM > 0 && !elem)) return 4;
  const typename M::K k = M::derive(*p);
  const bool fastexp = exp_mode_of(M::exponent(k)) == M::FAST_EXP_MODE;
  const HostPrepCl& C = g_cl;
  const cll::Strides S = cll::strides(C.lim, 4);
  const size_t rec_off = tet4_cl_rec_offset<M>(C.max_row_doubles);
  std::vector<double> lds(tet4_cl_lds_bytes<M>(C.max_row_doubles) / sizeof(double));
  for (size_t w = 0; w < C.desc.size(); w++) {
    const HostPrepCl::Desc& d = C.desc[w];
    std::fill(lds.begin(), lds.end(), std::nan(""));   // what the kernel does not write it must not read
    double* img = lds.data();
    double* lrhs = img + cll::rhs_offset((int)d.row_doubles);
    double* recs = lds.data() + rec_off;
    if ((size_t)cll::zero_doubles((int)d.row_doubles, NV * d.nown) > rec_off) return 5;   // the image reaches into the records
    for (int x = 0; x < cll::zero_doubles((int)d.row_doubles, NV * d.nown); x++) img[x] = 0.0;
    for (int le = 0; le < d.nelem; le++) {
      double r[R::N];
      tet4_cl_gather<M>(g_conn.data(), C.eid[w * S.elem + le], xyz, u, aux, r);
      std::copy(r, r + R::N, recs + (size_t)le * R::STRIDE);
    }
    for (int x = 0; x < d.npair; x++) {
      const uint32_t pw = C.pair[w * S.pair + x];
      const int le = cll::pair_elem(pw), li = cll::pair_row(pw), na = cll::pair_node(pw);
      const HostPrepCl::Node& nd = C.ntab[w * S.node + na];
      const double* ED = M::NELEM > 0 ? elem + (size_t)C.eid[w * S.elem + le] * M::NELEM : nullptr;
      const uint32_t slots = C.pslot[w * S.pslot + x];
      if (fastexp) tet4_cl_pair<M, M::FAST_EXP_MODE>(k, recs + (size_t)le * R::STRIDE, li, slots, img + nd.off, nd.len, lrhs + NV * na, ED);
      else tet4_cl_pair<M, 0>(k, recs + (size_t)le * R::STRIDE, li, slots, img + nd.off, nd.len, lrhs + NV * na, ED);
    }
    for (int a = 0; a < d.nown; a++) {
      const HostPrepCl::Node& nd = C.ntab[w * S.node + a];
      for (int x = 0; x < NV * NV * (int)nd.len; x++) val[(size_t)NV * NV * nd.bptr + x] = img[nd.off + x];
      for (int v = 0; v < NV; v++) rhs[(size_t)NV * nd.node + v] = lrhs[NV * a + v];
    }
  }
  return 0;
}
}  // namespace

extern "C" {

const char* t4_error() { return g_err.c_str(); }

// out4 = cll::tet4_limits(nvar): max_nodes, max_pairs, max_elems, max_row_doubles
void t4_limits(int nvar, int* out4) {
  const HostPrepCl::Limits lim = cll::tet4_limits(nvar);
  out4[0] = lim.max_nodes; out4[1] = lim.max_pairs; out4[2] = lim.max_elems; out4[3] = lim.max_row_doubles;
}

// The lists of a TET4 mesh with cll::tet4_limits(nvar) (pair_order as given; n_interior >= 0: "interior_nodes"), checked against
// the mesh: every owned node in exactly one cluster, every (owned node, element) pair listed once with the local element, local row
// node, node index and column slots (== eslot) of the mesh, the node table, the limits.  0 = ok, 1 = the builder refused
// (t4_error says why), > 1 = a check failed.  stats[8] = clusters, element visits, pairs, largest image (doubles), owned nodes
// covered, largest cluster, longest row (node blocks), node blocks of the owned rows
int t4_build(int64_t n_elem, int64_t n_node, int64_t n_owned, const uint32_t* conn, int nvar, int64_t n_interior, int pair_order, int64_t* stats) {
  g_cl = HostPrepCl();
  g_interior = n_interior;
  g_err = prep_build(4, n_elem, n_node, n_owned, conn, nvar, (size_t)50 * 1024, 256, g_prep);
  if (!g_err.empty()) return 1;
  g_conn.assign(conn, conn + n_elem * 4);
  HostPrepCl::Limits lim = cll::tet4_limits(nvar);
  lim.pair_order = pair_order;
  g_err = prep_build_cl(g_prep, g_conn.data(), lim, g_cl, n_interior);
  if (!g_err.empty()) return 1;
  const HostPrepCl& C = g_cl;
  const int nv2 = nvar * nvar;
  const cll::Strides S = cll::strides(lim, 4);
  std::vector<int32_t> npairs_of((size_t)n_owned, 0), seen((size_t)n_owned, 0);
  int64_t covered = 0, largest = 0, longest = 0;
  for (size_t w = 0; w < C.desc.size(); w++) {
    const HostPrepCl::Desc& d = C.desc[w];
    if (d.nown < 1 || d.nown > lim.max_nodes || d.npair > lim.max_pairs || d.nelem > lim.max_elems || (int)d.row_doubles > lim.max_row_doubles) { g_err = "limits"; return 2; }
    covered += d.nown;
    largest = std::max<int64_t>(largest, d.nown);
    uint32_t off = 0;
    for (int a = 0; a < d.nown; a++) {
      const HostPrepCl::Node& nd = C.ntab[w * S.node + a];
      if ((int64_t)nd.node >= n_owned || seen[nd.node]++) { g_err = "node listed twice"; return 3; }
      if (cll::seg_phase(off) != cll::seg_phase((uint32_t)(nv2 * g_prep.bptr[nd.node]))) off++;   // the segment has the 16-byte phase of its CSR segment
      if (nd.bptr != (uint32_t)g_prep.bptr[nd.node] || nd.len != g_prep.bptr[nd.node + 1] - g_prep.bptr[nd.node] || nd.off != off) { g_err = "node table"; return 4; }
      off += (uint32_t)(nv2 * nd.len);
      longest = std::max<int64_t>(longest, nd.len);
    }
    if (off != d.row_doubles) { g_err = "row_doubles"; return 5; }
    for (int x = 0; x < lim.max_elems; x++)
      if ((x < d.nelem) != (C.eid[w * S.elem + x] != cll::IDLE) || (x < d.nelem && C.eid[w * S.elem + x] >= (uint32_t)n_elem)) { g_err = "element list"; return 11; }
    for (int x = 0; x < lim.max_pairs; x++) {
      const uint32_t pr = C.pair[w * S.pair + x];
      if (x >= d.npair) { if (pr != cll::IDLE) { g_err = "pair beyond npair"; return 6; } continue; }
      const int le = cll::pair_elem(pr), li = cll::pair_row(pr), a = cll::pair_node(pr);
      if (le >= d.nelem || li >= 4 || a >= d.nown) { g_err = "pair fields"; return 7; }
      const uint32_t e = C.eid[w * S.elem + le];
      const uint32_t n = C.ntab[w * S.node + a].node;
      if (g_conn[(size_t)e * 4 + li] != n) { g_err = "pair does not match the mesh"; return 8; }
      for (int j = 0; j < 4; j++) {
        const int s = cll::pslot_get(&C.pslot[w * S.pslot + (size_t)x * cll::pslot_words(4)], j);
        if (s != (int)g_prep.eslot[(size_t)e * 16 + li * 4 + j] || s >= C.ntab[w * S.node + a].len) { g_err = "slot"; return 9; }
      }
      npairs_of[n]++;
    }
  }
  std::vector<int32_t> inc((size_t)n_owned, 0);
  for (size_t x = 0; x < g_conn.size(); x++) if ((int64_t)g_conn[x] < n_owned) inc[g_conn[x]]++;
  for (int64_t n = 0; n < n_owned; n++)
    if (inc[n] != npairs_of[n] || seen[n] != 1) { g_err = "pair coverage"; return 10; }
  stats[0] = (int64_t)C.desc.size(); stats[1] = C.n_elem_visits; stats[2] = C.n_pairs; stats[3] = (int64_t)C.max_row_doubles;
  stats[4] = covered; stats[5] = largest; stats[6] = longest; stats[7] = g_prep.bptr[(size_t)n_owned];
  return 0;
}

// two-part assembly: out[3] = leading clusters of interior nodes, rows complete after them, clusters mixing the two kinds;
// non-zero: the interior clusters are not exactly the leading ones (1) or a row below the bound belongs to a later cluster (2)
int t4_interior(int64_t* out) {
  const HostPrepCl& C = g_cl;
  out[0] = C.n_wg_interior; out[1] = C.part1_nodes; out[2] = 0;
  const size_t max_nodes = cll::strides(C.lim, 4).node;
  for (size_t w = 0; w < C.desc.size(); w++) {
    int n_in = 0;
    for (int a = 0; a < C.desc[w].nown; a++) n_in += (int64_t)C.ntab[w * max_nodes + a].node < g_interior;
    const bool interior = n_in == C.desc[w].nown;
    if (n_in != 0 && !interior) out[2]++;
    if (interior != ((int64_t)w < C.n_wg_interior)) return 1;
    if (!interior)
      for (int a = 0; a < C.desc[w].nown; a++) if ((int64_t)C.ntab[w * max_nodes + a].node < C.part1_nodes) return 2;
  }
  return 0;
}

// dynamic LDS (bytes) of the kernel for the last lists: 3 unknowns without / with aux values, 5 without / with
void t4_lds_bytes(int64_t* out4) {
  out4[0] = (int64_t)tet4_cl_lds_bytes<Hcc>(g_cl.max_row_doubles); out4[1] = (int64_t)tet4_cl_lds_bytes<Ripf>(g_cl.max_row_doubles);
  out4[2] = (int64_t)tet4_cl_lds_bytes<Pihna>(g_cl.max_row_doubles); out4[3] = (int64_t)tet4_cl_lds_bytes<Proteas>(g_cl.max_row_doubles);
}

// k_tet4_cl replayed from the lists of the last t4_build.  model: 0 PIHNA, 1 RIPF, 2 HCC, 4 ADPM, 5 PROTEAS, and the
// instantiations the context picks for the shipped parameter patterns: 3 PIHNA cell transport off, 6 the same in moment form,
// 7 RIPF reduced, 8 HCC mass only, 9 ADPM decay only (3 = they do not apply to these parameters)
int t4_assemble(int model, const void* params, const double* xyz, const double* u, const double* aux, const double* elem, double* val, double* rhs) {
  switch (model) {
    case 0: return replay<Pihna>((const rdc_pihna_params*)params, xyz, u, aux, elem, val, rhs);
    case 1: return replay<Ripf>((const rdc_ripf_params*)params, xyz, u, aux, elem, val, rhs);
    case 2: return replay<Hcc>((const rdc_hcc_params*)params, xyz, u, aux, elem, val, rhs);
    case 4: return replay<Adpm>((const rdc_adpm_params*)params, xyz, u, aux, elem, val, rhs);
    case 5: return replay<Proteas>((const rdc_proteas_params*)params, xyz, u, aux, elem, val, rhs);
    case 3: if (!PihnaNoCellTransport::applies(*(const rdc_pihna_params*)params)) return 3;
            return replay<PihnaNoCellTransport>((const rdc_pihna_params*)params, xyz, u, aux, elem, val, rhs);
    case 6: if (!PihnaNoCellTransport::applies(*(const rdc_pihna_params*)params)) return 3;
            return replay<PihnaNoCellTransportMoments>((const rdc_pihna_params*)params, xyz, u, aux, elem, val, rhs);
    case 7: if (!RipfReduced::applies(*(const rdc_ripf_params*)params)) return 3;
            return replay<RipfReduced>((const rdc_ripf_params*)params, xyz, u, aux, elem, val, rhs);
    case 8: if (!HccMassOnly::applies(*(const rdc_hcc_params*)params)) return 3;
            return replay<HccMassOnly>((const rdc_hcc_params*)params, xyz, u, aux, elem, val, rhs);
    case 9: if (!AdpmDecayOnly::applies(*(const rdc_adpm_params*)params)) return 3;
            return replay<AdpmDecayOnly>((const rdc_adpm_params*)params, xyz, u, aux, elem, val, rhs);
  }
  return 2;
}

}  // extern "C"
