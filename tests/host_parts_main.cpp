// Stand-alone driver of rdcfes_amd/csrc/rdc_parts.h for a sanitizer build (tools/asan_parts.sh): the splits of the pair lists and
// of the element-visit lists of a K(6) mesh for "interior_nodes" below, inside and beyond the owned nodes, with lists that
// respect the value and lists that do not, each against a linear restatement.  Prints "ok" and returns 0.
#include <algorithm>
#include <cstdio>

#include "../rdcfes_amd/csrc/rdc_parts.h"

using namespace rdc;

int main() {
  const int n = 6, m = n + 1;
  std::vector<uint32_t> conn;   // Kuhn: six tetrahedra per cube, one per order of the three axes
  const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++)
      for (int k = 0; k < n; k++)
        for (const auto& pm : perms) {
          int at[3] = {i, j, k};
          conn.push_back((uint32_t)((at[0] * m + at[1]) * m + at[2]));
          for (int s = 0; s < 3; s++) { at[pm[s]]++; conn.push_back((uint32_t)((at[0] * m + at[1]) * m + at[2])); }
        }
  const int64_t n_node = (int64_t)m * m * m, n_elem = (int64_t)conn.size() / 4;
  HostPrep P;
  std::string err = prep_build(4, n_elem, n_node, n_node, conn.data(), 5, 60 * 1024, 256, P);
  if (!err.empty() || !P.rg2_ok) { std::printf("prep_build: %s\n", err.c_str()); return 1; }
  int checked = 0;
  for (const int64_t interior : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)(0.37 * n_node), n_node - 1, n_node, n_node + 5}) {
    const PartSplit sp = split_pairs(P.wg2, interior);
    int wg = 0;
    while (wg < (int)P.wg2.size() && (int64_t)P.wg2[(size_t)wg].n0 + P.wg2[(size_t)wg].nnodes <= interior) wg++;
    if (sp.wg != wg || sp.nodes != (wg ? (int64_t)P.wg2[(size_t)wg - 1].n0 + P.wg2[(size_t)wg - 1].nnodes : 0)) return 2;
    for (const int64_t built_with : {(int64_t)-1, interior <= n_node ? interior : (int64_t)-1}) {
      HostPrepEv E;
      err = prep_build_ev(P, conn.data(), 54000, E, built_with);
      if (!err.empty()) { std::printf("prep_build_ev: %s\n", err.c_str()); return 3; }
      std::vector<uint32_t> perm(3, 7u);   // not empty: the split replaces what it finds
      const PartSplit se = split_ev(E.desc, interior, &perm);
      const PartSplit se2 = split_ev(E.desc, interior);
      if (se.wg != se2.wg || se.nodes != se2.nodes || perm.size() != E.desc.size()) return 4;
      int64_t bound = std::max<int64_t>(interior, 0);
      for (size_t x = 0; x < perm.size(); x++) {
        if (perm[x] >= E.desc.size()) return 5;
        const HostPrepEv::Desc& d = E.desc[perm[x]];
        const bool in = (int64_t)d.max_node < interior;
        if (in != ((int)x < se.wg)) return 6;
        if (x > 0 && x != (size_t)se.wg && perm[x] <= perm[x - 1]) return 7;   // each kind in list order
        if (!in) bound = std::min<int64_t>(bound, (int64_t)d.min_node);
      }
      if (se.nodes != bound) return 8;
      checked++;
    }
  }
  if (split_pairs({}, 5).wg != 0 || split_pairs({}, 5).nodes != 0 || split_ev({}, 5).wg != 0 || split_ev({}, 5).nodes != 5) return 11;   // no lists
  std::printf("ok: %d splits of %zu pair work items and their element-visit clusters\n", checked, P.wg2.size());
  return 0;
}
