// g++ build of what the rank-local Gauss-Seidel smoother across ranks (RDC_PRECOND_MULTIGRID_GS_LOCAL) adds on the host, for
// tests/test_host_solve_mg_gs_dist.py: mg_colour on every level of every rank's partitioned hierarchy, the interior split of
// colour 0 (mg_gs_interior) and the placement of the lists (mg_gs_place).  The hierarchies are those host_solve_mg_dist_shim.cpp
// builds rank by rank, whose text is taken in whole: its entry points drive the coarsening here too.
#include "host_solve_mg_dist_shim.cpp"

namespace {
std::vector<std::vector<rdc::MgColours>> g_rank_cols;   // [rank][level]
}  // namespace

extern "C" {

// colours every level of rank r as gs_upload does (level 0: the rank's rows, below: the steps); returns the number of levels,
// -(2 + l) if mg_colour refuses level l
int shim_gsd_colour(int r) {
  RankState* S = rank_of(r);
  if (!S || S->halos.empty()) return -1;
  if (g_rank_cols.size() < g_ranks.size()) g_rank_cols.resize(g_ranks.size());
  std::vector<rdc::MgColours> cols(S->steps.size() + 1);
  for (size_t l = 0; l < cols.size(); l++) {
    const bool ok = l == 0 ? rdc::mg_colour(S->halos[0].n_owned, S->bptr0.data(), S->bcol0.data(), cols[0])
                           : rdc::mg_colour(S->steps[l - 1].n, S->steps[l - 1].bptr.data(), S->steps[l - 1].bcol.data(), cols[l]);
    if (!ok) return -(2 + (int)l);
  }
  g_rank_cols[(size_t)r] = std::move(cols);
  return (int)g_rank_cols[(size_t)r].size();
}

// list `which` of level `level` of rank r (0 colour, 1 cptr, 2 nodes)
int64_t shim_gsd_list(int r, int level, int which, void* out) {
  if (r < 0 || r >= (int)g_rank_cols.size() || level < 0 || level >= (int)g_rank_cols[(size_t)r].size()) return -1;
  const rdc::MgColours& C = g_rank_cols[(size_t)r][(size_t)level];
  switch (which) {
    case 0: return give(C.colour, out);
    case 1: return give(C.cptr, out);
    case 2: return give(C.nodes, out);
  }
  return -1;
}

// the nodes of colour 0 of level 0 of rank r below n_int
int64_t shim_gsd_interior(int r, int64_t n_int) {
  if (r < 0 || r >= (int)g_rank_cols.size() || g_rank_cols[(size_t)r].empty()) return -1;
  return rdc::mg_gs_interior(g_rank_cols[(size_t)r][0], n_int);
}

// Places the lists of rank r into an arena of EXACTLY the measured bytes, allocated here, and compares what arrived: returns the
// bytes, -2 if the two passes disagree, -3 if a list did not arrive where the level says, -4 if a list is not aligned.
int64_t shim_gsd_place(int r, int32_t* n_colours) {
  if (r < 0 || r >= (int)g_rank_cols.size()) return -1;
  const std::vector<rdc::MgColours>& cols = g_rank_cols[(size_t)r];
  rdc::MgArena a;
  rdc::MgGsDev g;
  rdc::mg_gs_place(cols, a, g, [](void*, const void*, size_t) {});
  const size_t bytes = a.used;
  std::vector<char> arena(bytes);
  a = rdc::MgArena{arena.data()};
  rdc::mg_gs_place(cols, a, g, [](void* at, const void* list, size_t n) { std::memcpy(at, list, n); });
  if (a.used != bytes || g.n_levels != (int)cols.size()) return -2;
  for (int l = 0; l < g.n_levels; l++) {
    const rdc::MgColours& C = cols[(size_t)l];
    n_colours[l] = g.lv[l].n_colours;
    if (g.lv[l].cptr_host != C.cptr.data() || g.lv[l].n_colours != C.n_colours()) return -3;
    if (((const char*)g.lv[l].nodes - arena.data()) % rdc::MG_ALIGN || ((const char*)g.lv[l].cptr - arena.data()) % rdc::MG_ALIGN) return -4;
    if (!C.nodes.empty() && std::memcmp(g.lv[l].nodes, C.nodes.data(), C.nodes.size() * sizeof(int32_t))) return -3;
    if (std::memcmp(g.lv[l].cptr, C.cptr.data(), C.cptr.size() * sizeof(int64_t))) return -3;
  }
  return (int64_t)bytes;
}

}
