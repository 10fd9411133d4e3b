// Stand-alone run of what the rank-local Gauss-Seidel smoother across ranks (RDC_PRECOND_MULTIGRID_GS_LOCAL) adds on the host, for
// tools/asan_solve_mg_gs_dist.sh: no device, no Python.  The worlds, their split into ranks and the collective build are those of
// host_solve_mg_dist_main.cpp, whose text is taken in whole (its main under another name); here every level of every rank's
// ghosted hierarchy is coloured (mg_colour), the colouring checked against the rows, the interior split of colour 0 taken for every
// bound (mg_gs_interior), and the lists placed (mg_gs_place) into a heap buffer of exactly the measured size, so that the
// sanitizer sees every write.  One world has a rank that owns nothing.  Returns 0 if all of it holds.
#define main host_solve_mg_dist_main
#include "host_solve_mg_dist_main.cpp"
#undef main

namespace {

// 31: refused; 32: not proper or not a partition of the nodes; 33: a list does not ascend; 34: the split; 35 .. 37: the placement
int check_colours(const Rank& R) {
  std::vector<rdc::MgColours> cols(R.steps.size() + 1);
  for (size_t l = 0; l < cols.size(); l++) {
    const int64_t n = l ? R.steps[l - 1].n : R.halos[0].n_owned;
    const int64_t* bptr = l ? R.steps[l - 1].bptr.data() : R.bptr.data();
    const int32_t* bcol = l ? R.steps[l - 1].bcol.data() : R.bcol.data();
    rdc::MgColours& C = cols[l];
    if (!rdc::mg_colour(n, bptr, bcol, C)) return 31;
    if ((int64_t)C.colour.size() != n || (int64_t)C.nodes.size() != n || C.cptr.empty() || C.cptr.back() != n) return 32;
    if (n == 0 && C.n_colours() != 0) return 32;
    for (int64_t i = 0; i < n; i++)
      for (int64_t k = bptr[i]; k < bptr[i + 1]; k++)
        if (bcol[k] != i && bcol[k] < n && C.colour[(size_t)bcol[k]] == C.colour[(size_t)i]) return 32;
    for (int c = 0; c < C.n_colours(); c++)
      for (int64_t at = C.cptr[(size_t)c]; at < C.cptr[(size_t)c + 1]; at++) {
        if (C.colour[(size_t)C.nodes[(size_t)at]] != c) return 32;
        if (at > C.cptr[(size_t)c] && C.nodes[(size_t)at - 1] >= C.nodes[(size_t)at]) return 33;
      }
  }
  const int64_t n0 = R.halos[0].n_owned;
  for (int64_t n_int = 0; n_int <= n0 + 1; n_int++) {
    const int64_t k = rdc::mg_gs_interior(cols[0], n_int);
    const int64_t len = cols[0].n_colours() ? cols[0].cptr[1] : 0;
    if (k < 0 || k > len) return 34;
    for (int64_t at = 0; at < len; at++)
      if ((cols[0].nodes[(size_t)at] < n_int) != (at < k)) return 34;
  }
  rdc::MgArena a;
  rdc::MgGsDev g;
  rdc::mg_gs_place(cols, a, g, [](void*, const void*, size_t) {});
  const size_t bytes = a.used;
  if (bytes % rdc::MG_ALIGN) return 35;
  char* buf = bytes ? (char*)std::malloc(bytes) : nullptr;   // exactly the measured bytes: a write past them is caught
  a = rdc::MgArena{buf};
  rdc::mg_gs_place(cols, a, g, [](void* at, const void* list, size_t n) { std::memcpy(at, list, n); });
  int rc = a.used != bytes || g.n_levels != (int)cols.size() ? 36 : 0;
  for (int l = 0; l < g.n_levels && !rc; l++) {
    const rdc::MgColours& C = cols[(size_t)l];
    if (g.lv[l].n_colours != C.n_colours() || g.lv[l].cptr_host != C.cptr.data()) rc = 36;
    else if (buf && std::memcmp(g.lv[l].cptr, C.cptr.data(), C.cptr.size() * sizeof(int64_t))) rc = 37;
    else if (buf && !C.nodes.empty() && std::memcmp(g.lv[l].nodes, C.nodes.data(), C.nodes.size() * sizeof(int32_t))) rc = 37;
  }
  std::free(buf);
  return rc;
}

int check_world(const char* name, const std::vector<std::vector<int32_t>>& adj, const std::vector<int>& owner, int world) {
  std::vector<Rank> W = split(adj, owner, world);
  if (int rc = build(W)) return rc;
  std::printf("%s, %d ranks, colours per rank and level:", name, world);
  for (const Rank& R : W) {
    if (int rc = check_colours(R)) return rc;
    std::printf(" [");
    for (size_t l = 0; l <= R.steps.size(); l++) {
      rdc::MgColours C;
      rdc::mg_colour(l ? R.steps[l - 1].n : R.halos[0].n_owned, l ? R.steps[l - 1].bptr.data() : R.bptr.data(),
                     l ? R.steps[l - 1].bcol.data() : R.bcol.data(), C);
      std::printf("%s%d", l ? " " : "", C.n_colours());
    }
    std::printf("]");
  }
  std::printf("\n");
  return 0;
}

}  // namespace

int main() {
  int rc;
  const auto g = grid(9, 8, 8);
  for (int world : {1, 2, 3}) {
    std::vector<int> owner(g.size());
    for (size_t i = 0; i < g.size(); i++) owner[i] = (int)(i / 64) * world / 9;
    if ((rc = check_world("grid 9 x 8 x 8", g, owner, world))) return 40 * world + rc;
  }
  {   // three ranks, the last of which owns nothing
    std::vector<int> owner(g.size());
    for (size_t i = 0; i < g.size(); i++) owner[i] = (int)(i / 64) * 2 / 9;
    if ((rc = check_world("grid 9 x 8 x 8, rank 2 empty", g, owner, 3))) return 160 + rc;
  }
  auto u = grid(5, 10, 1);      // rank 1: ten nodes coupled to one node of rank 0 each and to nothing else
  std::vector<int> owner(60, 0);
  for (int i = 0; i < 10; i++) { u.push_back({(int32_t)i}); u[(size_t)i].push_back(50 + i); owner[(size_t)(50 + i)] = 1; }
  if ((rc = check_world("grid 5 x 10 and 10 unconnected nodes", u, owner, 2))) return 200 + rc;
  return 0;
}
