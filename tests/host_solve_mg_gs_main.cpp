// Stand-alone run of the colouring of the Gauss-Seidel smoother (rdcfes_amd/csrc/rdc_solve.h: mg_colour, mg_gs_place) for
// tools/asan_solve_mg_gs.sh: no device, no Python.  Patterns: a 7-point grid graph, a hub (one node coupled to all others), a
// chain, isolated nodes, one node, and the grid with one block removed on one side.  Returns 0 if every level of every hierarchy
// has a proper colouring with ascending lists and the placement fits what it measured: a host buffer of exactly the measured
// size stands in for the allocation and every list is copied into its slot, so the sanitizer sees each write.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {

struct Graph { std::vector<int64_t> bptr; std::vector<int32_t> bcol; };

Graph from_adjacency(std::vector<std::vector<int32_t>> adj) {
  Graph g;
  g.bptr.push_back(0);
  for (size_t i = 0; i < adj.size(); i++) {
    adj[i].push_back((int32_t)i);
    std::sort(adj[i].begin(), adj[i].end());
    adj[i].erase(std::unique(adj[i].begin(), adj[i].end()), adj[i].end());
    g.bcol.insert(g.bcol.end(), adj[i].begin(), adj[i].end());
    g.bptr.push_back((int64_t)g.bcol.size());
  }
  return g;
}

std::vector<std::vector<int32_t>> grid_adjacency(int n) {
  std::vector<std::vector<int32_t>> adj((size_t)n * n * n);
  auto id = [n](int i, int j, int k) { return (int32_t)((i * n + j) * n + k); };
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++)
      for (int k = 0; k < n; k++) {
        if (i + 1 < n) { adj[id(i, j, k)].push_back(id(i + 1, j, k)); adj[id(i + 1, j, k)].push_back(id(i, j, k)); }
        if (j + 1 < n) { adj[id(i, j, k)].push_back(id(i, j + 1, k)); adj[id(i, j + 1, k)].push_back(id(i, j, k)); }
        if (k + 1 < n) { adj[id(i, j, k)].push_back(id(i, j, k + 1)); adj[id(i, j, k + 1)].push_back(id(i, j, k)); }
      }
  return adj;
}

Graph hub(int n) {
  std::vector<std::vector<int32_t>> adj((size_t)n);
  for (int i = 0; i < n; i++)
    if (i != n / 2) { adj[(size_t)i].push_back(n / 2); adj[(size_t)(n / 2)].push_back(i); }
  return from_adjacency(adj);
}

Graph chain(int n, int step) {   // step > n: no edges at all
  std::vector<std::vector<int32_t>> adj((size_t)n);
  for (int i = 0; i + step < n; i += step) { adj[(size_t)i].push_back(i + step); adj[(size_t)(i + step)].push_back(i); }
  return from_adjacency(adj);
}

// 2: a list has the wrong size; 3: a colour is out of range; 4: a colour is empty or its list is not its nodes in ascending order;
// 5: two coupled nodes share a colour; 6: more colours than the longest row has blocks
int check_colours(int64_t n, const int64_t* bptr, const int32_t* bcol, const rdc::MgColours& C) {
  const int nc = C.n_colours();
  if ((int64_t)C.colour.size() != n || (int64_t)C.nodes.size() != n || C.cptr.empty() || C.cptr[0] != 0 || C.cptr.back() != n) return 2;
  int64_t longest = 0;
  for (int64_t i = 0; i < n; i++) {
    if (C.colour[(size_t)i] < 0 || C.colour[(size_t)i] >= nc) return 3;
    longest = std::max(longest, bptr[i + 1] - bptr[i]);
    for (int64_t k = bptr[i]; k < bptr[i + 1]; k++)
      if (bcol[k] != i && C.colour[(size_t)bcol[k]] == C.colour[(size_t)i]) return 5;
  }
  for (int c = 0; c < nc; c++) {
    if (C.cptr[(size_t)c + 1] <= C.cptr[(size_t)c]) return 4;
    for (int64_t at = C.cptr[(size_t)c]; at < C.cptr[(size_t)c + 1]; at++)
      if (C.colour[(size_t)C.nodes[(size_t)at]] != c || (at > C.cptr[(size_t)c] && C.nodes[(size_t)at] <= C.nodes[(size_t)at - 1])) return 4;
  }
  return nc > longest ? 6 : 0;
}

// 10: the two passes disagree, or the measure pass set a pointer; 11: an array is not aligned; 12: it leaves the allocation; 13: two
// arrays overlap, or a list did not arrive where its level points
int check_layout(const std::vector<rdc::MgColours>& cols) {
  rdc::MgArena a;
  rdc::MgGsDev g;
  rdc::mg_gs_place(cols, a, g, [](void*, const void*, size_t) {});
  const size_t bytes = a.used;
  if (bytes % rdc::MG_ALIGN || bytes == 0 || g.n_levels != (int)cols.size() || g.lv[0].nodes || g.lv[0].cptr) return 10;
  char* buf = (char*)std::aligned_alloc(rdc::MG_ALIGN, bytes);
  a = rdc::MgArena{buf};
  rdc::mg_gs_place(cols, a, g, [](void* at, const void* list, size_t n) { std::memcpy(at, list, n); });
  int rc = a.used != bytes ? 10 : 0;
  struct Span { const char* at; size_t bytes; };
  std::vector<Span> spans;
  for (size_t l = 0; l < cols.size() && !rc; l++) {
    const rdc::MgGsLevel& L = g.lv[l];
    if (L.n_colours != cols[l].n_colours() || L.cptr_host != cols[l].cptr.data()) rc = 10;
    spans.push_back({(const char*)L.nodes, cols[l].nodes.size() * sizeof(int32_t)});
    spans.push_back({(const char*)L.cptr, cols[l].cptr.size() * sizeof(int64_t)});
  }
  for (const Span& s : spans) {
    if (rc) break;
    if (!s.at || (size_t)(s.at - buf) % rdc::MG_ALIGN) rc = 11;
    else if (s.at < buf || s.at + s.bytes > buf + bytes) rc = 12;
  }
  std::sort(spans.begin(), spans.end(), [](const Span& x, const Span& y) { return x.at < y.at; });
  for (size_t i = 1; i < spans.size() && !rc; i++)
    if (spans[i - 1].at + spans[i - 1].bytes > spans[i].at) rc = 13;
  for (size_t l = 0; l < cols.size() && !rc; l++)
    if (std::memcmp(g.lv[l].nodes, cols[l].nodes.data(), cols[l].nodes.size() * 4) || std::memcmp(g.lv[l].cptr, cols[l].cptr.data(), cols[l].cptr.size() * 8)) rc = 13;
  std::free(buf);
  return rc;
}

int check(const char* name, const Graph& g) {
  std::vector<rdc::MgLevelHost> steps;
  int64_t n = (int64_t)g.bptr.size() - 1;
  if (!rdc::mg_build(n, g.bptr.data(), g.bcol.data(), steps)) return 1;
  std::vector<rdc::MgColours> cols(steps.size() + 1);
  const int64_t* bptr = g.bptr.data();
  const int32_t* bcol = g.bcol.data();
  std::printf("%s: colours per level", name);
  for (size_t l = 0; l < cols.size(); l++) {
    if (l) { n = steps[l - 1].n; bptr = steps[l - 1].bptr.data(); bcol = steps[l - 1].bcol.data(); }
    if (!rdc::mg_colour(n, bptr, bcol, cols[l])) return 5;
    if (int rc = check_colours(n, bptr, bcol, cols[l])) return rc;
    std::printf(" %d", cols[l].n_colours());
  }
  std::printf("\n");
  return check_layout(cols);
}

}  // namespace

int main() {
  int rc;
  if ((rc = check("grid 12^3", from_adjacency(grid_adjacency(12))))) return rc;
  if ((rc = check("hub 2000", hub(2000)))) return 20 + rc;
  if ((rc = check("chain 500", chain(500, 1)))) return 40 + rc;
  if ((rc = check("isolated 100", chain(100, 1000)))) return 60 + rc;
  if ((rc = check("one node", chain(1, 1)))) return 80 + rc;
  // one block removed on one side: node 1 no longer lists node 0, takes node 0's colour, and block (0, 1) joins two nodes of one colour
  Graph cut = from_adjacency(grid_adjacency(4));
  cut.bcol.erase(cut.bcol.begin() + cut.bptr[1]);
  for (size_t i = 2; i < cut.bptr.size(); i++) cut.bptr[i]--;
  rdc::MgColours C;
  if (rdc::mg_colour((int64_t)cut.bptr.size() - 1, cut.bptr.data(), cut.bcol.data(), C)) return 99;
  // ghost columns (>= n) are ignored: the first 32 rows of the grid alone
  const Graph g4 = from_adjacency(grid_adjacency(4));
  if (!rdc::mg_colour(32, g4.bptr.data(), g4.bcol.data(), C) || C.nodes.size() != 32) return 98;
  return 0;
}
