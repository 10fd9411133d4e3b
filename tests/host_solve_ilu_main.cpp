// Stand-alone run of the host+device functions of the block ILU(0) (rdcfes_amd/csrc/rdc_solve.h: ilu_build, ilu_value_offset,
// ilu_find, ilu_factor_node through ilu_factor_host, ilu_place) for tools/asan_solve_ilu.sh: no device, no Python.  Patterns: a
// 7-point grid graph, a hub (one node coupled to all others, the long row), a chain, isolated nodes, one node.  Values: a
// block-diagonally dominant matrix written straight into the private layout, in a buffer of exactly nvar^2 * blocks doubles, so
// that the sanitizer sees every read and write of the factorisation.  Returns 0 if every factorisation finds no bad pivot, L U
// reproduces the diagonal blocks of the matrix (what ILU(0) guarantees on the pattern), every position is found where it lies and
// every offset stays inside the node's own values, and the placement fits what it measured.
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

double value(int64_t i, int64_t j, int a, int b, int64_t len) {   // deterministic, block-diagonally dominant
  const double off = 0.25 * std::sin(1.0 + 0.37 * (double)i + 0.91 * (double)j + 1.3 * a + 2.1 * b) / (double)len;
  return i == j && a == b ? 2.0 + off : off;
}

template <int NV>
int check(const char* name, const Graph& g) {
  const int64_t n = (int64_t)g.bptr.size() - 1, blocks = g.bptr[(size_t)n];
  rdc::IluHost H;
  int64_t where = -1;
  const int rc = rdc::ilu_build(n, g.bptr.data(), g.bcol.data(), H, &where);
  if (rc) { std::printf("%s: ilu_build returned %d at %lld\n", name, rc, (long long)where); return 1; }
  double* val = (double*)std::malloc((size_t)std::max<int64_t>(blocks, 1) * NV * NV * sizeof(double));   // exactly the factor: an overrun is seen
  double* uinv = (double*)std::malloc((size_t)std::max<int64_t>(n, 1) * NV * NV * sizeof(double));
  std::vector<double> keep((size_t)blocks * NV * NV);
  for (int64_t i = 0; i < n; i++) {
    const int64_t b0 = g.bptr[(size_t)i], len = g.bptr[(size_t)i + 1] - b0, nl = H.nlow[(size_t)i];
    if (H.pcol[(size_t)(b0 + nl)] != i) { std::printf("%s: node %lld: no diagonal block at its lower count\n", name, (long long)i); return 1; }
    for (int64_t p = 0; p < len; p++) {
      if (rdc::ilu_find(H.pcol.data() + b0, len, H.col.colour.data(), H.pcol[(size_t)(b0 + p)]) != p) { std::printf("%s: ilu_find\n", name); return 1; }
      for (int a = 0; a < NV; a++)
        for (int b = 0; b < NV; b++) {
          const int64_t o = rdc::ilu_value_offset(b0, NV, len, nl, a, p, b);
          if (o < (int64_t)NV * NV * b0 || o >= (int64_t)NV * NV * (b0 + len)) { std::printf("%s: offset out of the node's values\n", name); return 1; }
          keep[(size_t)o] = val[o] = value(i, H.pcol[(size_t)(b0 + p)], a, b, len);
        }
    }
  }
  const int64_t bad = rdc::ilu_factor_host<NV>(n, g.bptr.data(), H, val, uinv);
  if (bad) { std::printf("%s: %lld bad pivots on a dominant matrix\n", name, (long long)bad); return 1; }
  // (L U)_ii = sum_{k lower} L_ik U_ki + U_ii reproduces the diagonal block of the matrix: row k has the block (k, i) by symmetry
  double worst = 0.0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t b0 = g.bptr[(size_t)i], len = g.bptr[(size_t)i + 1] - b0, nl = H.nlow[(size_t)i];
    for (int a = 0; a < NV; a++)
      for (int b = 0; b < NV; b++) {
        double s = val[rdc::ilu_value_offset(b0, NV, len, nl, a, nl, b)];
        for (int64_t p = 0; p < nl; p++) {
          const int64_t k = H.pcol[(size_t)(b0 + p)], k0 = g.bptr[(size_t)k], klen = g.bptr[(size_t)k + 1] - k0, knl = H.nlow[(size_t)k];
          const int64_t at = rdc::ilu_find(H.pcol.data() + k0, klen, H.col.colour.data(), (int32_t)i);
          if (at <= knl) { std::printf("%s: block (%lld, %lld) is not an upper block\n", name, (long long)k, (long long)i); return 1; }
          for (int c = 0; c < NV; c++)
            s += val[rdc::ilu_value_offset(b0, NV, len, nl, a, p, c)] * val[rdc::ilu_value_offset(k0, NV, klen, knl, c, at, b)];
        }
        worst = std::max(worst, std::fabs(s - keep[(size_t)rdc::ilu_value_offset(b0, NV, len, nl, a, nl, b)]));
      }
  }
  if (!(worst <= 1e-13)) { std::printf("%s: (LU)_ii differs from A_ii by %g\n", name, worst); return 1; }
  // placement: measured, then placed into host buffers of exactly the measured sizes, every list copied into its slot
  rdc::MgArena idx, arena;
  rdc::IluDev d;
  rdc::ilu_place(H, NV, n, blocks, idx, arena, d, [](void*, const void*, size_t) {});
  const size_t ib = idx.used, vb = arena.used;
  char* ibuf = (char*)std::malloc(std::max<size_t>(ib, 1));
  char* vbuf = (char*)std::malloc(std::max<size_t>(vb, 1));
  idx = rdc::MgArena{ibuf}; arena = rdc::MgArena{vbuf};
  rdc::ilu_place(H, NV, n, blocks, idx, arena, d, [](void* at, const void* list, size_t nb) { std::memcpy(at, list, nb); });
  int fail = idx.used != ib || arena.used != vb || d.n_colours != H.col.n_colours();
  if (!fail && blocks) fail = std::memcmp(d.pcol, H.pcol.data(), (size_t)blocks * 4) != 0;
  if (!fail && n) {
    std::memset(d.val, 0, (size_t)blocks * NV * NV * 8);
    std::memset(d.uinv, 0, (size_t)n * NV * NV * 8);
    std::memset(d.ph, 0, (size_t)n * NV * 8);
    std::memset(d.sh, 0, (size_t)n * NV * 8);
    fail = std::memcmp(d.nlow, H.nlow.data(), (size_t)n * 4) != 0 || std::memcmp(d.nodes, H.col.nodes.data(), (size_t)n * 4) != 0;
  }
  std::free(ibuf); std::free(vbuf); std::free(val); std::free(uinv);
  if (fail) { std::printf("%s: placement\n", name); return 1; }
  std::printf("%s (nvar %d): %lld nodes, %lld blocks, %d colours, |(LU)_ii - A_ii| <= %.1e\n", name, NV, (long long)n, (long long)blocks,
              H.col.n_colours(), worst);
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  const Graph grid = from_adjacency(grid_adjacency(6));
  bad += check<5>("grid 6^3", grid) + check<3>("grid 6^3", grid) + check<1>("grid 6^3", grid);
  {   // the grid with the face diagonals of one direction: triangles, so more than two colours and updates of lower and upper blocks
    const int n = 5;
    std::vector<std::vector<int32_t>> adj = grid_adjacency(n);
    auto id = [n](int i, int j, int k) { return (int32_t)((i * n + j) * n + k); };
    for (int i = 0; i + 1 < n; i++)
      for (int j = 0; j + 1 < n; j++)
        for (int k = 0; k < n; k++) { adj[(size_t)id(i, j, k)].push_back(id(i + 1, j + 1, k)); adj[(size_t)id(i + 1, j + 1, k)].push_back(id(i, j, k)); }
    const Graph tri = from_adjacency(adj);
    bad += check<5>("grid 5^3 with diagonals", tri) + check<3>("grid 5^3 with diagonals", tri);
  }
  std::vector<std::vector<int32_t>> hub(300);
  for (int32_t i = 0; i < 300; i++)
    if (i != 150) { hub[150].push_back(i); hub[(size_t)i].push_back(150); }
  bad += check<5>("hub of 300", from_adjacency(hub));
  std::vector<std::vector<int32_t>> chain(41);
  for (int32_t i = 0; i + 1 < 41; i++) { chain[(size_t)i].push_back(i + 1); chain[(size_t)i + 1].push_back(i); }
  bad += check<3>("chain of 41", from_adjacency(chain));
  bad += check<5>("7 isolated nodes", from_adjacency(std::vector<std::vector<int32_t>>(7)));
  bad += check<3>("one node", from_adjacency(std::vector<std::vector<int32_t>>(1)));
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
