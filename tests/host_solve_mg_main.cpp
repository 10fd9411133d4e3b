// Stand-alone run of the multigrid host code of rdcfes_amd/csrc/rdc_solve.h (aggregation, coarse patterns, contribution lists)
// for tools/asan_solve_mg.sh: no device, no Python.  Patterns: a 7-point grid graph, a hub (one node coupled to all others),
// a chain, isolated nodes.  Returns 0 if every hierarchy has the properties tests/test_host_solve_mg.py checks and, for 3 and 5
// unknowns per node, the device layout of mg_place fits what it measured: host buffers of exactly the measured sizes stand in
// for the two arenas, every list is copied into its slot and every other array is filled, so the sanitizer sees each write.
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

Graph grid(int n) {
  std::vector<std::vector<int32_t>> adj((size_t)n * n * n);
  auto id = [n](int i, int j, int k) { return (int32_t)((i * n + j) * n + k); };
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++)
      for (int k = 0; k < n; k++) {
        if (i + 1 < n) { adj[id(i, j, k)].push_back(id(i + 1, j, k)); adj[id(i + 1, j, k)].push_back(id(i, j, k)); }
        if (j + 1 < n) { adj[id(i, j, k)].push_back(id(i, j + 1, k)); adj[id(i, j + 1, k)].push_back(id(i, j, k)); }
        if (k + 1 < n) { adj[id(i, j, k)].push_back(id(i, j, k + 1)); adj[id(i, j, k + 1)].push_back(id(i, j, k)); }
      }
  return from_adjacency(adj);
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

// 15: the two passes disagree (the place pass does not end where the measure pass did, the measure pass set a pointer, or the
// level sizes are not those of the steps); 16: an array is not aligned; 17: it leaves its arena; 18: two arrays overlap (an
// array is smaller than what it holds), or a list did not arrive where its level points
int check_layout(const Graph& g0, const std::vector<rdc::MgLevelHost>& steps, int nv) {
  const int64_t n0 = (int64_t)g0.bptr.size() - 1;
  rdc::MgArena idx, val;
  rdc::MgDev g;
  rdc::mg_place(steps, nv, n0, g0.bptr[(size_t)n0], idx, val, g, [](void*, const void*, size_t) {});
  const size_t ibytes = idx.used, vbytes = val.used;
  if (g.ph || g.sh || g.t0 || (g.n_levels > 1 && (g.lv[1].agg || g.lv[1].val))) return 15;
  if (ibytes % rdc::MG_ALIGN || vbytes % rdc::MG_ALIGN || vbytes == 0) return 15;
  char* ibuf = ibytes ? (char*)std::aligned_alloc(rdc::MG_ALIGN, ibytes) : nullptr;
  char* vbuf = (char*)std::aligned_alloc(rdc::MG_ALIGN, vbytes);
  idx = rdc::MgArena{ibuf};
  val = rdc::MgArena{vbuf};
  rdc::mg_place(steps, nv, n0, g0.bptr[(size_t)n0], idx, val, g, [](void* at, const void* list, size_t bytes) { std::memcpy(at, list, bytes); });
  struct Span { const char* at; size_t bytes; };
  std::vector<Span> in_idx, in_val;
  auto lst = [&](const auto* at, const auto& v) { in_idx.push_back({(const char*)at, v.size() * sizeof(v[0])}); };
  auto vec = [&](double* at, int64_t doubles) {
    in_val.push_back({(const char*)at, (size_t)doubles * sizeof(double)});
    if (at) std::memset(at, 0x5a, (size_t)doubles * sizeof(double));
  };
  int rc = idx.used != ibytes || val.used != vbytes ? 15 : 0;
  if (g.n_levels != (int)steps.size() + 1 || g.lv[0].n != n0 || g.lv[0].blocks != g0.bptr[(size_t)n0]) rc = 15;
  const int64_t nn = std::max<int64_t>(n0 * nv, 1);
  vec(g.ph, nn); vec(g.sh, nn); vec(g.t0, nn);
  for (size_t l = 0; l < steps.size() && !rc; l++) {
    const rdc::MgLevelHost& L = steps[l];
    const rdc::MgLevelDev& D = g.lv[l + 1];
    if (D.n != L.n || D.blocks != (int64_t)L.bcol.size()) rc = 15;
    lst(D.agg, L.agg); lst(D.mptr, L.mptr); lst(D.member, L.member); lst(D.bptr, L.bptr); lst(D.bcol, L.bcol); lst(D.brow, L.brow);
    lst(D.cptr, L.cptr); lst(D.cidx, L.cidx); lst(D.cnode, L.cnode);
    vec(D.val, D.blocks * nv * nv); vec(D.dinv, D.n * nv * nv); vec(D.x, D.n * nv); vec(D.r, D.n * nv); vec(D.t, D.n * nv);
  }
  auto spans = [](std::vector<Span>& a, const char* base, size_t bytes) {
    for (const Span& s : a) {
      if (!s.at || (size_t)(s.at - base) % rdc::MG_ALIGN) return 16;
      if (s.at < base || s.at + s.bytes > base + bytes) return 17;
    }
    std::sort(a.begin(), a.end(), [](const Span& x, const Span& y) { return x.at < y.at; });
    for (size_t i = 1; i < a.size(); i++)
      if (a[i - 1].at + a[i - 1].bytes > a[i].at) return 18;
    return 0;
  };
  if (!rc) rc = spans(in_idx, ibuf, ibytes);
  if (!rc) rc = spans(in_val, vbuf, vbytes);
  for (size_t l = 0; l < steps.size() && !rc; l++)   // the lists arrived where the level points
    if (std::memcmp(g.lv[l + 1].cidx, steps[l].cidx.data(), steps[l].cidx.size() * 4) || std::memcmp(g.lv[l + 1].bptr, steps[l].bptr.data(), steps[l].bptr.size() * 8)) rc = 18;
  std::free(ibuf);
  std::free(vbuf);
  return rc;
}

int check(const char* name, const Graph& g) {
  std::vector<rdc::MgLevelHost> steps;
  int64_t n = (int64_t)g.bptr.size() - 1;
  if (!rdc::mg_build(n, g.bptr.data(), g.bcol.data(), steps)) return 1;
  const int64_t* bptr = g.bptr.data();
  const int32_t* bcol = g.bcol.data();
  std::printf("%s: %lld nodes", name, (long long)n);
  for (const rdc::MgLevelHost& L : steps) {
    std::printf(" -> %lld", (long long)L.n);
    if (L.n_fine != n || L.n <= 0 || L.n >= n || (int64_t)L.agg.size() != n || (int64_t)L.member.size() != n) return 2;
    for (int64_t i = 0; i < n; i++)
      if (L.agg[(size_t)i] < 0 || L.agg[(size_t)i] >= L.n) return 3;
    for (int64_t I = 0; I < L.n; I++) {
      if (L.mptr[(size_t)I + 1] <= L.mptr[(size_t)I] || L.bptr[(size_t)I + 1] <= L.bptr[(size_t)I]) return 4;
      for (int64_t m = L.mptr[(size_t)I]; m < L.mptr[(size_t)I + 1]; m++)
        if (L.agg[(size_t)L.member[(size_t)m]] != I || (m > L.mptr[(size_t)I] && L.member[(size_t)m] <= L.member[(size_t)m - 1])) return 5;
      for (int64_t k = L.bptr[(size_t)I] + 1; k < L.bptr[(size_t)I + 1]; k++)
        if (L.bcol[(size_t)k] <= L.bcol[(size_t)k - 1]) return 6;
      if (rdc::csr_diag_block(L.bptr.data(), L.bcol.data(), I) < 0) return 7;
    }
    const int64_t nblk = bptr[n], ncb = (int64_t)L.bcol.size();
    if ((int64_t)L.cidx.size() != nblk || (int64_t)L.cnode.size() != nblk || L.cptr[(size_t)ncb] != nblk || (int64_t)L.brow.size() != ncb) return 8;
    std::vector<char> seen((size_t)nblk, 0);
    for (int64_t c = 0; c < ncb; c++) {
      if (L.cptr[(size_t)c + 1] <= L.cptr[(size_t)c]) return 9;
      for (int64_t i = L.cptr[(size_t)c]; i < L.cptr[(size_t)c + 1]; i++) {
        const int64_t f = L.cidx[(size_t)i], node = L.cnode[(size_t)i];
        if (f < 0 || f >= nblk || seen[(size_t)f]++) return 10;
        if (f < bptr[node] || f >= bptr[node + 1]) return 11;
        if (L.agg[(size_t)node] != L.brow[(size_t)c] || L.agg[(size_t)bcol[f]] != L.bcol[(size_t)c]) return 12;
        if (i > L.cptr[(size_t)c] && f <= L.cidx[(size_t)i - 1]) return 13;
      }
    }
    n = L.n; bptr = L.bptr.data(); bcol = L.bcol.data();
  }
  std::printf("\n");
  for (int nv : {3, 5})
    if (int rc = check_layout(g, steps, nv)) return rc;
  if (n > rdc::MG_COARSEST_NODES && (int)steps.size() + 1 < rdc::MG_MAX_LEVELS) {   // stopped early: only if nothing merges
    rdc::MgLevelHost L;
    if (!rdc::mg_coarsen(n, bptr, bcol, L) || L.n < n) return 14;
  }
  return 0;
}

}  // namespace

int main() {
  int rc;
  if ((rc = check("grid 12^3", grid(12)))) return rc;
  if ((rc = check("hub 2000", hub(2000)))) return 20 + rc;
  if ((rc = check("chain 500", chain(500, 1)))) return 40 + rc;
  if ((rc = check("isolated 100", chain(100, 1000)))) return 60 + rc;
  if ((rc = check("one node", chain(1, 1)))) return 80 + rc;
  double d[3][3] = {{2, 0, 1}, {0, 4, 0}, {1, 0, 8}}, a[3][3] = {{1, 2, 3}, {4, 5, 6}, {7, 8, 10}}, out[3][3];
  rdc::scaled_block<3>(d, a, out);
  return out[0][0] == 9.0 && out[2][2] == 83.0 ? 0 : 99;
}
