// Stand-alone run of the block ILU(0) functions of rdcfes_amd/csrc/rdc_solve.h on patterns WITH ghost columns (ilu_build with ghosts,
// ilu_value_offset and ilu_find over the owned positions, ilu_factor_node<NV, true> through ilu_factor_host, ilu_place with a ghost
// tail) for tools/asan_solve_ilu_dist.sh: no device, no Python.  Patterns, each as one rank sees it: the two halves of a chain with
// one ghost per side; an arrow whose hub is a ghost (the owned square is a diagonal); a grid slab with a ghost layer on each side; a
// rank that owns nothing.  `colour` and `uinv` have exactly n_owned entries and the value buffer exactly nvar^2 * blocks, so the
// sanitizer sees any read of a ghost's colour or pivot and any write past the node's values.  The slots of the ghost blocks hold a
// marked NaN before the factorisation and must hold it afterwards.  Returns 0 if every factorisation finds no bad pivot, L U
// reproduces the diagonal blocks of the owned square, every private row has its ghosts last, and the same owned square given
// WITHOUT its ghost columns factors to the same bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rdcfes_amd/csrc/rdc_solve.h"

namespace {

struct Graph { int64_t n_owned; std::vector<int64_t> bptr; std::vector<int32_t> bcol; };

// rows of the first n_owned nodes of an adjacency over n_owned + ghosts nodes; every row gets its diagonal
Graph rows_of(int64_t n_owned, std::vector<std::vector<int32_t>> adj) {
  Graph g;
  g.n_owned = n_owned;
  g.bptr.push_back(0);
  for (int64_t i = 0; i < n_owned; i++) {
    adj[(size_t)i].push_back((int32_t)i);
    std::sort(adj[(size_t)i].begin(), adj[(size_t)i].end());
    adj[(size_t)i].erase(std::unique(adj[(size_t)i].begin(), adj[(size_t)i].end()), adj[(size_t)i].end());
    g.bcol.insert(g.bcol.end(), adj[(size_t)i].begin(), adj[(size_t)i].end());
    g.bptr.push_back((int64_t)g.bcol.size());
  }
  return g;
}

// the same rows without their ghost columns: the owned square as a pattern of its own
Graph owned_square(const Graph& g) {
  Graph s;
  s.n_owned = g.n_owned;
  s.bptr.push_back(0);
  for (int64_t i = 0; i < g.n_owned; i++) {
    for (int64_t k = g.bptr[(size_t)i]; k < g.bptr[(size_t)i + 1]; k++)
      if (g.bcol[(size_t)k] < g.n_owned) s.bcol.push_back(g.bcol[(size_t)k]);
    s.bptr.push_back((int64_t)s.bcol.size());
  }
  return s;
}

double value(int64_t i, int64_t j, int a, int b, int64_t len) {   // deterministic, block-diagonally dominant
  const double off = 0.25 * std::sin(1.0 + 0.37 * (double)i + 0.91 * (double)j + 1.3 * a + 2.1 * b) / (double)len;
  return i == j && a == b ? 2.0 + off : off;
}

struct Factored { rdc::IluHost H; std::vector<double> own_values, uinv; };   // own_values: per node its owned positions in private order

template <int NV>
int factor(const char* name, const Graph& g, bool ghosts, Factored& out) {
  const int64_t n = g.n_owned, blocks = g.bptr[(size_t)n];
  rdc::IluHost& H = out.H;
  int64_t where = -1;
  const int rc = rdc::ilu_build(n, g.bptr.data(), g.bcol.data(), H, &where, ghosts);
  if (rc) { std::printf("%s: ilu_build returned %d at %lld\n", name, rc, (long long)where); return 1; }
  if ((int64_t)H.col.colour.size() != n || (int64_t)H.nlow.size() != n || !(H.nown.empty() || (int64_t)H.nown.size() == n)) { std::printf("%s: list sizes\n", name); return 1; }
  uint64_t mark_bits = 0x7ff8000000c0ffeeull;
  double mark;
  std::memcpy(&mark, &mark_bits, sizeof(mark));
  double* val = (double*)std::malloc((size_t)std::max<int64_t>(blocks, 1) * NV * NV * sizeof(double));   // exactly the factor: an overrun is seen
  double* uinv = (double*)std::malloc((size_t)std::max<int64_t>(n, 1) * NV * NV * sizeof(double));      // exactly the owned pivots
  for (int64_t o = 0; o < blocks * NV * NV; o++) val[o] = mark;
  std::vector<double> keep((size_t)blocks * NV * NV);
  int fail = 0;
  for (int64_t i = 0; i < n && !fail; i++) {
    const int64_t b0 = g.bptr[(size_t)i], len = g.bptr[(size_t)i + 1] - b0, nl = H.nlow[(size_t)i];
    const int64_t own = H.nown.empty() ? len : H.nown[(size_t)i];
    if (nl >= own || H.pcol[(size_t)(b0 + nl)] != i) { std::printf("%s: node %lld: no diagonal block at its lower count\n", name, (long long)i); fail = 1; break; }
    for (int64_t p = 0; p < len; p++) {
      const int32_t j = H.pcol[(size_t)(b0 + p)];
      if ((p < own) != (j < n)) { std::printf("%s: node %lld: a ghost column among the owned positions, or the reverse\n", name, (long long)i); fail = 1; break; }
      if (p >= own) continue;
      if (rdc::ilu_find(H.pcol.data() + b0, own, H.col.colour.data(), j) != p) { std::printf("%s: ilu_find\n", name); fail = 1; break; }
      for (int a = 0; a < NV; a++)
        for (int b = 0; b < NV; b++) {
          const int64_t o = rdc::ilu_value_offset(b0, NV, own, nl, a, p, b);
          if (o < (int64_t)NV * NV * b0 || o >= (int64_t)NV * NV * (b0 + own)) { std::printf("%s: offset out of the node's owned values\n", name); fail = 1; }
          else keep[(size_t)o] = val[o] = value(i, j, a, b, own);
        }
    }
  }
  int64_t bad = 0;
  if (!fail) bad = rdc::ilu_factor_host<NV>(n, g.bptr.data(), H, val, uinv);
  if (bad) { std::printf("%s: %lld bad pivots on a dominant matrix\n", name, (long long)bad); fail = 1; }
  // (L U)_ii = sum_{k lower} L_ik U_ki + U_ii reproduces the diagonal block of the owned square; the ghost slots are untouched
  double worst = 0.0;
  for (int64_t i = 0; i < n && !fail; i++) {
    const int64_t b0 = g.bptr[(size_t)i], len = g.bptr[(size_t)i + 1] - b0, nl = H.nlow[(size_t)i];
    const int64_t own = H.nown.empty() ? len : H.nown[(size_t)i];
    for (int64_t o = (int64_t)NV * NV * (b0 + own); o < (int64_t)NV * NV * (b0 + len); o++)
      if (std::memcmp(&val[o], &mark, sizeof(mark)) != 0) { std::printf("%s: node %lld: the slot of a ghost block was written\n", name, (long long)i); fail = 1; }
    for (int a = 0; a < NV; a++)
      for (int b = 0; b < NV; b++) {
        double s = val[rdc::ilu_value_offset(b0, NV, own, nl, a, nl, b)];
        for (int64_t p = 0; p < nl; p++) {
          const int64_t k = H.pcol[(size_t)(b0 + p)], k0 = g.bptr[(size_t)k], knl = H.nlow[(size_t)k];
          const int64_t kown = H.nown.empty() ? g.bptr[(size_t)k + 1] - k0 : H.nown[(size_t)k];
          const int64_t at = rdc::ilu_find(H.pcol.data() + k0, kown, H.col.colour.data(), (int32_t)i);
          if (at <= knl) { std::printf("%s: block (%lld, %lld) is not an upper block\n", name, (long long)k, (long long)i); return 1; }
          for (int c = 0; c < NV; c++)
            s += val[rdc::ilu_value_offset(b0, NV, own, nl, a, p, c)] * val[rdc::ilu_value_offset(k0, NV, kown, knl, c, at, b)];
        }
        worst = std::max(worst, std::fabs(s - keep[(size_t)rdc::ilu_value_offset(b0, NV, own, nl, a, nl, b)]));
      }
    for (int64_t o = (int64_t)NV * NV * b0; o < (int64_t)NV * NV * (b0 + own); o++) out.own_values.push_back(val[o]);
  }
  if (!fail && !(worst <= 1e-13)) { std::printf("%s: (LU)_ii differs from A_ii by %g\n", name, worst); fail = 1; }
  out.uinv.assign(uinv, uinv + n * NV * NV);
  // placement with a ghost tail of 3 nodes: measured, then placed into host buffers of exactly the measured sizes
  if (!fail) {
    rdc::MgArena idx, arena;
    rdc::IluDev d;
    rdc::ilu_place(H, NV, n, blocks, idx, arena, d, [](void*, const void*, size_t) {}, n + 3);
    const size_t ib = idx.used, vb = arena.used;
    char* ibuf = (char*)std::malloc(std::max<size_t>(ib, 1));
    char* vbuf = (char*)std::malloc(std::max<size_t>(vb, 1));
    idx = rdc::MgArena{ibuf}; arena = rdc::MgArena{vbuf};
    rdc::ilu_place(H, NV, n, blocks, idx, arena, d, [](void* at, const void* list, size_t nb) { std::memcpy(at, list, nb); }, n + 3);
    fail = idx.used != ib || arena.used != vb || (d.nown != nullptr) != !H.nown.empty();
    if (!fail && d.nown) fail = std::memcmp(d.nown, H.nown.data(), (size_t)n * 4) != 0;
    if (!fail) {
      std::memset(d.val, 0, (size_t)blocks * NV * NV * 8);
      std::memset(d.uinv, 0, (size_t)n * NV * NV * 8);
      std::memset(d.ph, 0, (size_t)(n + 3) * NV * 8);
      std::memset(d.sh, 0, (size_t)(n + 3) * NV * 8);
      if (n) fail = std::memcmp(d.nlow, H.nlow.data(), (size_t)n * 4) != 0 || std::memcmp(d.pcol, H.pcol.data(), (size_t)blocks * 4) != 0;
    }
    std::free(ibuf); std::free(vbuf);
    if (fail) std::printf("%s: placement\n", name);
  }
  std::free(val); std::free(uinv);
  if (!fail && ghosts)
    std::printf("%s (nvar %d): %lld owned nodes, %lld blocks, %d colours, |(LU)_ii - A_ii| <= %.1e\n", name, NV, (long long)n, (long long)blocks,
                H.col.n_colours(), worst);
  return fail;
}

// the pattern with its ghost columns, and its owned square as a pattern of its own through the existing call: the same bits
template <int NV>
int check(const char* name, const Graph& g) {
  Factored with, without;
  if (factor<NV>(name, g, true, with)) return 1;
  rdc::IluHost refused;
  int64_t where = -1;
  bool any_ghost = false;
  for (int32_t j : g.bcol) any_ghost = any_ghost || j >= g.n_owned;
  if (any_ghost && rdc::ilu_build(g.n_owned, g.bptr.data(), g.bcol.data(), refused, &where) != 2) { std::printf("%s: the existing call took a ghost column\n", name); return 1; }
  if (any_ghost == with.H.nown.empty() && g.n_owned) { std::printf("%s: nown kept without ghosts, or the reverse\n", name); return 1; }
  if (factor<NV>(name, owned_square(g), false, without)) return 1;
  if (with.H.col.colour != without.H.col.colour || with.H.nlow != without.H.nlow || with.H.col.nodes != without.H.col.nodes) { std::printf("%s: lists differ from those of the owned square\n", name); return 1; }
  if (with.own_values.size() != without.own_values.size() ||
      (!with.own_values.empty() && std::memcmp(with.own_values.data(), without.own_values.data(), with.own_values.size() * 8) != 0) ||
      (!with.uinv.empty() && std::memcmp(with.uinv.data(), without.uinv.data(), with.uinv.size() * 8) != 0)) {
    std::printf("%s: the factor differs from that of the owned square\n", name);
    return 1;
  }
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  {   // a chain of 2 m nodes split in two: each half owns m nodes and sees one ghost, the neighbour across the cut
    const int32_t m = 21;
    std::vector<std::vector<int32_t>> left((size_t)m + 1), right((size_t)m + 1);
    for (int32_t i = 0; i + 1 < m; i++) { left[(size_t)i].push_back(i + 1); left[(size_t)i + 1].push_back(i); }
    left[(size_t)m - 1].push_back(m);    // local node m = the first node of the other half
    right = left;                        // ... whose own chain is the same, with its ghost at its FIRST node
    right[(size_t)m - 1].pop_back();
    right[0].push_back(m);
    bad += check<3>("left half of a chain", rows_of(m, left)) + check<5>("left half of a chain", rows_of(m, left));
    bad += check<3>("right half of a chain", rows_of(m, right)) + check<1>("right half of a chain", rows_of(m, right));
  }
  {   // an arrow whose hub is a ghost: 30 owned leaves, each coupled to itself and to the hub only
    std::vector<std::vector<int32_t>> arrow(31);
    for (int32_t i = 0; i < 30; i++) arrow[(size_t)i].push_back(30);
    bad += check<5>("arrow with a ghost hub", rows_of(30, arrow)) + check<3>("arrow with a ghost hub", rows_of(30, arrow));
  }
  {   // a slab of a grid with face diagonals: 4 owned layers of 5 x 5, one ghost layer below and one above (ghost ids behind the owned ones)
    const int n = 5, layers = 4;
    auto id = [n](int l, int i, int j) -> int32_t {   // l = -1 and l = layers are the ghost layers
      if (l >= 0 && l < layers) return (int32_t)((l * n + i) * n + j);
      return (int32_t)(layers * n * n + (l < 0 ? 0 : n * n) + i * n + j);
    };
    std::vector<std::vector<int32_t>> adj((size_t)(layers + 2) * n * n);
    auto link = [&](int32_t x, int32_t y) { adj[(size_t)x].push_back(y); adj[(size_t)y].push_back(x); };
    for (int l = -1; l <= layers; l++)
      for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
          if (l + 1 <= layers) link(id(l, i, j), id(l + 1, i, j));
          if (i + 1 < n) link(id(l, i, j), id(l, i + 1, j));
          if (j + 1 < n) link(id(l, i, j), id(l, i, j + 1));
          if (i + 1 < n && j + 1 < n) link(id(l, i, j), id(l, i + 1, j + 1));
          if (l + 1 <= layers && i + 1 < n) link(id(l, i, j), id(l + 1, i + 1, j));
        }
    const Graph slab = rows_of((int64_t)layers * n * n, adj);
    bad += check<5>("grid slab with two ghost layers", slab) + check<3>("grid slab with two ghost layers", slab);
  }
  bad += check<5>("a rank that owns nothing", rows_of(0, std::vector<std::vector<int32_t>>(4)));
  bad += check<3>("one owned node and a ghost", rows_of(1, {{1}, {0}}));
  std::printf(bad ? "FAILED\n" : "ok\n");
  return bad ? 1 : 0;
}
